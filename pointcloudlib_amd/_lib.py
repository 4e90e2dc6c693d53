"""ctypes loader of ``libpcl_hip.so`` (the C ABI declared in ``include/pcl_hip.h``).

There is NO fallback: if the HIP library is missing or a call fails, we raise.  The CPU oracle under
``oracle/`` is test infrastructure and is never imported from here.
"""
import ctypes
import functools
import os
import re
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
# PCL_HIP_SO: developer knob for timing experiments (a variant build of the same sources, csrc/Makefile EXP=n)
_SO = os.environ.get("PCL_HIP_SO") or os.path.join(_PKG, "libpcl_hip.so")
_HEADER = os.path.join(os.path.dirname(_PKG), "include", "pcl_hip.h")
_lib = None

c_void_p, c_int, c_float, c_double, c_size_t = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                                ctypes.c_double, ctypes.c_size_t)


class PclError(RuntimeError):
    pass


def so_path():
    return _SO


def build(verbose=False):
    """Compile every HIP source for gfx950 into ``pointcloudlib_amd/libpcl_hip.so`` (in-tree)."""
    cmd = ["make", "-C", os.path.join(_PKG, "csrc"), "-j8"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return _SO


# ---------------------------------------------------------------- the C ABI, read from include/pcl_hip.h
# The header is the one definition of the ABI (the compiler holds every .hip file to it).  The ctypes signatures and the
# descriptor structs are derived from its text, once, at import; tests/test_abi_cpu.py holds this parser to the host compiler.
_SCALAR = {"int": c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "float": c_float, "double": c_double, "size_t": c_size_t}
_DECL = re.compile(r"(const\s+)?(\w+)((?:\s*\*\s*(?:const\b)?)*)\s*(\w+)?\s*(?:\[([^\]]*)\])?\s*$")
_TOP = re.compile(r"""\s*(?: extern\s+"C"\s*\{ | \}
                         | typedef\s+struct\s+\w*\s*\{ (?P<body>[^{}]*) \}\s*(?P<sname>\w+)\s*;
                         | (?P<ret>[\w\s*]+?) \b(?P<fname>\w+)\s*\( (?P<params>[^;{}]*) \)\s*; )""", re.X)


def parse_abi(text, origin=_HEADER):
    """The declarations of an ABI header -> ({function: (restype, [argtypes])}, {struct: ctypes.Structure}, {macro: int}).

    Every pointer is ``c_void_p`` except ``const char*`` (``c_char_p``).  Strict: text that is no function declaration,
    ``typedef struct``, preprocessor line or ``extern "C"`` bracket raises, and so does a type outside ``_SCALAR``."""
    def fail(where, what):
        raise PclError(f"{origin}: {where}: {what}")

    def declarator(decl, where):                   # ``const float* const* W`` | ``int32_t c[PCL_N + 1]`` -> (name, type | None for void)
        m = None if "(" in decl or ":" in decl else _DECL.match(decl.strip())
        if m is None:
            fail(where, f"cannot type `{decl.strip()}` (function pointers and bit-fields are not part of the ABI)")
        const, base, stars, name, dim = m.groups()
        if stars:
            if base not in _SCALAR and base not in structs and base not in ("void", "char"):
                fail(where, f"unknown type `{base}`")
            t = ctypes.c_char_p if const and base == "char" and stars.strip() == "*" else c_void_p
        elif base == "void":
            t = None
        else:
            t = _SCALAR.get(base) or structs.get(base) or fail(where, f"unknown type `{base}`")
        if dim is not None:
            try:
                t = t * sum(int(x) if x.strip().isdigit() else defines[x.strip()] for x in dim.split("+"))
            except (KeyError, TypeError):
                fail(where, f"cannot size `{decl.strip()}`")
        return name, t

    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    loose = set(re.findall(r"\b(pcl_[a-z0-9_]+)\s*\(", text))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    sigs, structs, pos = {}, {}, 0
    while text[pos:].strip():
        m = _TOP.match(text, pos)
        if m is None:
            fail("declaration", f"cannot parse `{' '.join(text[pos:].split())[:100]}`")
        pos = m.end()
        if m["sname"]:
            fields = []
            for stmt in filter(str.strip, m["body"].split(";")):           # ``int32_t K, N, bn_mode`` repeats the base type
                first, *more = stmt.split(",")
                base = re.match(r"\s*(?:const\s+)?\w*", first)[0]
                for decl in [first] + [f"{base} {d}" for d in more]:
                    name, t = declarator(decl, m["sname"])
                    if name is None or t is None:
                        fail(m["sname"], f"`{decl.strip()}` is no field")
                    fields.append((name, t))
            structs[m["sname"]] = type(m["sname"], (ctypes.Structure,), {"_fields_": fields})
        elif m["fname"]:
            args = []
            for decl in [] if m["params"].strip() in ("", "void") else m["params"].split(","):
                t = declarator(decl, m["fname"])[1]
                if t is None or issubclass(t, (ctypes.Structure, ctypes.Array)):
                    fail(m["fname"], f"`{decl.strip()}` is neither a scalar nor a pointer")
                args.append(t)
            sigs[m["fname"]] = (declarator(m["ret"], m["fname"])[1], args)
    if loose != set(sigs):
        fail("declaration", f"the grammar missed or misread {sorted(loose ^ set(sigs))}")
    return sigs, structs, defines


def _read_header():
    try:
        with open(_HEADER) as f:
            return f.read()
    except OSError as e:
        raise PclError(f"{_HEADER} is needed at run time (the ctypes signatures are derived from it): {e}") from None


_SIGS, _STRUCTS, _DEFINES = parse_abi(_read_header())


def declared_symbols():
    """Every function name ``include/pcl_hip.h`` declares (used by the symbol-export test)."""
    return sorted(_SIGS)


def struct(name):
    """The ``ctypes.Structure`` of a ``typedef struct`` of the header (one class object per name)."""
    return _STRUCTS[name]


def define(name):
    """An integer ``#define`` of the header (``PCL_STACK_MAX_LAYERS``, ...)."""
    return _DEFINES[name]


# ---------------------------------------------------------------- lab switches (csrc/common.h: LabSwitches; the table in DESIGN.md section 1)
# The environment is read HERE (host side) and handed over as C calls -- the library itself reads none.  One row per variable:
# (variable, setter, its arguments), an argument being a number (-1: "leave as is") or how the variable's text becomes one.
def _on(text):
    return int(text != "0")


_ENV_SWITCHES = (("PCL_FWD_RES", "pcl_set_kernel_paths", (_on, -1, -1)),
                 ("PCL_NARROW", "pcl_set_kernel_paths", (-1, _on, -1)),
                 ("PCL_FUSED_BWD", "pcl_set_kernel_paths", (-1, -1, _on)),
                 ("PCL_SIDE_DW", "pcl_set_stack_overlap", (_on, -1)),
                 ("PCL_BWD_W_ROWS", "pcl_set_pointconv_paths", (_on,)),
                 ("PCL_SCATTER", "pcl_set_scatter_form", (_on,)),
                 ("PCL_BWD_PAIR", "pcl_set_bwd_pair", (_on,)),
                 ("PCL_FB_TWO", "pcl_set_fb_two_images", (_on,)),
                 ("PCL_FEWROW", "pcl_set_fewrow_backward", (_on,)),
                 ("PCL_DW_GX", "pcl_set_dw_tuning", (int,)))
# Several size queries answer by the switches, so whatever the host keeps of such an answer is dropped whenever a setter runs:
# lib() puts a Python function over every setter of the header that calls it and then the registered invalidators.  Setters are
# never called on a launch path.
_SWITCH_SETTERS = [n for n in _SIGS if n.startswith("pcl_set_") or n == "pcl_frag_set_tuning"]
_INVALIDATORS = []


def on_switch_change(fn):
    """Register ``fn()`` to run after every lab-switch setter (a cache whose contents depend on a switch registers its clear)."""
    _INVALIDATORS.append(fn)
    return fn


def _invalidating(setter):
    def set_and_invalidate(*args):
        setter(*args)
        for fn in _INVALIDATORS:
            fn()
    return set_and_invalidate


def lib():
    """The loaded library; raises PclError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise PclError(f"{_SO} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # PyTorch-ROCm bundles its own libamdhip64 (same SONAME).  Kernels launched here must run in the SAME HIP
        # runtime instance that owns torch's device buffers and streams, so torch's copy has to be the one the
        # dynamic linker resolves for us: load torch first, then dlopen (otherwise /opt/rocm's copy is pulled in as
        # a second runtime and every launch fails with hipErrorNoDevice).
        import torch  # noqa: F401
        L = ctypes.CDLL(_SO)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        for name in _SWITCH_SETTERS:
            setattr(L, name, _invalidating(getattr(L, name)))
        for var, setter, args in _ENV_SWITCHES:
            if os.environ.get(var) is not None:
                getattr(L, setter)(*(a(os.environ[var]) if callable(a) else a for a in args))
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().pcl_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise PclError(f"{what}: rc={rc}: {msg}")


# ---------------------------------------------------------------- per-kernel event timing (bench.py)
PROFILER = None   # set to a KernelTimer by bench.py; None in normal operation (zero overhead)


# entry points that launch exactly one GEMM-family kernel (plus, for dW, small reductions that are not the kernel of interest)
KERNEL_TIMED = {"pcl_linear_fwd_rows_f32", "pcl_linear_fwd_f32", "pcl_linear_bwd_dx_rows_f32", "pcl_linear_bwd_dx_f32",
                "pcl_linear_bwd_dw_rows_f32", "pcl_linear_bwd_dw_f32", "pcl_linear_bwd_fused_rows_f32",
                "pcl_linear_bwd_dw_plain_f32", "pcl_frag_linear_bwd_dx_f32", "pcl_frag_linear_fwd_f32",
                "pcl_knn_f32", "pcl_knn_fma_f32", "pcl_knn_nk_f32"}      # (k-NN: the fused kernel; the two-pass form arms nothing and is not recorded)
_hip = None


def _hiprt():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        _hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        _hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
    return _hip


class _HipEventPair:
    """Two timing-enabled hipEvent_t owned by this object."""

    def __init__(self):
        h = _hiprt()
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        if h.hipEventCreate(ctypes.byref(a)) or h.hipEventCreate(ctypes.byref(b)):
            raise PclError("hipEventCreate failed")
        self.start, self.stop = a, b

    def elapsed_ms(self):
        ms = ctypes.c_float()
        rc = _hiprt().hipEventElapsedTime(ctypes.byref(ms), self.start, self.stop)
        if rc:                                       # (this call launched no kernel of the timed families: the events were never recorded)
            _hiprt().hipGetLastError()               # the runtime keeps the code as its "last error": torch's next check would raise it
            return None
        return ms.value

    def __del__(self):
        try:
            _hiprt().hipEventDestroy(self.start); _hiprt().hipEventDestroy(self.stop)
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass


class KernelTimer:
    """Brackets selected C-ABI calls with HIP events on the stream they are launched on (torch's current
    stream) and accumulates per-entry-point time plus the algorithmic bytes/flops the caller states."""

    def __init__(self, names=None, tags=None, max_records=None, inner=None):
        """``inner`` = (entry point, launch tag, algo_bytes, algo_flops): time ONE kernel inside the per-stack entry points
        (csrc/stack.hip) -- the launch whose tag matches gets the armed events (pcl_time_tagged_launch); the record is filed
        under (entry point, launch tag) with the stated algorithmic bytes / flops per launch."""
        self.inner = inner
        if inner is not None:
            names = ["pcl_mlp_stack_fwd_f32", "pcl_mlp_stack_bwd_f32"]
            tags = None
        self.names = None if names is None else set(names)
        self.tags = None if tags is None else set(tags)          # restrict to these launch shapes
        self.max_records = max_records                           # per (name, tag): timing events perturb the stream
        self.records = {}                                        # (each record is a marker packet), so bound them
        self.order = []                                          # (name, tag) in launch order
        self.calls = 0                                           # every C-ABI call seen, recorded or not

    def want(self, name, tag=None):
        self.calls += 1
        if self.names is not None and name not in self.names:
            return False
        if self.tags is not None and tag is not None and tag not in self.tags:
            return False
        if self.inner is not None:
            return self.max_records is None or len(self.records.get(self.inner[:2], ())) < 3 * self.max_records
        if self.max_records is not None and tag is not None:
            return len(self.records.get((name, tag), ())) < self.max_records
        return True

    def begin(self, name=None):
        if self.inner is not None:
            pair = _HipEventPair()
            lib().pcl_time_tagged_launch(pair.start, pair.stop, self.inner[1].encode())
            return pair
        if name in KERNEL_TIMED:
            # the GEMM-family kernel this entry point launches reports its own begin / end timestamps into two events
            # (pcl_time_next_launch): the same interval rocprofv3's kernel trace shows, without the two marker packets'
            # dispatch gaps (~20 us around a 0.2 ms kernel)
            pair = _HipEventPair()
            lib().pcl_time_next_launch(pair.start, pair.stop)
            return pair
        import torch
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, name, tag, start, algo_bytes, algo_flops):
        if self.inner is not None:
            name, tag, algo_bytes, algo_flops = self.inner
        if isinstance(start, _HipEventPair):
            lib().pcl_time_next_launch(None, None)                # (disarm: a call that launched no such kernel)
            ev = None
        else:
            import torch
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
        self.records.setdefault((name, tag), []).append((start, ev, algo_bytes, algo_flops))
        fam = ""
        if isinstance(start, _HipEventPair) and self.inner is None:      # which kernel the entry point chose (tools/pmc_traffic.py)
            fam = (lib().pcl_last_launch_kernel() or b"").decode().strip("()").split("<")[0]
        self.order.append((name, tag, fam))

    def summary(self):
        """{(name, tag): dict(launches, avg_ms, algo_bytes, algo_flops)} -- call after a device sync."""
        out = {}
        def val(v):            # algorithmic bytes/flops may depend on a device-resident row count: resolved here,
            return v() if callable(v) else v          # after the timed region, never inside it

        for key, recs in self.records.items():
            ms = [s.elapsed_ms() if e is None else s.elapsed_time(e) for s, e, _, _ in recs]
            recs = [r for r, m in zip(recs, ms) if m is not None]
            ms = [m for m in ms if m is not None]
            if not ms:
                continue
            ab = [val(r[2]) for r in recs]
            af = [val(r[3]) for r in recs]
            out[key] = {"launches": len(recs), "avg_ms": sum(ms) / len(ms), "total_ms": sum(ms),
                        "algo_bytes": sum(ab) / len(ab), "algo_flops": sum(af) / len(af)}
        return out


@functools.lru_cache(maxsize=None)
def size_query(name, *ints):
    """Pure size functions of the ABI (``pcl_mlp_stat_rows``, ``pcl_linear_bwd_dw_workspace_bytes``, ...): asked once per shape."""
    return getattr(lib(), name)(*ints)


on_switch_change(size_query.cache_clear)


_FN = {}            # entry point name -> bound ctypes function


def call(name, *args, algo_bytes=0, algo_flops=0, tag=""):
    """Invoke one C-ABI entry point; raises on a non-zero return code."""
    fn = _FN.get(name)
    if fn is None:
        fn = _FN[name] = getattr(lib(), name)
    prof = PROFILER
    if prof is None:                               # normal operation: straight through
        rc = fn(*args)
    else:
        tag = tag or (name if callable(algo_bytes) else f"{algo_bytes}")
        if prof.want(name, tag):
            start = prof.begin(name)
            rc = fn(*args)
            prof.end(name, tag, start, algo_bytes, algo_flops)
        else:
            rc = fn(*args)
    if rc != 0:
        check(rc, name)
