"""Recipe: the reference's own three index kernels, compiled by hipcc for gfx950.  Test infrastructure only.

The reference keeps its hot path as CUDA text inside Python strings (misc/ops.py).  The host snippets around them need
nvcc and Jittor's ``jt.code`` prelude; the ``__global__`` kernels themselves are plain CUDA C (``__syncthreads()`` at every
reduction step, no warp-size assumption, no texture, no library call) and hipcc compiles them as they stand.  This module

* ``extract()``  cuts the kernel text out of a reference checkout into ``oracle/_ref/*.inc`` (parsed with ``ast``, never
  imported);
* ``build()``    compiles ``oracle/ref_launch.hip`` (our launcher) around them into ``oracle/_ref/libpcl_ref_off.so``
  (``-ffp-contract=off``, the gate) and ``oracle/_ref/libpcl_ref_fast.so`` (``-ffp-contract=fast``);
* ``load()``     returns a ctypes front-end that takes torch CUDA tensors, or ``None`` when the library was not built.

``oracle/_ref/`` is never committed: it holds reference text and binaries made from it.  This file holds none of either.

    python -m oracle.ref_kernels            # what `make -C oracle _ref` runs
"""
import ast
import ctypes
import os
import re
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
LAUNCHER = os.path.join(_HERE, "ref_launch.hip")
DEFAULT_REFERENCE_DIR = "/root/reference"
REFERENCE_DIR_ENV = "PCL_ORACLE_REFERENCE_DIR"          # read by this recipe only, never by the library
CONTRACTS = ("off", "fast")

# include file -> the kernels (and device functions) that must be in it
KERNELS = {
    "fps.inc": ("__update", "furthest_point_sampling_kernel"),
    "ball_query.inc": ("query_ball_point_kernel",),
    "knn.inc": ("compute_distances", "modified_insertion_sort"),
}
_HOST_MARKER = "int block_size = #block_size;"              # first host line of the two jt.code bodies
_KNN_MARKER = "inline static bool knn_cuda_global"          # first host function of KNN's header
_KNN_DROP = ("#undef out", '#include "helper_cuda.h"')      # Jittor prelude lines of KNN's header


class ExtractError(RuntimeError):
    pass


def reference_dir(reference_dir=None):
    return reference_dir or os.environ.get(REFERENCE_DIR_ENV) or DEFAULT_REFERENCE_DIR


def lib_path(contract="off"):
    if contract not in CONTRACTS:
        raise ValueError(f"contract {contract!r}: one of {CONTRACTS}")
    return os.path.join(REF_DIR, f"libpcl_ref_{contract}.so")


def _string_constant(node, what):
    if not (isinstance(node, ast.Constant) and isinstance(node.value, str)):
        raise ExtractError(f"{what} is not a string constant")
    return node.value


def _class(tree, name):
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == name:
            return node
    raise ExtractError(f"class {name} not found in misc/ops.py")


def _class_attr(tree, cls, attr):
    for node in _class(tree, cls).body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == attr for t in node.targets):
            return _string_constant(node.value, f"{cls}.{attr}")
    raise ExtractError(f"{cls}.{attr} not found in misc/ops.py")


def _init_self_attr(tree, cls, attr):
    for fn in _class(tree, cls).body:
        if isinstance(fn, ast.FunctionDef) and fn.name == "__init__":
            for node in ast.walk(fn):
                if isinstance(node, ast.Assign) and any(
                        isinstance(t, ast.Attribute) and t.attr == attr and isinstance(t.value, ast.Name) and t.value.id == "self"
                        for t in node.targets):
                    return _string_constant(node.value, f"self.{attr} of {cls}.__init__")
    raise ExtractError(f"self.{attr} is not assigned in {cls}.__init__ of misc/ops.py")


def _cut_before_line(text, marker, what):
    """``text`` up to, not including, the line that holds ``marker``."""
    at = text.find(marker)
    if at < 0:
        raise ExtractError(f"{what}: marker {marker!r} not found")
    return text[:text.rfind("\n", 0, at) + 1]


def cut(reference_dir):
    """Reference checkout -> {include file name: kernel text}.  Raises ExtractError naming what it did not find."""
    path = os.path.join(reference_dir, "misc", "ops.py")
    if not os.path.isfile(path):
        raise ExtractError(f"{path} not found")
    with open(path, encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)
    knn = _cut_before_line(_init_self_attr(tree, "KNN", "cuda_inc"), _KNN_MARKER, "KNN.cuda_inc")
    kept = []
    for line in knn.splitlines(keepends=True):
        if line.strip() in _KNN_DROP:
            continue
        kept.append(line)
    if len(kept) != len(knn.splitlines()) - len(_KNN_DROP):
        raise ExtractError(f"KNN.cuda_inc: expected exactly the lines {_KNN_DROP} to drop")
    texts = {
        "fps.inc": _cut_before_line(_class_attr(tree, "FurthestPointSampler", "cuda_src"), _HOST_MARKER, "FurthestPointSampler.cuda_src"),
        "ball_query.inc": _cut_before_line(_class_attr(tree, "BallQueryGrouper", "cuda_src"), _HOST_MARKER, "BallQueryGrouper.cuda_src"),
        "knn.inc": "".join(kept),
    }
    for name, text in texts.items():
        missing = [k for k in KERNELS[name] if k not in kernels_in(text)]
        if missing:
            raise ExtractError(f"{name}: kernel(s) {missing} absent from the text cut out of misc/ops.py")
        if "<<<" in text or "#block_size" in text:
            raise ExtractError(f"{name}: host launch text left in the cut")
    return texts


def kernels_in(text):
    """Names of the ``__global__`` / ``__device__`` void functions defined in ``text``."""
    return re.findall(r"__(?:global|device)__\s+void\s+(\w+)\s*\(", text)


def extract(reference_dir):
    """Reference checkout -> ``oracle/_ref/{fps,ball_query,knn}.inc``; returns {file name: kernel names found in it}."""
    texts = cut(reference_dir)
    found = {name: [k for k in kernels_in(text) if k in KERNELS[name]] for name, text in texts.items()}
    os.makedirs(REF_DIR, exist_ok=True)
    for name, text in texts.items():
        out = os.path.join(REF_DIR, name)
        old = None
        if os.path.exists(out):
            with open(out, encoding="utf-8") as f:
                old = f.read()
        if old != text:                      # unchanged text keeps its time stamp: no rebuild
            with open(out, "w", encoding="utf-8") as f:
                f.write(text)
    return found


def _stale(out, inputs):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(i) for i in inputs)


def build(reference_dir_=None, force=False, verbose=True):
    """Extract + compile both libraries.  Without a reference checkout (a GPU host gets ``oracle/_ref/`` ready-made) it prints
    one line and leaves ``oracle/_ref/`` as it is.  Returns the paths of the libraries present afterwards."""
    ref = reference_dir(reference_dir_)
    if not os.path.isdir(ref):
        if verbose:
            have = [c for c in CONTRACTS if os.path.exists(lib_path(c))]
            print(f"oracle/ref_kernels: no reference tree at {ref}; oracle/_ref left as it is (libraries present: {have or 'none'})")
        return [lib_path(c) for c in CONTRACTS if os.path.exists(lib_path(c))]
    found = extract(ref)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inputs = [LAUNCHER, os.path.abspath(__file__)] + [os.path.join(REF_DIR, n) for n in found]
    for c in CONTRACTS:
        out = lib_path(c)
        if force or _stale(out, inputs):
            tmp = out + ".tmp"
            subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", f"-ffp-contract={c}",
                                   "-I", REF_DIR, "-o", tmp, LAUNCHER])
            os.replace(tmp, out)
    if verbose:
        print(f"oracle/ref_kernels: {sum(len(v) for v in found.values())} reference kernels -> "
              + ", ".join(os.path.relpath(lib_path(c), os.path.dirname(_HERE)) for c in CONTRACTS))
    return [lib_path(c) for c in CONTRACTS]


# ----------------------------------------------------------------------------- ctypes front-end (torch CUDA tensors)
class RefKernels:
    """The reference's kernels behind ``ref_launch.hip``.  Every method takes contiguous float32 CUDA tensors and launches on
    torch's current stream; shapes and layouts are the reference's (misc/ops.py)."""

    def __init__(self, path, contract):
        self.path, self.contract = path, contract
        import torch  # noqa: F401  -- before dlopen, so that the library binds to the HIP runtime that owns torch's buffers (as _lib.py)
        L = ctypes.CDLL(path)
        p, i = ctypes.c_void_p, ctypes.c_int
        L.ref_fps.argtypes = [p, p, p, i, i, i, i, p]
        L.ref_ball_query.argtypes = [p, p, p, p, i, i, i, ctypes.c_float, i, i, p]
        L.ref_knn.argtypes = [p, p, p, p, i, i, i, i, i, p]
        for f in (L.ref_fps, L.ref_ball_query, L.ref_knn):
            f.restype = ctypes.c_int
        self._L = L

    @staticmethod
    def _t(t, name):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            raise TypeError(f"{name}: a float32 CUDA tensor is required")
        return t.contiguous()

    @staticmethod
    def _stream():
        import torch
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: HIP error {rc}")

    def fps(self, xyz, m, block_size):
        """xyz [B,N,3] -> idx int32 [B,m]   (FurthestPointSampler's jt.code body, launched with ``block_size`` threads)."""
        import torch
        xyz = self._t(xyz, "xyz")
        B, N, _ = xyz.shape
        if not 1 <= m <= N:
            raise ValueError(f"m={m} must be in [1, N={N}]")
        temp = torch.empty((B, N), dtype=torch.float32, device=xyz.device)
        idx = torch.full((B, m), -1, dtype=torch.int32, device=xyz.device)
        self._check(self._L.ref_fps(xyz.data_ptr(), temp.data_ptr(), idx.data_ptr(), B, N, m, int(block_size), self._stream()), "ref_fps")
        return idx

    def ball_query(self, new_xyz, xyz, radius, nsample, block_size, fill=-1):
        """new_xyz [B,m,3], xyz [B,N,3] -> (idx int32 [B,m,nsample], cnt int32 [B,m]).  The kernel leaves the row of a query
        without a hit unwritten: such rows keep ``fill``."""
        import torch
        new_xyz, xyz = self._t(new_xyz, "new_xyz"), self._t(xyz, "xyz")
        B, m, _ = new_xyz.shape
        N = xyz.shape[1]
        if xyz.shape[0] != B or nsample < 1:
            raise ValueError("batch size mismatch or nsample < 1")
        idx = torch.full((B, m, nsample), fill, dtype=torch.int32, device=xyz.device)
        cnt = torch.full((B, m), -1, dtype=torch.int32, device=xyz.device)
        self._check(self._L.ref_ball_query(new_xyz.data_ptr(), xyz.data_ptr(), idx.data_ptr(), cnt.data_ptr(), B, N, m,
                                           ctypes.c_float(float(radius)), int(nsample), int(block_size), self._stream()), "ref_ball_query")
        return idx, cnt

    def knn(self, x_q, x_r, k):
        """KNN(k).execute(x_q [B,C,Nq], x_r [B,C,Nr]) -> idx int32 [B,k,Nq]."""
        import torch
        x_q, x_r = self._t(x_q, "x_q"), self._t(x_r, "x_r")
        B, C, Nq = x_q.shape
        Nr = x_r.shape[2]
        if x_r.shape[:2] != (B, C) or not 1 <= k <= Nr:
            raise ValueError(f"x_q {tuple(x_q.shape)} / x_r {tuple(x_r.shape)} / k={k}: equal B and C, 1 <= k <= Nr")
        dist = torch.empty((B, Nr, Nq), dtype=torch.float32, device=x_q.device)
        idx = torch.full((B, k, Nq), -1, dtype=torch.int32, device=x_q.device)
        self._check(self._L.ref_knn(x_r.data_ptr(), x_q.data_ptr(), dist.data_ptr(), idx.data_ptr(), B, C, Nr, Nq, int(k), self._stream()),
                    "ref_knn")
        return idx


_LOADED = {}


def load(contract="off"):
    """ctypes front-end of ``libpcl_ref_<contract>.so``, or ``None`` when that library was not built."""
    path = lib_path(contract)
    if not os.path.exists(path):
        return None
    if contract not in _LOADED:
        _LOADED[contract] = RefKernels(path, contract)
    return _LOADED[contract]


if __name__ == "__main__":
    build(sys.argv[1] if len(sys.argv) > 1 else None)
