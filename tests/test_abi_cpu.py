"""The ctypes view of the C ABI is derived from include/pcl_hip.h (pointcloudlib_amd/_lib.py::parse_abi).  These tests hold that
parser to the host C++ compiler: a generated program includes the header and prints, from the compiler's own types, every
function's return / parameter classes and every descriptor struct's sizeof / offsetof.  No HIP, no linking, no GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from pointcloudlib_amd import _lib

CLASS = {"v": None, "i": ctypes.c_int, "f": ctypes.c_float, "d": ctypes.c_double, "z": ctypes.c_size_t, "p": ctypes.c_void_p,
         "s": ctypes.c_char_p}
# one class letter per C type; a by-value type without a letter (a struct, a 64-bit integer) does not compile
PROBE_HEAD = r"""
#include <cstddef>
#include <cstdio>
#include "pcl_hip.h"
template <class T> struct K;
template <> struct K<void> { static constexpr char c = 'v'; };
template <> struct K<int> { static constexpr char c = 'i'; };
template <> struct K<float> { static constexpr char c = 'f'; };
template <> struct K<double> { static constexpr char c = 'd'; };
template <> struct K<size_t> { static constexpr char c = 'z'; };
template <class T> struct K<T*> { static constexpr char c = 'p'; };
template <> struct K<const char*> { static constexpr char c = 's'; };
template <class F> struct Sig;                      // decltype(&f) names no symbol: the program links against nothing
template <class R, class... A> struct Sig<R (*)(A...)> {
    static void print(const char* name) {
        std::printf("F %s %c", name, K<R>::c);
        ((void)std::printf(" %c", K<A>::c), ...);
        std::printf("\n");
    }
};
int main() {
"""


def _header_text():
    with open(_lib._HEADER) as f:
        return f.read()


def _layout(cls):
    return ctypes.sizeof(cls), [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_]


def _disagreements(parsed, probe):
    """Names of the functions and structs on which a parse_abi() result differs from what the compiler printed."""
    sigs, structs, _ = parsed
    fns, layouts = probe
    bad = {n for n in set(fns) | set(sigs) if fns.get(n) != sigs.get(n)}
    bad |= {n for n in set(layouts) | set(structs) if n not in structs or layouts.get(n) != _layout(structs[n])}
    return sorted(bad)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("clang++", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("abi_probe")
    names = sorted(set(re.findall(r"\b(pcl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S))))
    body = [f'    Sig<decltype(&{n})>::print("{n}");' for n in names]
    for s, cls in _lib._STRUCTS.items():
        body.append(f'    std::printf("S {s} %zu\\n", sizeof({s}));')
        body += [f'    std::printf("O {s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof({s}::{f}));' for f, _ in cls._fields_]
    src = tmp / "abi_probe.cpp"
    src.write_text(PROBE_HEAD + "\n".join(body) + "\n    return 0;\n}\n")
    subprocess.run([cxx, "-std=c++17", "-I", os.path.dirname(_lib._HEADER), str(src), "-o", str(tmp / "abi_probe")], check=True)
    out = subprocess.run([str(tmp / "abi_probe")], check=True, capture_output=True, text=True).stdout
    fns, layouts = {}, {}
    for kind, name, *rest in map(str.split, out.splitlines()):
        if kind == "F":
            fns[name] = (CLASS[rest[0]], [CLASS[c] for c in rest[1:]])
        elif kind == "S":
            layouts[name] = (int(rest[0]), [])
        else:
            layouts[name][1].append((rest[0], int(rest[1]), int(rest[2])))
    assert len(fns) == len(names)
    return fns, layouts


def test_parser_agrees_with_the_compiler(probe):
    fns, layouts = probe
    assert len(fns) == len(_lib._SIGS) >= 148
    assert sorted(layouts) == sorted(_lib._STRUCTS) and len(layouts) >= 4
    assert _disagreements((_lib._SIGS, _lib._STRUCTS, None), probe) == []
    for n in fns:                                                   # (spelled out: the message names the entry and both readings)
        assert _lib._SIGS[n] == fns[n], n
    for n in layouts:
        assert _layout(_lib.struct(n)) == layouts[n], n
    assert _lib.struct("pcl_mlp_stack_t") is _lib.struct("pcl_mlp_stack_t")
    assert ctypes.sizeof(_lib.struct("pcl_mlp_stack_t")) == 896 and ctypes.sizeof(_lib.struct("pcl_fc_head_t")) == 544
    assert (_lib.define("PCL_STACK_MAX_LAYERS"), _lib.define("PCL_HEAD_MAX_LAYERS"), _lib.define("PCL_EINVAL")) == (8, 4, -1)


def test_comparison_names_a_wrong_type_a_dropped_parameter_and_swapped_fields(probe):
    """The comparison has teeth: one in-memory edit of the header's text each, parsed and held against the compiler's reading of
    the header as it is."""
    text = _header_text()
    edits = {
        "pcl_knn_f32": (r"(int pcl_knn_f32\([^;]*?)size_t workspace_bytes", r"\1int workspace_bytes"),
        "pcl_ball_query_f32": (r"(int pcl_ball_query_f32\([^;]*?)int nsample,", r"\1"),
        "pcl_mlp_stack_t": (r"const int32_t\* idx;(\s*)const int32_t\* cnt;", r"const int32_t* cnt;\1const int32_t* idx;"),
    }
    for name, (pattern, repl) in edits.items():
        edited, n = re.subn(pattern, repl, text)
        assert n == 1 and edited != text, name
        assert _disagreements(_lib.parse_abi(edited), probe) == [name]


def test_parser_is_strict(monkeypatch):
    parse, E = _lib.parse_abi, _lib.PclError
    c_int, P, S = ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p
    # what it accepts
    sigs, structs, defines = parse("""
        #define PCL_M 3
        #define PCL_NEG (-2)   /* comment */
        typedef struct pcl_in_t { const float* p; float q; } pcl_in_t;
        typedef struct pcl_out_t {
            int32_t a, b, c;        /* three fields */
            uint64_t x[PCL_M + 1];
            pcl_in_t layer[PCL_M];
            void* tail;
        } pcl_out_t;
        int pcl_f(void);
        const char* pcl_g(const char* tag, char* buf, const float* const* W, size_t n, double d, float /* inline */ f);
        void pcl_h(const pcl_out_t* desc, int32_t* const* idx_out);
    """)
    assert defines == {"PCL_M": 3, "PCL_NEG": -2}
    assert sigs == {"pcl_f": (c_int, []), "pcl_g": (S, [S, P, P, ctypes.c_size_t, ctypes.c_double, ctypes.c_float]),
                    "pcl_h": (None, [P, P])}
    assert _layout(structs["pcl_in_t"]) == (16, [("p", 0, 8), ("q", 8, 4)])
    assert _layout(structs["pcl_out_t"]) == (104, [("a", 0, 4), ("b", 4, 4), ("c", 8, 4), ("x", 16, 32), ("layer", 48, 48), ("tail", 96, 8)])
    out = structs["pcl_out_t"]()
    out.layer[2].q, out.x[3] = 1.5, 2 ** 63
    assert (out.layer[2].q, out.x[3]) == (1.5, 2 ** 63)
    # what it refuses, naming the declaration
    struct_s = "typedef struct pcl_s_t { int32_t a; } pcl_s_t;"
    for text, what in [
            ("int pcl_f(foo_t x);", r"pcl_f: unknown type `foo_t`"),
            ("int pcl_f(const foo_t* x);", r"pcl_f: unknown type `foo_t`"),
            ("foo_t pcl_f(int x);", r"pcl_f: unknown type `foo_t`"),
            ("int pcl_f(unsigned int x);", r"pcl_f: cannot type `unsigned int x`"),
            ("int pcl_f(char c);", r"pcl_f: unknown type `char`"),
            ("int pcl_f(void (*cb)(int), void* stream);", r"pcl_f: cannot type `void \(\*cb\)\(int\)`"),
            (struct_s + " int pcl_f(pcl_s_t s);", r"pcl_f: `pcl_s_t s` is neither a scalar nor a pointer"),
            ("int pcl_f(int v[4]);", r"pcl_f: `int v\[4\]` is neither a scalar nor a pointer"),
            ("typedef struct pcl_s_t { int32_t a : 3; } pcl_s_t;", r"pcl_s_t: cannot type `int32_t a : 3`"),
            ("typedef struct pcl_s_t { bar_t a; } pcl_s_t;", r"pcl_s_t: unknown type `bar_t`"),
            ("typedef struct pcl_s_t { int32_t a[PCL_N]; } pcl_s_t;", r"pcl_s_t: cannot size `int32_t a\[PCL_N\]`"),
            ("typedef struct pcl_s_t { struct { int32_t a; } in; } pcl_s_t;", r"cannot parse `typedef struct pcl_s_t"),
            ("int pcl_f(int a) { return a; }", r"cannot parse `int pcl_f\(int a\)"),
            ("int pcl_f(int a); int x;", r"cannot parse `int x;`"),
            ("int PCL_F(int a);", r"missed or misread \['PCL_F'\]"),                       # the loose scan and the grammar disagree
            ("#define pcl_m(a) \\\n  pcl_f(a)\nint pcl_f(int a);", r"pcl_f: cannot type `a\)"),
    ]:
        with pytest.raises(E, match=what):
            parse(text)
    # the header is needed at run time
    monkeypatch.setattr(_lib, "_HEADER", os.path.join(os.path.dirname(_lib._HEADER), "no_such_header.h"))
    with pytest.raises(E, match=r"no_such_header\.h is needed at run time"):
        _lib._read_header()
