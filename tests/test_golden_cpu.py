"""CPU: the oracle reproduces the committed fixtures; the C-ABI library loads and exports every symbol the
header declares (no compute calls without a GPU)."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_small_cases_match_oracle(oracle):
    g = np.load(os.path.join(GOLD, "small_cases.npz"))
    names = sorted({k.split(".")[0] for k in g.files if k.endswith(".xyz")})
    assert names
    for name in names:
        pts = g[f"{name}.xyz"]
        N = pts.shape[1]
        m = max(2, N // 3)
        for S in (1, 2, 4, 8, 16):
            assert np.array_equal(oracle.fps(pts, m, block_size=S), g[f"{name}.fps_S{S}"]), (name, S)
        _, new_xyz = oracle.fps(pts, m, block_size=1, return_xyz=True)
        for key in [k for k in g.files if k.startswith(f"{name}.bq_r")]:
            r, ns = re.match(r".*bq_r([0-9.]+)_ns(\d+)", key).groups()
            assert np.array_equal(oracle.ball_query(new_xyz, pts, float(r), int(ns)), g[key]), key
    for k in (1, 7, 33):
        assert np.array_equal(oracle.knn(g["knn.q"], g["knn.r"], k), g[f"knn.k{k}"])


def test_full_size_digests_match_oracle(oracle):
    from pointcloudlib_amd import synth
    big = json.load(open(os.path.join(GOLD, "full_size_digests.json")))
    c = big["cfg2_N1024"]
    pts = synth.gauss_ball(c["B"], c["N"], c["seed"])
    assert sha(pts) == c["xyz_sha"], "synthetic generator changed"
    i1, x1 = oracle.fps(pts, 512, block_size=c["tie_stride"], return_xyz=True)
    assert sha(i1) == c["fps1_sha"]
    assert sha(oracle.ball_query(x1, pts, 0.2, 64)) == c["bq1_sha"]


def test_capi_exports_every_declared_symbol():
    from pointcloudlib_amd import _lib
    so = _lib.so_path()
    assert os.path.exists(so), "libpcl_hip.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(so)
    declared = _lib.declared_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/pcl_hip.h but not exported"
    assert set(declared) == set(_lib._SIGS), "ctypes signature table out of sync with the header"
    lib = _lib.lib()
    assert lib.pcl_version() >= 100
    assert [lib.pcl_optimal_block(b) for b in (1, 2, 3, 8, 16, 32, 55)] == [1, 1, 2, 4, 4, 8, 16]


def test_capi_argument_validation_needs_no_gpu():
    """Argument errors are detected on the host before any launch: negative code + message."""
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert lib.pcl_fps_f32(None, 1, 8, 4, 1, 1e-3, None, None, None, None) == -1
    assert b"null" in lib.pcl_last_error()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pcl_fps_f32(p, 1, 8, 9, 1, 1e-3, None, p, None, None) == -1         # m > N
    assert lib.pcl_fps_f32(p, 1, 8, 4, 3, 1e-3, None, p, None, None) == -1         # tie_stride not a power of two
    assert lib.pcl_knn_f32(p, p, 1, 3, 8, 8, 9, p, None, 0, None) == -1            # k > Nr
    assert lib.pcl_knn_workspace_bytes(2, 3, 8, 16, 2) == 0                        # fused distance + select: no [Nq, Nr] matrix
    assert lib.pcl_knn_workspace_bytes(2, 3, 4096, 4096, 20) == 0
    assert lib.pcl_knn_workspace_bytes(2, 64, 1024, 1024, 20) == 0
    assert lib.pcl_knn_workspace_bytes(2, 3, 5000, 16, 2) == 2 * 5000 * 16 * 4     # beyond 4096 references: two passes
    assert lib.pcl_knn_f32(p, p, 1, 3, 5000, 8, 2, p, None, 0, None) == -4         # workspace too small


def test_ops_reject_cpu_tensors():
    import torch
    from pointcloudlib_amd.misc import ops
    x = torch.zeros(1, 8, 3)
    for fn in (lambda: ops.furthest_point_sample(x, 4), lambda: ops.ball_query(x, x, 0.1, 2),
               lambda: ops.knn_indices(x.transpose(1, 2), x.transpose(1, 2), 2)):
        try:
            fn()
        except RuntimeError as e:
            assert "GPU" in str(e)
        else:
            raise AssertionError("CPU tensor accepted: the HIP path must fail loudly")


def test_mlp_has_no_silent_cpu_path():
    """PointwiseMLP's default backend is the HIP path and must refuse CPU tensors; the package ships NO other implementation --
    a backend name nobody registered raises; the plain-PyTorch composite is test infrastructure (oracle/torch_backend.py) and
    runs only when a test imports it AND names it."""
    import subprocess
    import sys
    import torch
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    code = ("import torch; from pointcloudlib_amd.misc.layers import PointwiseMLP, _REFERENCE_BACKENDS\n"
            "assert not _REFERENCE_BACKENDS, 'the package registered a reference backend by itself'\n"
            "m = PointwiseMLP([4, 8]); m.backend = 'torch'\n"
            "try:\n    m(torch.randn(2, 5, 4))\nexcept RuntimeError as e:\n    assert 'not part of pointcloudlib_amd' in str(e)\n"
            "else:\n    raise SystemExit('unregistered backend ran')\n")
    root = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)
    import oracle.torch_backend  # noqa: F401
    m = PointwiseMLP([4, 8])
    x = torch.randn(2, 5, 4)
    try:
        m(x)
    except RuntimeError as e:
        assert "GPU" in str(e)
    else:
        raise AssertionError("CPU tensor accepted by the default (HIP) backend")
    m.backend = "torch"
    assert m(x).shape == (2, 5, 8)


def test_new_paths_refuse_cpu_tensors():
    """The fused head, EdgeConv, PointConv contraction and folded-grouping paths have no CPU route either."""
    import pytest
    import torch
    from torch import nn
    from pointcloudlib_amd.misc.head import head_layer
    from pointcloudlib_amd.misc.edgeconv import edge_conv
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.misc.pointconv_utils import pointconv_contract
    with pytest.raises(RuntimeError):
        head_layer(torch.randn(4, 8), nn.Linear(8, 3))
    with pytest.raises(RuntimeError):
        edge_conv(PointwiseMLP([6, 8], slope=0.2), torch.randn(1, 5, 3), torch.zeros(1, 5, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        pointconv_contract(torch.randn(1, 2, 3, 4), torch.rand(1, 2, 3, 1), torch.randn(1, 2, 3, 16))
    with pytest.raises(RuntimeError):
        PointwiseMLP([6, 8, 8]).forward_grouped(torch.randn(1, 9, 3), torch.randn(1, 2, 3), torch.randn(1, 9, 3),
                                                torch.zeros(1, 2, 4, dtype=torch.int32), torch.ones(1, 2, dtype=torch.int32),
                                                torch.zeros(3, dtype=torch.int32))


def test_sa_level_fixture_is_reproduced_by_the_restatement():
    """tests/golden/sa_level.npz: (input, weights) -> (idx, grouped, pooled) of one set-abstraction level."""
    import torch
    from oracle.cpu_model import sa_module_cpu
    g = np.load(os.path.join(GOLD, "sa_level.npz"))
    T = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt)
    for dt, key, tol in ((torch.float64, "pooled_f64", 1e-12), (torch.float32, "pooled_f32", 1e-5)):
        nx, y, aux = sa_module_cpu(T(g["xyz"], dt), T(g["feat"], dt), [T(g[f"w{i}"], dt) for i in range(3)],
                                   [T(g[f"gamma{i}"], dt) for i in range(3)], [T(g[f"beta{i}"], dt) for i in range(3)],
                                   int(g["n_points"]), float(g["radius"]), int(g["n_samples"]), int(g["tie_stride"]), return_aux=True)
        assert np.array_equal(aux["fps_idx"], g["fps_idx"]) and np.array_equal(aux["bq_idx"], g["bq_idx"])
        assert np.array_equal(aux["grouped"].float().numpy(), g["grouped"])
        assert np.abs(y.double().numpy() - g[key]).max() <= tol
    # the fp32 evaluation is within 1e-5 of the fp64 one (the tolerance the HIP path is held to)
    assert np.abs(g["pooled_f32"].astype(np.float64) - g["pooled_f64"]).max() <= 1e-5 * max(1.0, np.abs(g["pooled_f64"]).max())


def test_host_only_switches_roundtrip():
    """pcl_set_matrix_form / pcl_set_kernel_paths / pcl_set_fps_tuning are host-side state (no GPU needed): set, read back, restore."""
    import ctypes
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pointcloudlib_amd", "libpcl_hip.so")
    if not os.path.exists(so):
        pytest.skip("libpcl_hip.so not built")
    L = ctypes.CDLL(so)
    L.pcl_get_matrix_form.restype = ctypes.c_int
    assert L.pcl_get_matrix_form() == 0                       # the fp32 MFMA form is the default
    for form in (1, 2, 3, 2 | (64 << 8), 0):
        L.pcl_set_matrix_form(form)
        assert L.pcl_get_matrix_form() == (form & 7)
    L.pcl_set_kernel_paths(0, 0, 0)
    L.pcl_set_kernel_paths(-1, -1, -1)                        # negative: leave as is
    L.pcl_set_kernel_paths(1, 1, 1)
    L.pcl_set_fps_tuning(256, 0)
    L.pcl_set_fps_tuning(0, 0)


def test_round5_entry_points_validate_on_the_host():
    """The round-5 entry points (optimiser step, few-row backward, the scatter as a gather, lab switches): argument errors and size
    queries need no GPU; the switches read back and default to what DESIGN section 10 says."""
    import ctypes
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pcl_sgd_momentum_f32(None, None, None, None, 3, 0.1, 0.9, 0.0, 0.0, None) == -1
    assert lib.pcl_sgd_momentum_f32(p, p, p, p, 0, 0.1, 0.9, 0.0, 0.0, None) == 0            # no tensors: nothing launched
    assert lib.pcl_bn_bwd_dy_supported(4096, 1024) == 1 and lib.pcl_bn_bwd_dy_supported(4096, 259) == 0
    assert lib.pcl_get_fewrow_backward() == 0 and lib.pcl_get_stack_overlap() == 0            # measured, not faster: off by default
    lib.pcl_set_fewrow_backward(1)
    assert lib.pcl_mlp_fewrow_layer(4096, 1024, 512, 0) == 1 and lib.pcl_mlp_fewrow_layer(100000, 1024, 512, 0) == 0
    assert lib.pcl_mlp_fewrow_layer(4096, 128, 64, 0) == 0                                    # a shape the fused dX + dW kernel has
    lib.pcl_set_fewrow_backward(0)
    assert lib.pcl_mlp_fewrow_layer(4096, 1024, 512, 0) == 0
    assert lib.pcl_linear_bwd_dw_plain_workspace_bytes(4096, 1024, 512) % (1024 * 512 * 4) == 0
    assert lib.pcl_group_rows_transpose_supported(512, 128, 64) == 1 and lib.pcl_group_rows_transpose_supported(16384, 128, 64) == 0
    assert lib.pcl_group_linear_bwd_gather_supported(128) == 1 and lib.pcl_group_linear_bwd_gather_supported(96) == 0
    lib.pcl_set_scatter_form(0)
    assert lib.pcl_group_linear_bwd_gather_supported(128) == 0
    lib.pcl_set_scatter_form(1)
    assert lib.pcl_group_rows_transpose_i32(None, None, 1, 8, 2, 2, None, None, None) == -1
    assert lib.pcl_group_linear_bwd_gather_f32(p, p, p, p, p, p, p, p, p, 1, 8, 96, p, None, None, 0, None) == -1      # C1 = 96
    assert b"C1" in lib.pcl_last_error()
    assert lib.pcl_frag_linear_fwd_f32(p, 8, p, 8, None, None, None, 0.0, 4, 8, 8, p, 8, None, None, 16, None) == -1  # flush_k not 0 / 8 / 32
    assert lib.pcl_frag_linear_fwd_f32(p, 8, p, 8, None, None, None, 0.0, 4, 8, 8, p, 8, p, None, 0, None) == -1    # Y_lo without the fp64 sum
    assert b"Y_lo" in lib.pcl_last_error()


def test_stack_backward_refuses_a_gout_stride_it_cannot_honour():
    """pcl_mlp_stack_t.gout_ld (a pooled stack reads its slice of a concatenated gradient in place): a stride below the width, or any
    stride but the width on a stack without pooling, is an argument error raised on the host before anything is launched."""
    import ctypes
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc.mlp_hip import _CStack
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def desc(pool, gout_ld):
        d = _CStack()
        d.struct_bytes, d.n_layers, d.P, d.pool = ctypes.sizeof(_CStack), 2, 64, pool
        d.c[0], d.c[1], d.c[2] = 16, 64, 128
        d.slope, d.out_slope, d.eps, d.momentum = 0.0, 0.0, 1e-5, 0.1
        d.x = p
        for l in range(2):
            d.layer[l].W = d.layer[l].gamma = d.layer[l].beta = p
        d.out = d.save = d.tmp = d.gout = p
        d.gout_ld = gout_ld
        return d

    for pool, ld, word in ((32, 100, b"gout_ld"), (0, 320, b"gout_ld"), (32, -4, b"gout_ld")):
        d = desc(pool, ld)
        assert lib.pcl_mlp_stack_bwd_f32(ctypes.byref(d)) == -1, (pool, ld)
        assert word in lib.pcl_last_error(), lib.pcl_last_error()


def test_ball_query_multi_validates_on_the_host():
    """pcl_ball_query_multi_f32: the radius count, the per-radius sample counts and output pointers are checked before any launch."""
    import ctypes
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    r = (ctypes.c_float * 5)(0.1, 0.2, 0.3, 0.4, 0.5)
    s = (ctypes.c_int32 * 5)(4, 4, 0, 4, 4)
    out = (ctypes.c_void_p * 5)(*[p.value] * 5)
    assert lib.pcl_ball_query_multi_f32(p, p, 1, 1, 8, 5, r, s, out, None, None) == -1 and b"n_radii" in lib.pcl_last_error()
    assert lib.pcl_ball_query_multi_f32(p, p, 1, 1, 8, 3, r, s, out, None, None) == -1 and b"radius 2" in lib.pcl_last_error()
    assert lib.pcl_ball_query_multi_f32(p, p, 1, 1, 8, 2, r, s, None, None, None) == -1
    assert lib.pcl_ball_query_multi_f32(p, p, 0, 1, 8, 2, r, s, out, None, None) == 0            # empty batch: nothing launched
    assert lib.pcl_group_offsets_multi_i32(5, out, 8, out, None) == -1 and lib.pcl_group_offsets_multi_i32(2, None, 8, out, None) == -1
    bad = (ctypes.c_void_p * 2)(p.value, None)
    assert lib.pcl_group_offsets_multi_i32(2, bad, 8, out, None) == -1 and b"array 1" in lib.pcl_last_error()
