"""The step's short reduction kernels keep several rows' loads in flight (csrc/common.h: rows_in_flight): which thread owns which
element, the order of a thread's compares and additions, the lane / LDS folds and the partial-row layouts are what they were, so
every output is the same bits as before.  The yardstick here is NOT a second run of the library but a NumPy restatement of each
kernel's documented order -- sequential per thread, then the documented fold -- compared bit for bit.

  pcl_bn_act_max_f32 / pcl_bn_act_max_mean_f32   slice sl of SL (4, or 16 from ns = 256) scans the rows sl, sl + SL, .. with a strict >
                                                 (the first row wins), fp64 sum in that order; slices merge 1 .. SL-1 in order with
                                                 z > best || (z == best && s < bi); the mean is (float)(sum / ns)
  pcl_maxgrad_prep_f32                           CW = min(256, 2^ceil(log2 C)) lanes over channels, RS = 256 / CW row lanes, rows =
                                                 min(ceil(G / RS), 512) partial rows; row lane (y, rsub) adds g = y RS + rsub, + rows RS, ..
                                                 in fp64, then row lane 0 adds the lanes 1 .. RS-1 in order
  the dW0 sums                                   lane l of a wave adds the partial rows l, l + 64, .. from 0.f, then the xor tree 32 .. 1
  pcl_group_offsets_i32                          goff = exclusive cumsum of max(cnt, 1), goff[G] the total (integers: any order)

fmaf(scale, y, shift) is restated exactly (product exact in fp64, the sum rounded to odd before the one rounding to fp32)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64, I32 = np.float32, np.float64, np.int32


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])


def _same(got, want):
    """bit for bit (tells -0.0 from 0.0, which == does not)"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _fmaf(a, y, b):
    """fp32 fma(a, y, b) of fp32 arrays with its single rounding."""
    a, y, b = (np.asarray(v, F64) for v in (a, y, b))
    p = a * y                                   # exact: 24 x 24 significant bits
    s = p + b
    t = s - p
    e = (p - (s - t)) + (b - t)                 # p + b = s + e exactly
    fix = (e != 0) & ((_bits(s) & 1) == 0)      # round to odd: the fp64 sum may not sit on an fp32 tie it did not earn
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _lrelu(x, slope):
    return np.where(x > 0, x, x * F32(slope)).astype(F32)


def _pool_restated(Y, scale, shift, slope, SL):
    """Y [G, ns, C] -> (max, arg, y at arg, mean) in the kernels' order; SL = 1 is the one-thread-per-(g, c) kernel."""
    G, ns, C = Y.shape
    z = _lrelu(_fmaf(scale[None, None], Y, shift[None, None]), slope)
    best = np.full((SL, G, C), -np.inf, F32)
    bi, by, sm = np.zeros((SL, G, C), I32), np.zeros((SL, G, C), F32), np.zeros((SL, G, C), F64)
    for sl in range(SL):
        for s in range(sl, ns, SL):
            up = z[:, s] > best[sl]
            best[sl] = np.where(up, z[:, s], best[sl])
            bi[sl] = np.where(up, s, bi[sl])
            by[sl] = np.where(up, Y[:, s], by[sl])
            sm[sl] = sm[sl] + z[:, s].astype(F64)
    B, I, Yb, S = best[0].copy(), bi[0].copy(), by[0].copy(), sm[0].copy()
    for j in range(1, SL):
        up = (best[j] > B) | ((best[j] == B) & (bi[j] < I))
        B, I, Yb = np.where(up, best[j], B), np.where(up, bi[j], I), np.where(up, by[j], Yb)
        S = S + sm[j]
    return B.astype(F32), I.astype(I32), Yb.astype(F32), (S / ns).astype(F32)


POOL_SHAPES = [(2, 64, 64), (3, 67, 70), (2, 256, 64), (1, 259, 33), (1, 64, 1)]


def _pool_case(G, ns, C, variant, SL):
    """A third of the gammas negative.  "neg": slope 0 and every activation of group 0 <= 0 (row 0 must be named).  "dup": the maximum
    of the last group appears twice, in rows of different slices and of different batches of 8 trips (trips 1 and 11 of their
    slices); in the odd channels the lower row lies in the higher slice."""
    rng = np.random.default_rng(1000 * G + 10 * ns + C + (variant == "dup"))
    scale = rng.uniform(0.5, 1.5, C).astype(F32)
    scale[rng.permutation(C)[: (C + 2) // 3]] *= -1
    shift = rng.standard_normal(C).astype(F32)
    Y = rng.standard_normal((G, ns, C)).astype(F32)
    slope = 0.0 if variant == "neg" else 0.2
    if variant == "neg":
        Y[0] = (-np.sign(scale) * (np.abs(shift / scale) + np.abs(Y[0]) + 0.01)).astype(F32)
    else:
        for par, (lo, hi) in enumerate(((SL + 1, 11 * SL + 2), (SL + 2, 11 * SL + 1))):
            assert lo < hi < ns and lo % SL != hi % SL and (lo // SL) // 8 != (hi // SL) // 8
            Y[-1, lo, par::2] = Y[-1, hi, par::2] = (50 * np.sign(scale))[par::2]
    return Y, scale, shift, slope


@pytest.fixture(scope="module")
def pool_truth():
    memo = {}

    def get(G, ns, C, variant, SL):
        key = (G, ns, C, variant, SL)
        if key not in memo:
            Y, scale, shift, slope = _pool_case(G, ns, C, variant, SL)
            want = _pool_restated(Y, scale, shift, slope, SL)
            if variant == "neg":
                assert (want[1][0] == 0).all() and (want[0][0] <= 0).all()
            elif SL > 1:
                assert (want[1][-1, 0::2] == SL + 1).all() and (want[1][-1, 1::2] == SL + 2).all()
            memo[key] = (Y, scale, shift, slope, want)
        return memo[key]
    return get


@pytest.mark.parametrize("variant", ["neg", "dup"])
@pytest.mark.parametrize("G,ns,C", POOL_SHAPES)
def test_sliced_max_names_what_the_sequential_scan_names(dev, pool_truth, G, ns, C, variant):
    from pointcloudlib_amd import _lib
    Y, scale, shift, slope, want = pool_truth(G, ns, C, variant, 16 if ns >= 256 else 4)
    out = torch.full((G, C), float("nan"), device=dev)
    ymax = torch.full((G, C), float("nan"), device=dev)
    arg = torch.full((G, C), -1, dtype=torch.int32, device=dev)
    dY, dsc, dsh = (torch.from_numpy(v).to(dev) for v in (Y, scale, shift))
    _lib.call("pcl_bn_act_max_f32", _p(dY), _p(dsc), _p(dsh), slope, G, ns, C, _p(out), _p(arg), _p(ymax), _st())
    assert _same(arg, want[1]), "arg"
    assert _same(out, want[0]), "out"
    assert _same(ymax, want[2]), "ymax"


@pytest.mark.parametrize("variant", ["neg", "dup"])
@pytest.mark.parametrize("G,ns,C", POOL_SHAPES)
def test_max_mean_pool_in_the_documented_order(dev, pool_truth, G, ns, C, variant):
    from pointcloudlib_amd import _lib
    Y, scale, shift, slope, want = pool_truth(G, ns, C, variant, 16 if ns >= 256 else 4)
    both = torch.full((G, 2 * C), float("nan"), device=dev)          # [max | mean], as DGCNN concatenates them
    arg = torch.full((G, C), -1, dtype=torch.int32, device=dev)
    dY, dsc, dsh = (torch.from_numpy(v).to(dev) for v in (Y, scale, shift))
    _lib.call("pcl_bn_act_max_mean_f32", _p(dY), _p(dsc), _p(dsh), slope, G, ns, C, 2 * C, _p(both), _p(both[:, C:]), _p(arg), _st())
    assert _same(arg, want[1]), "arg"
    assert _same(both[:, :C].contiguous(), want[0]), "max"
    assert _same(both[:, C:].contiguous(), want[3]), "mean"


# the one-thread-per-(g, c) kernel (ns < 64): 13 rows = batches of 8, 4 and 1; one row; 40 rows = five batches of 8
@pytest.mark.parametrize("G,ns,C", [(5, 13, 70), (3, 1, 5), (2, 40, 33)])
def test_plain_max_names_what_the_sequential_scan_names(dev, G, ns, C):
    from pointcloudlib_amd import _lib
    Y, scale, shift, slope = _pool_case(G, ns, C, "neg", 1)
    want = _pool_restated(Y, scale, shift, slope, 1)
    assert (want[1][0] == 0).all()
    out, ymax = torch.full((G, C), float("nan"), device=dev), torch.full((G, C), float("nan"), device=dev)
    arg = torch.full((G, C), -1, dtype=torch.int32, device=dev)
    dY, dsc, dsh = (torch.from_numpy(v).to(dev) for v in (Y, scale, shift))
    _lib.call("pcl_bn_act_max_f32", _p(dY), _p(dsc), _p(dsh), slope, G, ns, C, _p(out), _p(arg), _p(ymax), _st())
    assert _same(arg, want[1]) and _same(out, want[0]) and _same(ymax, want[2])


# ---------------------------------------------------------------------------------------------------------------- pcl_maxgrad_prep_f32
def _maxgrad_restated(gout, out, ymax, slope, G, C):
    CW = 256
    while CW // 2 >= C and CW > 1:
        CW >>= 1
    RS = 256 // CW
    rows = min((G + RS - 1) // RS, 512)
    gz = (gout[:, :C] * np.where(out > 0, F32(1), F32(slope))).astype(F32)
    s1, s2 = np.zeros((rows, RS, C), F64), np.zeros((rows, RS, C), F64)
    first = (np.arange(rows)[:, None] * RS + np.arange(RS)[None, :])              # [rows, RS]: a row lane's first g
    for t in range((G + rows * RS - 1) // (rows * RS)):
        g = first + t * rows * RS
        live = (g < G)[:, :, None]
        v = gz[np.minimum(g, G - 1)]
        y = ymax[np.minimum(g, G - 1)]
        s1 = np.where(live, s1 + v.astype(F64), s1)
        s2 = np.where(live, s2 + v.astype(F64) * y.astype(F64), s2)
    S1, S2 = s1[:, 0].copy(), s2[:, 0].copy()
    for j in range(1, RS):
        S1, S2 = S1 + s1[:, j], S2 + s2[:, j]
    return gz, rows, np.stack([S1, S2], axis=1)                                   # [rows][2][C]


# the last shape is this file's own: 20 trips per row lane (batches of 8, 8 and 4; the lanes past G: 8, 8, 2 and 1)
@pytest.mark.parametrize("G,C,ldg", [(1, 64, 64), (5, 128, 128), (37, 256, 300), (1030, 128, 128), (9000, 96, 96), (33, 1024, 1024),
                                     (20000, 128, 128)])
def test_maxgrad_prep_sums_in_the_documented_order(dev, G, C, ldg):
    from pointcloudlib_amd import _lib
    rng = np.random.default_rng(G + C)
    gout = rng.standard_normal((G, ldg)).astype(F32)
    out = rng.standard_normal((G, C)).astype(F32)
    out[rng.random((G, C)) < 0.1] = 0.0                                           # act'(0) is the slope
    ymax = rng.standard_normal((G, C)).astype(F32)
    slope = 0.2
    want_gz, want_rows, want_stats = _maxgrad_restated(gout, out, ymax, slope, G, C)
    gz = torch.full((G, C), float("nan"), device=dev)
    stats = torch.full((512, 2, C), float("nan"), dtype=torch.float64, device=dev)
    rows = ctypes.c_int(-1)
    dg, do, dy = (torch.from_numpy(v).to(dev) for v in (gout, out, ymax))
    if ldg == C:
        _lib.call("pcl_maxgrad_prep_f32", _p(dg), _p(do), _p(dy), slope, G, C, _p(gz), _p(stats), ctypes.byref(rows), _st())
    else:       # a column slice of a wider gradient, as a stack whose output was concatenated with others' receives it
        _lib.call("pcl_maxgrad_prep_ld_f32", _p(dg), ldg, _p(do), _p(dy), slope, G, C, _p(gz), _p(stats), ctypes.byref(rows), _st())
    assert rows.value == want_rows
    assert _same(gz, want_gz), "gz"
    assert _same(stats[:want_rows], want_stats), "fp64 partial rows"


# ---------------------------------------------------------------------------------------------------------------- the dW0 sums
def _wave_sum_restated(part):
    """part [rows, n] fp32 -> [n]: lane l adds rows l, l + 64, .. from 0.f; lanes fold by xor 32, 16, .. 1; lane 0's value"""
    rows, n = part.shape
    s = np.zeros((64, n), F32)
    for r0 in range(0, rows, 64):
        k = min(64, rows - r0)
        s[:k] = s[:k] + part[r0:r0 + k]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[lanes ^ o]).astype(F32)
    return s[0]


@pytest.mark.parametrize("CF", [0, 3])
@pytest.mark.parametrize("C1", [64, 128])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 200, 1024])
def test_dw0_sums_agree_with_each_other_and_the_documented_order(dev, rows, C1, CF):
    from pointcloudlib_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(rows * 1000 + C1 + CF)
    px = rng.standard_normal((rows, C1, 3)).astype(F32)
    pf = rng.standard_normal((rows, C1, CF)).astype(F32) if CF else None
    ld = 3 + CF + 2                                                                # two columns nobody owns: they keep their 7s
    want = np.full((C1, ld), 7, F32)
    want[:, :3] = _wave_sum_restated(px.reshape(rows, -1)).reshape(C1, 3)
    if CF:
        want[:, 3:3 + CF] = _wave_sum_restated(pf.reshape(rows, -1)).reshape(C1, CF)
    dpx = torch.from_numpy(px).to(dev)
    dpf = torch.from_numpy(pf).to(dev) if CF else None
    own = torch.full((C1, ld), 7.0, device=dev)
    _lib.call("pcl_group_linear_dw_sum_f32", _p(dpx), _p(dpf), rows, C1, CF, 3, ld, _p(own), _st())
    assert _same(own, want), "group_linear_dw_kernel"
    # the same sum riding in the finish launch of the point GEMMs' pair (coordinate columns only), beside the tile sum it is there for
    P, Cout, Cin = 64, C1, 128
    ws_bytes = L.pcl_linear_bwd_dw_workspace_bytes(P, Cout, Cin)
    ws = torch.randn(ws_bytes // 4, device=dev)
    dW, dW_plain = torch.full((Cout, Cin), 7.0, device=dev), torch.full((Cout, Cin), 7.0, device=dev)
    rode = torch.full((C1, ld), 7.0, device=dev)
    none = [None] * 4
    _lib.call("pcl_linear_bwd_pair_finish_xyz_f32", _p(ws), ws_bytes, P, Cout, Cin, _p(dW), 0, None, 0, None, None, None, 0, *none, None, None,
              _p(dpx), rows, C1, ld, _p(rode), _st())
    _lib.call("pcl_linear_bwd_pair_finish_f32", _p(ws), ws_bytes, P, Cout, Cin, _p(dW_plain), 0, None, 0, None, None, None, 0, *none, None, None, _st())
    want_x = np.full((C1, ld), 7, F32)
    want_x[:, :3] = want[:, :3]
    assert _same(rode, want_x), "FinishXJob blocks"
    assert _same(rode[:, :3].contiguous(), own[:, :3].contiguous().cpu().numpy()), "the two launches disagree"
    assert torch.equal(dW, dW_plain) and torch.isfinite(dW).all(), "the tile sum beside it"


# ---------------------------------------------------------------------------------------------------------------- pcl_group_offsets_i32
@pytest.mark.parametrize("G", [1, 1023, 1024, 1025, 16384])
def test_group_offsets_is_the_cumsum(dev, G):
    from pointcloudlib_amd import _lib
    rng = np.random.default_rng(G)
    cnts = [rng.integers(0, 65, G).astype(I32) for _ in range(3)]
    cnts[0][rng.random(G) < 0.2] = 0
    cnts[1][:] = 0                                                                  # every group empty: one row each
    want = [np.concatenate([[0], np.cumsum(np.maximum(c, 1))]).astype(I32) for c in cnts]
    dc = [torch.from_numpy(c).to(dev) for c in cnts]
    got = torch.full((G + 1,), -1, dtype=torch.int32, device=dev)
    _lib.call("pcl_group_offsets_i32", _p(dc[0]), G, _p(got), _st())
    assert _same(got, want[0])
    # the same body, one workgroup per array
    outs = [torch.full((G + 1,), -1, dtype=torch.int32, device=dev) for _ in cnts]
    arr = ctypes.c_void_p * 3
    _lib.call("pcl_group_offsets_multi_i32", 3, arr(*(c.data_ptr() for c in dc)), G, arr(*(o.data_ptr() for o in outs)), _st())
    for o, w in zip(outs, want):
        assert _same(o, w)
