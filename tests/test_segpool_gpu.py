"""The segmented pooling kernels (csrc/segpool.hip) on the GPU, against the EXISTING kernels run cloud by cloud.

B = 5 clouds with 300, 1, 64, 65 and 257 packed rows (R = 687): a one-row cloud, counts on either side of a wave of rows, two clouds
beyond the 256-row threshold of the dense kernel; and B = 1 with 300 rows, where the mean cloud size crosses the threshold at which
the new launchers go from 4 to 16 waves per workgroup.  C = 64 takes the float4 path, 7 and 130 the one-float path (130: three
channel tiles, the last with two live lanes).  ``scale`` has negative entries and one exact zero; two ties are planted in cloud 0:
a constant column (the first row must win) and a column whose maximum sits in rows 3 and 200, which different slices own (row 3
must win).  Two sentinel rows lie behind every output buffer.

Forward and ``du`` must equal the dense kernels bit for bit: the same fmaf + lrelu expression, and a max / first-index fold is exact
in any order.  The BatchNorm-backward sums are fp64 sums of exactly representable terms (an fp32 value, or the exact fp64 product
of two) in some order: at most R - 1 additions, each rounding by at most 2^-53 of a partial sum that never exceeds sum|term|, so the
total lies within R * 2^-52 * sum|term| of the true sum with a factor two to spare for the fp64 reference's own rounding.  The
segment sum adds n_b fp32 values in fp64 and rounds once to fp32: within 2^-24 |s| + n_b 2^-52 sum|g| of the fp64 sum s."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(C, slope) for C in (64, 7, 130) for slope in (0.0, 0.2, 1.0)]
LAYOUTS = {"B5": [300, 1, 64, 65, 257], "B1": [300]}
SENT = -7.25


def _same(a, b):
    """Bit equality (NaN-safe, -0.0 != +0.0)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _p(t):
    return t.data_ptr()


def _layout(dev, lengths):
    from pointcloudlib_amd.misc import ops
    B, N = len(lengths), max(lengths)
    row_off, R = ops.row_offsets(lengths, B, N, dev)
    assert R == sum(lengths)
    rc = ops.row_cloud(row_off, B, R)
    want = torch.repeat_interleave(torch.arange(B), torch.tensor(lengths)).to(torch.int32)
    assert rc.dtype == torch.int32 and torch.equal(rc.cpu(), want), "row_cloud"
    return row_off, rc, R


def _inputs(dev, lengths, C, seed=0):
    g = torch.Generator().manual_seed(17 * C + len(lengths) + seed)
    R = sum(lengths)
    Y = torch.randn(R, C, generator=g)
    scale = torch.randn(C, generator=g)
    scale[0] = 0.0                                # an exact zero: every row ties, the first wins
    scale[2] = 1.5
    scale[3] = -abs(scale[3]) - 0.1               # a negative one for sure
    shift = 0.3 * torch.randn(C, generator=g)
    Y[:lengths[0], 1] = 0.75                      # a constant column in cloud 0
    Y[3, 2] = Y[200, 2] = 100.0                   # the maximum twice, in rows of different slices
    return Y.to(dev), scale.to(dev), shift.to(dev)


def _forward(dev, Y, row_off, scale, shift, slope, B, C, n_rows):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc import ops
    out = torch.full((B + 2, C), SENT, device=dev)
    arg = torch.full((B + 2, C), -77, dtype=torch.int32, device=dev)
    _lib.call("pcl_bn_act_seg_max_f32", _p(Y), _p(row_off), _p(scale), _p(shift), slope, B, C, n_rows, _p(out), _p(arg), ops._stream())
    assert bool((out[B:] == SENT).all()) and bool((arg[B:] == -77).all()), "forward wrote behind its outputs"
    return out[:B], arg[:B]


def _dense_forward(dev, Y, off, scale, shift, slope, C):
    """pcl_bn_act_max_mean_f32 on every cloud alone (G = 1, ns = n_b): the truth."""
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc import ops
    B = len(off) - 1
    out = torch.empty((B, C), device=dev)
    mean = torch.empty((B, C), device=dev)
    arg = torch.empty((B, C), dtype=torch.int32, device=dev)
    for b in range(B):
        n = off[b + 1] - off[b]
        _lib.call("pcl_bn_act_max_mean_f32", _p(Y[off[b]:]), _p(scale), _p(shift), slope, 1, n, C, C, _p(out[b]), _p(mean[b]), _p(arg[b]),
                  ops._stream())
    return out, arg


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("C,slope", CASES)
def test_segment_max_forward_equals_the_dense_kernels_per_cloud(dev, layout, C, slope):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc import ops
    lengths = LAYOUTS[layout]
    B = len(lengths)
    row_off, rc, R = _layout(dev, lengths)
    off = row_off.tolist()
    Y, scale, shift = _inputs(dev, lengths, C)
    out, arg = _forward(dev, Y, row_off, scale, shift, slope, B, C, R)
    want, want_arg = _dense_forward(dev, Y, off, scale, shift, slope, C)
    assert _same(out, want), "out differs from pcl_bn_act_max_mean_f32 per cloud"
    assert _same(arg, want_arg), "arg differs from pcl_bn_act_max_mean_f32 per cloud"
    assert arg[0, 0].item() == 0 and arg[0, 1].item() == 0 and arg[0, 2].item() == 3, "planted ties: the first row wins"
    # the other segmented max of the library: one lane per (group, channel piece)
    o2 = torch.empty((B, C), device=dev)
    a2 = torch.empty((B, C), dtype=torch.int32, device=dev)
    y2 = torch.empty((B, C), device=dev)
    _lib.call("pcl_bn_act_max_rows_f32", _p(Y), _p(row_off), _p(scale), _p(shift), slope, B, C, _p(o2), _p(a2), _p(y2), ops._stream())
    assert _same(out, o2) and _same(arg, a2), "differs from pcl_bn_act_max_rows_f32 with group_off = row_off"
    # a short n_rows: the last cloud loses its last 10 rows and nothing else changes
    if lengths[-1] > 10:
        out_s, arg_s = _forward(dev, Y, row_off, scale, shift, slope, B, C, R - 10)
        off_s = off[:-1] + [R - 10]
        want_s, want_arg_s = _dense_forward(dev, Y, off_s, scale, shift, slope, C)
        assert _same(out_s, want_s) and _same(arg_s, want_arg_s), "n_rows = R - 10"
    # the public operator without constants is a plain segmented max
    plain = ops.segment_max(Y, row_off, rc, B)
    want_plain = torch.stack([Y[off[b]:off[b + 1]].max(0)[0] for b in range(B)])
    assert _same(plain, want_plain), "ops.segment_max (unit constants) is not the plain max"


def test_segment_max_of_a_cut_off_cloud_is_minus_infinity(dev):
    """An empty segment arises only from an n_rows below the cloud's first row: out = -inf, arg = 0 (documented in the header)."""
    lengths = LAYOUTS["B5"]
    row_off, _, R = _layout(dev, lengths)
    Y, scale, shift = _inputs(dev, lengths, 7)
    out, arg = _forward(dev, Y, row_off, scale, shift, 0.2, 5, 7, 430)          # cloud 4 starts at row 430
    assert bool((out[4] == float("-inf")).all()) and bool((arg[4] == 0).all())
    assert bool(torch.isfinite(out[:4]).all())


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("C,slope", CASES)
def test_segment_max_backward_equals_the_dense_kernel_per_cloud(dev, layout, C, slope):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc import ops
    lengths = LAYOUTS[layout]
    B = len(lengths)
    row_off, rc, R = _layout(dev, lengths)
    off = row_off.tolist()
    Y, scale, shift = _inputs(dev, lengths, C)
    _, arg = _forward(dev, Y, row_off, scale, shift, slope, B, C, R)
    arg = arg.contiguous()
    ldg = C + 5                                                                # gmax: a column slice of a wider gradient
    wide = torch.randn(B, ldg, generator=torch.Generator().manual_seed(C)).to(dev)
    gmax = wide[:, 3:]
    assert gmax.data_ptr() == wide.data_ptr() + 12

    def run(n_rows):
        du = torch.full((R + 2, C), SENT, device=dev)
        stats = torch.full((1024 + 2, 2, C), SENT, dtype=torch.float64, device=dev)
        rows = ctypes.c_int(0)
        _lib.call("pcl_bn_act_seg_max_bwd_f32", _p(gmax), ldg, _p(arg), _p(Y), _p(scale), _p(shift), slope, _p(row_off), _p(rc), B, C, n_rows,
                  _p(du), _p(stats), ctypes.byref(rows), ops._stream())
        assert 1 <= rows.value <= 1024, f"stat_rows_out = {rows.value}"
        assert bool((stats[rows.value:] == SENT).all()), "stats rows behind stat_rows_out were written"
        return du, stats[:rows.value]

    du, stats = run(R)
    assert bool((du[R:] == SENT).all()), "du: a row >= n_rows was written"
    # the truth: pcl_bn_act_max_mean_bwd_f32 per cloud with a zero mean gradient
    want = torch.empty((R, C), device=dev)
    zeros = torch.zeros(ldg, device=dev)
    ws = torch.empty((1024, 2, C), dtype=torch.float64, device=dev)
    rows = ctypes.c_int(0)
    for b in range(B):
        n = off[b + 1] - off[b]
        _lib.call("pcl_bn_act_max_mean_bwd_f32", _p(gmax[b]), _p(zeros), ldg, _p(arg[b]), _p(Y[off[b]:]), _p(scale), _p(shift), slope, 1, n, C,
                  _p(want[off[b]:]), _p(ws), ctypes.byref(rows), ops._stream())
    assert _same(du[:R], want), "du differs from pcl_bn_act_max_mean_bwd_f32 per cloud"
    assert int((du[:R] != 0).any(1).sum()) >= 1
    # the BatchNorm-backward sums against fp64, bound derived in the module docstring
    d64, y64 = du[:R].double().cpu(), Y.double().cpu()
    got = stats.cpu().sum(0)
    for k, term in enumerate((d64, d64 * y64)):
        err = (got[k] - term.sum(0)).abs()
        bound = R * 2.0 ** -52 * term.abs().sum(0)
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{layout} C={C} slope={slope}: stats[{k}] worst err / bound = {worst:.3g}")
        assert bool((err <= bound).all()), f"stats[{k}]: worst err / bound = {worst:.3g}"
    # a short n_rows: rows >= n_rows keep their sentinel, the others are unchanged
    du_s, _ = run(R - 10)
    assert _same(du_s[:R - 10], want[:R - 10]) and bool((du_s[R - 10:] == SENT).all()), "n_rows = R - 10"


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("C", [64, 7, 130])
def test_broadcast_rows_and_its_segment_sum(dev, layout, C):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc import ops
    lengths = LAYOUTS[layout]
    B = len(lengths)
    row_off, rc, R = _layout(dev, lengths)
    off = row_off.tolist()
    g = torch.Generator().manual_seed(C + B)
    src = torch.randn(B, C, generator=g).to(dev)
    for n_rows in (R, R - 10):
        dst = torch.full((R + 2, C), SENT, device=dev)
        _lib.call("pcl_seg_broadcast_rows_f32", _p(src), _p(rc), B, C, n_rows, _p(dst), ops._stream())
        assert _same(dst[:n_rows], src[rc.long()[:n_rows]]), "broadcast differs from src[row_cloud]"
        assert bool((dst[n_rows:] == SENT).all()), "broadcast: a row >= n_rows was written"
    grad = torch.randn(R, C, generator=g).to(dev)
    runs = []
    for _ in range(2):
        gsrc = torch.full((B + 2, C), SENT, device=dev)
        _lib.call("pcl_seg_sum_rows_f32", _p(grad), _p(row_off), B, C, R, _p(gsrc), ops._stream())
        assert bool((gsrc[B:] == SENT).all()), "segment sum wrote behind its output"
        runs.append(gsrc[:B].clone())
    assert _same(runs[0], runs[1]), "segment sum is not run-to-run identical"
    g64 = grad.double().cpu()
    for b in range(B):
        seg = g64[off[b]:off[b + 1]]
        s = seg.sum(0)
        bound = 2.0 ** -24 * s.abs() + lengths[b] * 2.0 ** -52 * seg.abs().sum(0)
        err = (runs[0][b].double().cpu() - s).abs()
        assert bool((err <= bound).all()), f"cloud {b}: worst err / bound = {(err / bound).max().item():.3g}"
    # the operators: forward the broadcast, backward the sum
    v = src.clone().requires_grad_(True)
    out = ops.broadcast_rows(v, row_off, rc, R)
    assert _same(out.detach(), src[rc.long()])
    out.backward(grad)
    assert _same(v.grad, runs[0])
