"""The folded first layer's backward without the Y read (csrc/compact.hip: group_linear_bwd_regen_kernel,
group_linear_bwd_gather_regen_kernel): y is formed again from the row records (and Uf) by the device function the forward forms it
with, so every output must be BIT-identical to the entry points that read the Y the forward stored.  The witnesses are those older
entry points, fed the forward entry point's own Y.

Geometry (built by hand, the smallest that reaches every branch): B = 2 clouds of N = 40 points, m = 24 groups of up to ns = 16 rows.
Point 0 of each cloud is in all 24 groups (more than PPW * U = 16 rows: the gather's chunk loop runs twice at C1 = 64), points 36..39
are in no group (o0 == o1, among them the last point of the last cloud), several groups have one row, the row count is no multiple of
16, and the second cloud makes the point base non-zero."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, M, NS = 2, 40, 24, 16
CNT = [1, 16, 5, 1, 9, 2, 13, 1, 7, 16, 3, 11, 1, 6, 15, 4, 1, 10, 8, 2, 12, 1, 14, 5]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def geo(dev):
    from pointcloudlib_amd import _lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(11)
    cnt = torch.tensor(CNT * B, dtype=torch.int32)
    idx = torch.zeros(B, M, NS, dtype=torch.int32)               # slot 0 and the padding: point 0, as ball query pads with the first hit
    for b in range(B):
        for gi in range(M):
            for s in range(1, CNT[gi]):
                idx[b, gi, s] = 1 + (gi * 7 + b * 3 + s) % 35   # distinct within a group (s < 35), never 36..39
    R = int(cnt.sum())
    assert R % 16 != 0 and CNT.count(1) >= 3
    xyz, new_xyz = torch.randn(B * N, 3, generator=g), torch.randn(B * M, 3, generator=g)
    d = dict(cnt=cnt.to(dev), idx=idx.to(dev), xyz=xyz.to(dev), new_xyz=new_xyz.to(dev), R=R, st=st)
    d["goff"] = torch.empty(B * M + 1, dtype=torch.int32, device=dev)
    _lib.call("pcl_group_offsets_i32", _p(d["cnt"]), B * M, _p(d["goff"]), st)
    assert int(d["goff"][-1].item()) == R
    return d


def _forward(dev, geo, C1, CF, use_xyz, pad, wide):
    """pcl_group_linear_f32 on the hand-built groups: Y as the forward stores it, the row records, the weights it read."""
    from pointcloudlib_amd import _lib
    L = _lib.lib()
    st = geo["st"]
    torch.manual_seed(1000 * C1 + 10 * CF + use_xyz + 2 * pad)
    off = 3 if use_xyz else 0
    ldw = off + CF + pad                                         # row stride of the stored weight: wider than the columns used when pad > 0
    W0 = torch.randn(C1, max(ldw, 1), device=dev)
    feat = torch.randn(B * N, CF, device=dev) if CF else None
    # the per-point product with a conv bias folded in: arbitrary values as far as these kernels are concerned
    Uf = (torch.randn(B * N, C1, device=dev) + torch.randn(C1, device=dev)) if wide else None
    cap = B * M * NS
    Y = torch.full((cap, C1), float("nan"), device=dev)
    meta = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    src = torch.empty(cap, dtype=torch.int32, device=dev)
    loc = torch.empty(cap, 4, device=dev)
    rfeat = torch.empty(cap, 4, device=dev) if CF else None
    stats = torch.empty(L.pcl_group_linear_stat_rows(B, M), 2, C1, dtype=torch.float64, device=dev)
    Wx = W0 if use_xyz else None
    Wf = W0[:, off:] if CF else None
    _lib.call("pcl_group_linear_f32", _p(geo["xyz"]), _p(geo["new_xyz"]), _p(Uf), _p(Wx), _p(feat), _p(Wf), CF, ldw, _p(geo["idx"]), _p(geo["cnt"]),
              _p(geo["goff"]), B, N, M, NS, C1, _p(Y), _p(meta), _p(src), _p(loc), _p(rfeat), _p(stats), st)
    R = geo["R"]
    assert torch.isfinite(Y[:R]).all()
    dU = torch.randn(cap, C1, device=dev)
    a, k1, k2, mu = (torch.randn(C1, device=dev) for _ in range(4))
    return dict(W0=W0, Wx=Wx, Wf=Wf, ldw=ldw, off=off, Uf=Uf, Y=Y, src=src, loc=loc, rfeat=rfeat, dU=dU, a=a, k1=k1, k2=k2, mu=mu)


V4_CASES = [(C1, CF, xyz, 0) for C1 in (64, 128, 256) for CF in (0, 3, 4) for xyz in (True, False) if (CF or xyz)]
V4_CASES += [(64, 3, True, 5), (128, 4, False, 5), (256, 0, True, 5)]


@pytest.mark.parametrize("C1,CF,use_xyz,pad", V4_CASES)
def test_regen_form_equals_the_form_that_reads_y(dev, geo, C1, CF, use_xyz, pad):
    from pointcloudlib_amd import _lib
    L = _lib.lib()
    assert L.pcl_group_linear_bwd_regen_supported(C1, CF) == 1
    f = _forward(dev, geo, C1, CF, use_xyz, pad, wide=False)
    st, rows_blk = geo["st"], L.pcl_group_linear_stat_rows(B, M)
    ld0 = f["off"] + CF + pad
    nrows = geo["goff"][B * M:]

    def run(which):
        dWx = torch.full((rows_blk, C1, 3), 3.0, device=dev) if use_xyz else None
        dWf = torch.full((rows_blk, C1, CF), 3.0, device=dev) if CF else None
        dW0 = torch.full((C1, ld0), 3.0, device=dev)
        if which == "y":
            _lib.call("pcl_group_linear_bwd_f32", _p(f["loc"]), _p(f["rfeat"]), CF, _p(f["dU"]), _p(f["Y"]), _p(f["a"]), _p(f["k1"]), _p(f["k2"]),
                      _p(f["mu"]), _p(f["src"]), _p(nrows), B, N, C1, None, _p(dWx), _p(dWf), _p(dW0), ld0, f["off"], st)
        else:
            _lib.call("pcl_group_linear_bwd_regen_f32", _p(f["loc"]), _p(f["rfeat"]), _p(f["Wx"]), _p(f["Wf"]), CF, f["ldw"], _p(f["dU"]), _p(f["a"]),
                      _p(f["k1"]), _p(f["k2"]), _p(f["mu"]), _p(nrows), C1, _p(dWx), _p(dWf), _p(dW0), ld0, f["off"], st)
        return dWx, dWf, dW0

    want, got, again = run("y"), run("regen"), run("regen")
    for name, w, g, g2 in zip(("dWx_part", "dWf_part", "dW0"), want, got, again):
        if w is None:
            continue
        assert torch.isfinite(w).all(), name
        assert torch.equal(w, g), (name, (w - g).abs().max().item())
        assert torch.equal(g, g2), name + " (second call)"


GATHER_CASES = [(C1, xyz, 0) for C1 in (64, 128, 256) for xyz in (True, False)] + [(128, True, 5)]


@pytest.mark.parametrize("C1,use_xyz,pad", GATHER_CASES)
def test_gather_regen_form_equals_the_form_that_reads_y(dev, geo, C1, use_xyz, pad):
    from pointcloudlib_amd import _lib
    L = _lib.lib()
    assert L.pcl_group_linear_bwd_gather_supported(C1) == 1 and L.pcl_group_rows_transpose_supported(N, M, NS) == 1
    f = _forward(dev, geo, C1, 0, use_xyz, pad, wide=True)
    st, rows_blk, R = geo["st"], L.pcl_group_linear_stat_rows(B, M), geo["R"]
    in_off = torch.empty(B * N + 1, dtype=torch.int32, device=dev)
    in_rows = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call("pcl_group_rows_transpose_i32", _p(f["src"]), _p(geo["goff"]), B, N, M, NS, _p(in_off), _p(in_rows), st)
    io = in_off.cpu()
    assert int(io[1] - io[0]) == M and int(io[N + 1] - io[N]) == M          # point 0 of each cloud: in every group
    assert int(io[B * N]) == R and int(io[B * N - 1]) == R                  # the last point of the last cloud: in none
    ld0 = 3 + pad

    def run(which):
        dUf = torch.full((B * N, C1), float("nan"), device=dev)
        dWx = torch.full((rows_blk, C1, 3), 3.0, device=dev) if use_xyz else None
        dW0 = torch.full((C1, ld0), 3.0, device=dev) if use_xyz else None
        if which == "y":
            _lib.call("pcl_group_linear_bwd_gather_f32", _p(f["loc"]), _p(f["dU"]), _p(f["Y"]), _p(f["a"]), _p(f["k1"]), _p(f["k2"]), _p(f["mu"]),
                      _p(in_off), _p(in_rows), B, N, C1, _p(dUf), _p(dWx), _p(dW0), ld0, st)
        else:
            _lib.call("pcl_group_linear_bwd_gather_regen_f32", _p(f["loc"]), _p(f["dU"]), _p(f["Uf"]), _p(f["Wx"]), f["ldw"], _p(f["a"]), _p(f["k1"]),
                      _p(f["k2"]), _p(f["mu"]), _p(in_off), _p(in_rows), B, N, C1, _p(dUf), _p(dWx), _p(dW0), ld0, st)
        return dUf, dWx, dW0

    want, got, again = run("y"), run("regen"), run("regen")
    assert (want[0][36:40] == 0).all() and (want[0][N + 36:] == 0).all()
    for name, w, g, g2 in zip(("dUf", "dWx_part", "dW0"), want, got, again):
        if w is None:
            continue
        assert torch.isfinite(w).all(), name
        assert torch.equal(w, g), (name, (w - g).abs().max().item())
        assert torch.equal(g, g2), name + " (second call)"


@pytest.mark.parametrize("C,feat_grad,spec_tail", [(3, False, [64, 64, 128]), (64, True, [128, 128])])
def test_stack_path_equals_per_kernel_path(dev, C, feat_grad, spec_tail):
    """Grouped-inline (Cf = 3, 64-64-128) and grouped-wide (Cf = 64, C1 = 128): the per-stack entry points and the per-kernel path run
    the same regenerating kernels on the same operands: parameter and input gradients bit-identical."""
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.misc import mlp_hip, ops
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    torch.manual_seed(5)
    b, n, m, ns = 4, 512, 96, 32
    x = torch.from_numpy(synth.gauss_ball(b, n, 31)).to(dev)
    feat0 = torch.randn(b, n, C, device=dev)
    _, new_xyz = ops.furthest_point_sample(x, m)
    idx, cnt = ops.ball_query(new_xyz, x, 0.25, ns, return_cnt=True)
    goff = ops.group_offsets(cnt)
    mlp = PointwiseMLP([3 + C] + spec_tail).to(dev).train()
    with torch.no_grad():
        for g in mlp.gammas:
            g.uniform_(0.5, 1.5); g[::4] *= -1.0
    gout = torch.randn(b, m, spec_tail[-1], device=dev)

    def go():
        mm = copy.deepcopy(mlp)
        f = feat0.clone().requires_grad_(feat_grad)
        out = mm.forward_grouped(x, new_xyz, f, idx, cnt, goff, True)
        out.backward(gout)
        return out.detach(), (f.grad.detach() if feat_grad else None), {k: p.grad.detach() for k, p in mm.named_parameters()}

    assert mlp_hip.USE_STACK
    a = go()
    with mlp_hip.per_kernel_path():
        k = go()
    assert torch.equal(a[0], k[0])
    for name in a[2]:
        assert torch.equal(a[2][name], k[2][name]), name
    if feat_grad:
        assert torch.equal(a[1], k[1])
