"""Frozen PointNet part segmentation on the GPU (pointcloudlib_amd/inference.py: FrozenPointNetPartseg,
csrc/infer_pointnet_seg.hip): every entry point through the C ABI on exactly representable data (bit for bit against fp64) over
its shapes, strides and ragged batches; a ragged batch against its clouds alone; whole networks on random data against an fp64
evaluation-mode restatement; the module plan; the memory a forward needs; the contract of ``FrozenPointNetPartseg``.

Yardstick (tests/test_inference_gpu.py): the frozen result may be no further from the fp64 restatement than ``net.eval()`` on the
same inputs, x 1.25, plus 1e-6."""
import copy
import ctypes
import functools

import pytest
import torch

from test_inference_gpu import _act, _consts64, _err, _perturb

pytestmark = pytest.mark.gpu

RAGGED = [200, 1, 64, 65, 129]
# (B, N, n_valid or None): dense N around the 64-row tile at B = 3, the ragged batch, one cloud of one tile
SHAPES = [(3, 1, None), (3, 63, None), (3, 64, None), (3, 65, None), (3, 129, None), (5, 200, RAGGED), (1, 64, None)]
SLOPES = [0.0, 0.5]
LDF = 840                                    # F's row stride in the kernel tests: 832 + 8 columns that must stay untouched
NAN = float("nan")


def _P(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _arr(tensors):
    return (ctypes.c_void_p * len(tensors))(*[_P(t) for t in tensors])


def _w(widths):
    return (ctypes.c_int32 * len(widths))(*widths)


def _lib():
    from pointcloudlib_amd import _lib
    return _lib


def _part_ws(B, N, C, dev):
    need = _lib().lib().pcl_pointnet_seg_part_workspace_bytes(B, N, C)
    return torch.full((need // 4,), NAN, device=dev), need          # never cleared, never read where it was not written


def _rows_bytes(B, N, ldf=LDF):
    return _lib().lib().pcl_pointnet_seg_rows_workspace_bytes(B, N, ldf)


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _call_stn(x, nv, P, slope, ldo=1024 + 8):
    """x [B,3,N] (a view of any strides) -> out [B, ldo], columns beyond 1024 filled with 7 before the call"""
    B, _, N = x.shape
    Ws, sc, sh = P
    ws, need = _part_ws(B, N, 1024, x.device)
    out = torch.full((B, ldo), 7.0, device=x.device)
    _lib().call("pcl_pointnet_seg_stn_infer_f32", _P(x), x.stride(0), x.stride(2), x.stride(1), _P(nv), B, N, 3, _w([w.shape[0] for w in Ws]),
                _P(Ws[0]), Ws[0].shape[1], _arr(Ws), _arr(sc), _arr(sh), float(slope), _P(ws), need, _P(out), ldo, _stream())
    return out


def _call_trunk(x, nv, T3, Pc, Ps, slope, ldo=1024 + 8):
    """-> (F [B*N, LDF] prefilled with NaN, out [B, ldo] prefilled with 7)"""
    B, _, N = x.shape
    (Wc, scc, shc), (Wsn, scs, shs) = Pc, Ps
    ws, need = _part_ws(B, N, 1024, x.device)
    F = torch.full((B * N, LDF), NAN, device=x.device)
    out = torch.full((B, ldo), 7.0, device=x.device)
    _lib().call("pcl_pointnet_seg_trunk_infer_f32", _P(x), x.stride(0), x.stride(2), x.stride(1), _P(nv), B, N, _P(T3), 3,
                _w([w.shape[0] for w in Wc]), _P(Wc[0]), Wc[0].shape[1], _arr(Wc), _arr(scc), _arr(shc), 3, _w([w.shape[0] for w in Wsn]),
                _arr(Wsn), _arr(scs), _arr(shs), float(slope), _P(F), LDF, _rows_bytes(B, N), _P(ws), need, _P(out), ldo, _stream())
    return F, out


def _call_global(F, nv, B, N, TT, P, slope, ldo=2048 + 8):
    """F [B*N, LDF] is updated in place (columns 320..831) -> out [B, ldo] prefilled with 7"""
    Ws, sc, sh = P
    ws, need = _part_ws(B, N, 2048, F.device)
    out = torch.full((B, ldo), 7.0, device=F.device)
    _lib().call("pcl_pointnet_seg_global_infer_f32", _P(F), LDF, _rows_bytes(B, N), _P(nv), B, N, _P(TT), 2, _w([w.shape[0] for w in Ws]),
                _arr(Ws), _arr(sc), _arr(sh), float(slope), _P(ws), need, _P(out), ldo, _stream())
    return out


def _call_head(F, nv, B, N, bias, P, Wout, bout, part_num, slope):
    """-> the whole output buffer [B, part_num + 1, N + 3] prefilled with 7; the logits are its [:, :part_num, :N]"""
    Ws, sc, sh = P
    buf = torch.full((B, part_num + 1, N + 3), 7.0, device=F.device)
    out = buf[:, :part_num, :N]
    _lib().call("pcl_pointnet_seg_head_infer_f32", _P(F), LDF, _rows_bytes(B, N), _P(nv), B, N, _P(bias), bias.stride(0), 4,
                _w([w.shape[0] for w in Ws] + [part_num]), _arr(list(Ws) + [Wout]), Wout.shape[0], _arr(sc), _arr(sh), _P(bout), float(slope),
                _P(out), out.stride(0), out.stride(1), out.stride(2), _stream())
    return buf


def _call_rows(x, W, scale, shift, slope):
    R, K = x.shape
    y = torch.full((R, W.shape[0] + 2), 7.0, device=x.device)
    _lib().call("pcl_pointnet_seg_rows_f32", _P(x), x.stride(0), R, K, _P(W), W.shape[0], _P(scale), _P(shift), float(slope), _P(y), y.stride(0),
                _stream())
    return y


# ----------------------------------------------------------------------------------------------------------- exact data
def _signed_rows(g, cout, cin, nz=4):
    """[cout, cin] with min(nz, cin) entries of +-1 per row"""
    W = torch.zeros(cout, cin)
    nz = min(nz, cin)
    for r in range(cout):
        cols = torch.randperm(cin, generator=g)[:nz]
        W[r, cols] = torch.randint(0, 2, (nz,), generator=g).float() * 2 - 1
    return W


@functools.lru_cache(maxsize=None)
def _exact_stack(spec, seed):
    """Made once, read only: as _exact_params of tests/test_inference_pointnet_gpu.py for any spec -- every weight row 4 entries
    of +-1 (3 when K = 3), scale +-1/2, shift an integer in [-2, 2]."""
    g = torch.Generator().manual_seed(seed)
    Ws, scales, shifts = [], [], []
    for cin, cout in zip(spec[:-1], spec[1:]):
        Ws.append(_signed_rows(g, cout, cin).cuda())
        scales.append(((torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1) / 2).cuda())
        shifts.append(torch.randint(-2, 3, (cout,), generator=g).float().cuda())
    return Ws, scales, shifts


class _Exact:
    """fp64 evaluation that asserts, as it goes, the precondition under which fp32 gives the same bits in any summation order
    (written like _assert_exact_precondition): with q the quantum of the current values, the sum of |products| of every layer and
    every value it produces stay below 2^24 q, and every value is a multiple of its q."""

    def __init__(self, q=1.0):
        self.q = q

    def _check(self, z):
        assert z.abs().max().item() / self.q < 2 ** 24
        assert bool((z / self.q == (z / self.q).round()).all())
        return z

    def linear(self, z, W, add=None):
        """z W^T (+ add): no change of quantum (the addend holds multiples of q)"""
        bound = z.abs() @ W.double().abs().t()
        y = z @ W.double().t()
        if add is not None:
            bound, y = bound + add.double().abs(), y + add.double()
        assert bound.max().item() / self.q < 2 ** 24
        return self._check(y)

    def affine(self, y, sc, sh, slope=None):
        """sc * y + sh with sc = +-1/2, then the leaky ReLU unless slope is None"""
        z = sc.double() * y + sh.double()
        self.q /= 2
        self._check(z)
        if slope is None:
            return z
        self.q *= slope if slope else 1.0
        return self._check(_act(z, slope))

    def stack(self, z, P, slope, last_act=True):
        Ws, scales, shifts = P
        for l, (W, sc, sh) in enumerate(zip(Ws, scales, shifts)):
            z = self.affine(self.linear(z, W), sc, sh, slope if (last_act or l + 1 < len(Ws)) else None)
        return z


def _cloud_max(z, n):
    return torch.stack([z[b, :n[b]].max(dim=0)[0] for b in range(z.shape[0])])


def _points(B, N, n_valid, dev):
    """Integer coordinates in [-4, 4] as a loader's [B,N,3]; -> (pts for the fp64 side, pts with NaN pad rows, counts, n_valid tensor)"""
    g = torch.Generator().manual_seed(B * 10007 + N)
    pts = torch.randint(-4, 5, (B, N, 3), generator=g).float().to(dev)
    n = [N] * B if n_valid is None else n_valid
    nv, padded = None, pts
    if n_valid is not None:
        nv = torch.tensor(n_valid, dtype=torch.int32, device=dev)
        padded = pts.clone()
        for b in range(B):
            padded[b, n[b]:] = NAN
    return pts, padded, n, nv


def _valid_mask(B, N, n, dev):
    return (torch.arange(N, device=dev).view(1, N) < torch.tensor(n, device=dev).view(B, 1)).reshape(B * N)


def _int_rows(B, N, C, n, seed, dev):
    """[B*N, C] integers in [-4, 4] on the valid rows, NaN on the pad rows; and the same with zeros for the fp64 side"""
    g = torch.Generator().manual_seed(seed)
    clean = torch.randint(-4, 5, (B * N, C), generator=g).float().to(dev)
    valid = _valid_mask(B, N, n, dev)
    return clean, torch.where(valid[:, None], clean, torch.full_like(clean, NAN)), valid


@pytest.mark.parametrize("B,N,n_valid", SHAPES)
@pytest.mark.parametrize("slope", SLOPES)
def test_stn_exact_bit_for_bit(dev, B, N, n_valid, slope):
    P = _exact_stack((3, 64, 128, 1024), 11)
    pts, padded, n, nv = _points(B, N, n_valid, dev)
    want = _cloud_max(_Exact().stack(pts.double(), P, slope), n).float()
    cf = padded.transpose(1, 2).contiguous()                                         # [B,3,N] dense, the network's layout
    got_nl = _call_stn(padded.transpose(1, 2), nv, P, slope)                         # [B,N,3] strides
    got_cf = _call_stn(cf, nv, P, slope)
    again = _call_stn(cf, nv, P, slope)
    torch.cuda.synchronize()
    assert bool((got_cf[:, 1024:] == 7.0).all()) and bool((got_nl[:, 1024:] == 7.0).all()), "wrote beyond column 1024"
    assert torch.equal(got_cf, again), "two calls differ"
    assert torch.equal(got_cf, got_nl), "the two layouts differ"
    assert torch.equal(got_cf[:, :1024], want), f"max |diff| {(got_cf[:, :1024] - want).abs().max().item():.3e}"


def _signed_perm(g, k):
    """[k, k] with one +-1 per row and column"""
    T = torch.zeros(k, k)
    T[torch.arange(k), torch.randperm(k, generator=g)] = torch.randint(0, 2, (k,), generator=g).float() * 2 - 1
    return T


@pytest.mark.parametrize("B,N,n_valid", SHAPES)
@pytest.mark.parametrize("slope", SLOPES)
def test_trunk_exact_bit_for_bit(dev, B, N, n_valid, slope):
    Pc, Ps = _exact_stack((3, 64, 128, 128), 12), _exact_stack((128, 64, 128, 1024), 13)
    pts, padded, n, nv = _points(B, N, n_valid, dev)
    g = torch.Generator().manual_seed(5 + B)
    T3 = torch.stack([_signed_perm(g, 3) for _ in range(B)]).to(dev)                 # a signed permutation per cloud
    ex = _Exact()
    z, outs = ex.linear(pts.double(), torch.eye(3, device=dev)) @ T3.double(), []
    for l in range(3):
        z = ex.stack(z, ([Pc[0][l]], [Pc[1][l]], [Pc[2][l]]), slope)
        outs.append(z)
    want_rows = torch.cat(outs, dim=2).reshape(B * N, 320).float()
    want = _cloud_max(ex.stack(z, Ps, slope), n).float()
    cf = padded.transpose(1, 2).contiguous()
    F_nl, got_nl = _call_trunk(padded.transpose(1, 2), nv, T3, Pc, Ps, slope)
    F_cf, got_cf = _call_trunk(cf, nv, T3, Pc, Ps, slope)
    F_again, again = _call_trunk(cf, nv, T3, Pc, Ps, slope)
    torch.cuda.synchronize()
    valid = _valid_mask(B, N, n, dev)
    assert bool((got_cf[:, 1024:] == 7.0).all()), "wrote beyond column 1024"
    assert bool(torch.isnan(F_cf[:, 320:]).all()) and bool(torch.isnan(F_cf[~valid]).all()), "wrote F outside rows < n_b, columns < 320"
    assert torch.equal(got_cf, again) and torch.equal(F_cf[valid, :320], F_again[valid, :320]), "two calls differ"
    assert torch.equal(got_cf, got_nl) and torch.equal(F_cf[valid, :320], F_nl[valid, :320]), "the two layouts differ"
    assert torch.equal(F_cf[valid, :320], want_rows[valid]), "out1 | out2 | out3"
    assert torch.equal(got_cf[:, :1024], want), f"max |diff| {(got_cf[:, :1024] - want).abs().max().item():.3e}"


@pytest.mark.parametrize("B,N,n_valid", SHAPES)
@pytest.mark.parametrize("slope", SLOPES)
def test_global_exact_bit_for_bit(dev, B, N, n_valid, slope):
    P = _exact_stack((128, 512, 2048), 14)
    n = [N] * B if n_valid is None else n_valid
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32, device=dev)
    out3, out3_nan, valid = _int_rows(B, N, 128, n, B * 31 + N, dev)
    g = torch.Generator().manual_seed(7 + B)
    T128 = torch.stack([_signed_perm(g, 128) for _ in range(B)]).to(dev)             # one +-1 per row and column, per cloud
    TT = T128.transpose(1, 2).contiguous()
    ex = _Exact()
    nt = torch.bmm(ex.linear(out3.double(), torch.eye(128, device=dev)).view(B, N, 128), T128.double())
    out4 = ex.stack(nt, ([P[0][0]], [P[1][0]], [P[2][0]]), slope)
    out5 = ex.stack(out4, ([P[0][1]], [P[1][1]], [P[2][1]]), slope, last_act=False)
    want = _cloud_max(out5, n).float()

    def run():
        F = torch.full((B * N, LDF), NAN, device=dev)
        F[:, 192:320] = out3_nan
        return F, _call_global(F, nv, B, N, TT, P, slope)

    F, got = run()
    F2, again = run()
    torch.cuda.synchronize()
    assert bool((got[:, 2048:] == 7.0).all()), "wrote beyond column 2048"
    assert bool(torch.isnan(F[:, :192]).all()) and bool(torch.isnan(F[:, 832:]).all()) and bool(torch.isnan(F[~valid]).all())
    assert torch.equal(F[valid, 192:320], out3[valid]), "out3 changed"
    assert torch.equal(got, again) and torch.equal(F[valid, 320:832], F2[valid, 320:832]), "two calls differ"
    assert torch.equal(F[valid, 320:832], out4.reshape(B * N, 512).float()[valid]), "out4"
    assert torch.equal(got[:, :2048], want), f"max |diff| {(got[:, :2048] - want).abs().max().item():.3e}"


@pytest.mark.parametrize("B,N,n_valid", SHAPES)
@pytest.mark.parametrize("part_num", [50, 6])
@pytest.mark.parametrize("slope", SLOPES)
def test_head_exact_bit_for_bit(dev, B, N, n_valid, part_num, slope):
    P = _exact_stack((832, 256, 256, 128), 15)
    n = [N] * B if n_valid is None else n_valid
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32, device=dev)
    rows, rows_nan, valid = _int_rows(B, N, 832, n, B * 37 + N, dev)
    g = torch.Generator().manual_seed(9 + part_num)
    bias = torch.randint(-3, 4, (B, 256), generator=g).float().to(dev)               # the per-cloud bias: small integers
    padded_rows = -(-part_num // 32) * 32
    Wout = torch.full((padded_rows, 128), NAN, device=dev)                           # rows >= part_num reach no result
    Wout[:part_num] = _signed_rows(g, part_num, 128).to(dev)
    bout = torch.randint(-2, 3, (part_num,), generator=g).float().to(dev)
    ex = _Exact()
    y = ex.linear(rows.double().view(B, N, 832), P[0][0], add=bias.double()[:, None, :])
    z = ex.affine(y, P[1][0], P[2][0], slope)
    z = ex.stack(z, ([P[0][1], P[0][2]], [P[1][1], P[1][2]], [P[2][1], P[2][2]]), slope)
    logits = ex.linear(z, Wout[:part_num], add=bout.double()).float()                # [B, N, part_num]
    want = torch.where(valid.view(B, N, 1), logits, torch.zeros_like(logits)).permute(0, 2, 1)

    def run():
        F = torch.full((B * N, LDF), NAN, device=dev)
        F[:, :832] = rows_nan
        return _call_head(F, nv, B, N, bias, P, Wout, bout, part_num, slope)

    buf, again = run(), run()
    torch.cuda.synchronize()
    assert bool((buf[:, part_num:] == 7.0).all()) and bool((buf[:, :, N:] == 7.0).all()), "wrote outside [B, part_num, N]"
    assert torch.equal(buf, again), "two calls differ"
    got = buf[:, :part_num, :N]
    assert bool((got.permute(0, 2, 1).reshape(B * N, part_num)[~valid] == 0.0).all()), "logits of pad points must be exact zeros"
    assert torch.equal(got, want), f"max |diff| {(got - want).abs().max().item():.3e}"


@pytest.mark.parametrize("K,C", [(1024, 512), (256, 9), (2064, 256)])
def test_rows_exact_and_independent_of_the_row_count(dev, K, C):
    g = torch.Generator().manual_seed(K + C)
    x = torch.randint(-4, 5, (5, K), generator=g).float().to(dev)
    W = _signed_rows(g, C, K, nz=16).to(dev)
    scale = ((torch.randint(0, 2, (C,), generator=g).float() * 2 - 1) / 2).to(dev)
    shift = torch.randint(-2, 3, (C,), generator=g).float().to(dev)
    ex = _Exact()
    want = ex.affine(ex.linear(x.double(), W), scale, shift, 0.5).float()
    got = _call_rows(x, W, scale, shift, 0.5)
    plain = _call_rows(x, W, None, shift, 1.0)
    torch.cuda.synchronize()
    assert bool((got[:, C:] == 7.0).all())
    assert torch.equal(got[:, :C], want)
    assert torch.equal(plain[:, :C], (x.double() @ W.double().t() + shift.double()).float())
    xr = torch.randn(5, K, generator=g).to(dev)                                      # random data: a row alone gives the same bits
    Wr = torch.randn(C, K, generator=g).to(dev)
    full = _call_rows(xr, Wr, scale, shift, 0.2)
    ref = _act(scale.double() * (xr.double() @ Wr.double().t()) + shift.double(), 0.2)
    for r in range(5):
        assert torch.equal(_call_rows(xr[r:r + 1], Wr, scale, shift, 0.2)[0], full[r])
    # one fp32 chain of at most 36 terms per lane and a 6-level tree: a generous K * 2^-24 * sum |products| bounds the rounding
    bound = K * 2.0 ** -24 * (xr.double().abs() @ Wr.double().abs().t()).max().item()
    assert _err(full[:, :C], ref) <= bound


# ----------------------------------------------------------------------------------------------------------- networks
def _net(dev, seed=0, slope=0.0, part_num=50, head_mid=None):
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
    torch.manual_seed(seed)
    net = PointNet_partseg(part_num=part_num)
    if head_mid is not None:                                   # one changed width: the head's second layer
        net.convs = PointwiseMLP([4944, 256, head_mid, 128], bias=True)
    for m in net.modules():
        if isinstance(m, PointwiseMLP):
            m.slope = float(slope)
    return _perturb(net.to(dev), seed + 1)


@functools.lru_cache(maxsize=None)
def _inputs(B, N, seed=0):
    """(points [B,N,3], one-hot label [B,16]); read only"""
    from pointcloudlib_amd import synth
    pts = torch.from_numpy(synth.gauss_ball(B, N, seed)).cuda()
    label = torch.nn.functional.one_hot(torch.arange(B) % 16, 16).float().cuda()
    return pts, label


def _mlp64(mlp, z):
    for l in range(mlp.n_layers):
        W, sc, sh = _consts64(mlp, l)
        z = sc * (z @ W.t()) + sh
        if mlp.last_act or l + 1 < mlp.n_layers:
            z = _act(z, mlp.slope)
    return z


def _tnet64(tnet, z):
    """z [n, k] fp64 -> [k, k]"""
    g = _mlp64(tnet.convs, z).max(dim=0)[0]
    t = _mlp64(tnet.fcs, g[None]) @ tnet.fc3.weight.double().t() + tnet.fc3.bias.double()
    return (t + torch.eye(tnet.k, device=z.device, dtype=torch.float64).reshape(1, -1)).reshape(tnet.k, tnet.k)


def _ref_partseg(net, pts, label, n):
    """fp64 evaluation-mode restatement of PointNet_partseg.forward, cloud by cloud on its first n[b] points:
    -> (T3 [B,3,3], T128 [B,128,128], out_max [B,2048], [logits [part_num, n_b]])"""
    T3s, T128s, maxs, logits = [], [], [], []
    for b in range(pts.shape[0]):
        x = pts[b, :n[b]].double()
        T3 = _tnet64(net.stn, x)
        out1 = _mlp64(net.conv1, x @ T3)
        out2 = _mlp64(net.conv2, out1)
        out3 = _mlp64(net.conv3, out2)
        T128 = _tnet64(net.fstn, out3)
        out4 = _mlp64(net.conv4, out3 @ T128)
        out5 = _mlp64(net.conv5, out4)
        out_max = out5.max(dim=0)[0]
        expand = torch.cat([out_max, label[b].double()])[None].expand(n[b], -1)
        h = _mlp64(net.convs, torch.cat([expand, out1, out2, out3, out4, out5], dim=1))
        logits.append((h @ net.convs4.weight.double().t() + net.convs4.bias.double()).t())
        T3s.append(T3); T128s.append(T128); maxs.append(out_max)
    return torch.stack(T3s), torch.stack(T128s), torch.stack(maxs), logits


def _eval_parts(ev, x, label):
    """net.eval()'s own intermediate tensors, by the statements of PointNet_partseg.forward"""
    pc = x.transpose(1, 2).contiguous()
    T3 = ev.stn(pc)
    out3 = ev.conv3(ev.conv2(ev.conv1(torch.bmm(pc, T3))))
    T128 = ev.fstn(out3)
    out_max = ev.conv5(ev.conv4(torch.bmm(out3, T128))).max(dim=1)[0]
    return T3, T128, out_max, ev(x, label)


@pytest.mark.parametrize("seed,slope", [(0, 0.0), (1, 0.2), (2, 0.0)])
def test_frozen_partseg_against_fp64(dev, seed, slope):
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    net = _net(dev, seed, slope)
    B, N = 4, 300
    pts, label = _inputs(B, N, seed)
    ref = _ref_partseg(net, pts, label, [N] * B)
    ref = ref[:3] + (torch.stack(ref[3]),)
    x = pts.transpose(1, 2)                                                          # [B,3,N], strides of [B,N,3]
    fnet = FrozenPointNetPartseg(net)
    assert fnet.plan == "fused"
    got = fnet.run(x, label)
    ev = copy.deepcopy(net).eval()
    with torch.no_grad():
        evs = _eval_parts(ev, x.contiguous(), label)
    torch.cuda.synchronize()
    assert got[3].shape == (B, 50, N) and got[3].shape == evs[3].shape
    failed = []
    for name, g, e, r in zip(("T3", "T128", "out_max", "logits"), got, evs, ref):
        ef, ee = _err(g, r), _err(e, r)
        print(f"seed {seed} slope {slope} {name}: frozen {ef:.3e} eval {ee:.3e}")
        if not ef <= 1.25 * ee + 1e-6:
            failed.append(f"{name}: frozen {ef:.3e} vs eval {ee:.3e} from fp64")
    assert not failed, "; ".join(failed)


def test_frozen_partseg_ragged_equals_alone(dev):
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    net = _net(dev, 3, 0.2)
    B, N = 5, 200
    pts, label = _inputs(B, N, 3)
    pts = pts.clone()
    for b in range(B):
        pts[b, RAGGED[b]:] = NAN
    fnet = FrozenPointNetPartseg(net)
    _, _, out_max, logits = fnet.run(pts.transpose(1, 2), label, RAGGED)
    on_device = fnet(pts.transpose(1, 2), label, torch.tensor(RAGGED, dtype=torch.int32, device=dev))
    assert torch.equal(on_device, logits), "host and device lengths differ"
    assert logits.shape == (B, 50, N) and not bool(torch.isnan(logits).any()) and not bool(torch.isnan(out_max).any())
    ref = _ref_partseg(net, pts, label, RAGGED)
    for b in range(B):
        n = RAGGED[b]
        assert bool((logits[b, :, n:] == 0.0).all()), f"cloud {b}: logits of pad points must be exact zeros"
        _, _, alone_max, alone = fnet.run(pts[b:b + 1, :n].contiguous().transpose(1, 2), label[b:b + 1])
        assert torch.equal(alone[0], logits[b, :, :n]), f"cloud {b} alone: logits"
        assert torch.equal(alone_max[0], out_max[b]), f"cloud {b} alone: out_max"
        assert _err(logits[b, :, :n], ref[3][b]) < 1e-2 * max(1.0, ref[3][b].abs().max().item()), f"cloud {b}: far from fp64"


def _changed_net(dev):
    return _net(dev, 4, 0.0, head_mid=192)


def test_module_plan_equals_eval(dev):
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    from pointcloudlib_amd.misc.ops import unpack_rows
    net = _changed_net(dev)
    B, N = 5, 200
    pts, label = _inputs(B, N, 4)
    x = pts.transpose(1, 2).contiguous()
    fnet = FrozenPointNetPartseg(net)
    assert fnet.plan == "module"
    ev = copy.deepcopy(net).eval()
    lengths = torch.tensor(RAGGED, dtype=torch.int32, device=dev)
    with torch.no_grad():
        want = ev(x, label)
        rows, row_off = ev.forward_packed(x, label, RAGGED)
        want_ragged = unpack_rows(rows, lengths, row_off, N).permute(0, 2, 1)
    assert torch.equal(fnet(x, label), want)
    got = fnet(x, label, RAGGED)
    assert got.shape == (B, 50, N) and torch.equal(got, want_ragged)
    for b in range(B):
        assert bool((got[b, :, RAGGED[b]:] == 0.0).all())


def test_frozen_partseg_forward_memory(dev):
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    net = _net(dev)
    B, N = 4, 2048
    pts, label = _inputs(B, N)
    x = pts.transpose(1, 2)
    concat = B * N * 4944 * 4                                  # the tensor net.eval() materialises

    def peak(fn):
        fn()                                                   # warm-up: one-time allocations
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        assert out.shape == (B, 50, N)
        return torch.cuda.max_memory_allocated() - base

    fnet = FrozenPointNetPartseg(net)
    ev = copy.deepcopy(net).eval()
    xc = x.contiguous()

    def eval_forward():
        with torch.no_grad():
            return ev(xc, label)

    p_frozen, p_eval = peak(lambda: fnet(x, label)), peak(eval_forward)
    print(f"peak above the inputs: frozen {p_frozen / 2**20:.1f} MiB, eval {p_eval / 2**20:.1f} MiB, concat {concat / 2**20:.1f} MiB")
    assert p_frozen < concat / 4, f"frozen forward peak +{p_frozen / 2**20:.1f} MiB >= a quarter of the concat, {concat / 2**22:.1f} MiB"
    assert p_eval > concat, f"eval forward peak +{p_eval / 2**20:.1f} MiB <= the concat, {concat / 2**20:.1f} MiB"


def test_frozen_partseg_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    net = _net(dev, 5).train()
    pts, label = _inputs(4, 300, 5)
    x = pts.transpose(1, 2)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = FrozenPointNetPartseg(net)
    out = fnet(x, label)
    torch.cuda.synchronize()
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    for change in (lambda: net.conv5.running_var_0.mul_(3.0), lambda: net.convs.weights[0].mul_(1.5), lambda: net.fstn.fc3.weight.mul_(0.5)):
        with torch.no_grad():
            change()
        stale = fnet(x, label)
        fresh = fnet.refresh()(x, label)
        torch.cuda.synchronize()
        assert torch.equal(stale, out)
        assert not torch.equal(fresh, out)
        assert torch.equal(fresh, FrozenPointNetPartseg(net)(x, label))
        out = fresh
    with pytest.raises(TypeError):
        fnet(x.double(), label)
    with pytest.raises(TypeError):
        fnet(x, label.long())
    with pytest.raises(TypeError):
        fnet(x.cpu(), label.cpu())
    with pytest.raises(ValueError):
        fnet(pts, label)                                       # [B,N,3]
    with pytest.raises(ValueError):
        fnet(x, label[:, :15])
    with pytest.raises(ValueError):
        fnet(x, label, [300, 300, 300])                        # three counts for four clouds
