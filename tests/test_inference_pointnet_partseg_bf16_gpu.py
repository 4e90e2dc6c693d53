"""bf16 frozen PointNet part segmentation on the GPU (``FrozenPointNetPartseg(net, precision="bf16")``,
pcl_pointnet_seg_global_infer_bf16_f32 / pcl_pointnet_seg_head_infer_bf16_f32, csrc/infer_pointnet_seg.hip): both entries bit for
bit against fp64 and against their fp32 counterparts on data that keeps every rounded activation bf16-representable; random data
against the yardstick of tests/pointnet_partseg_bf16_yardstick.py; the class on ragged batches and against its fp32 form."""
import functools

import pytest
import torch

import pointnet_partseg_bf16_yardstick as ys
from test_inference_pointnet_partseg_gpu import (LDF, NAN, RAGGED, SHAPES, SLOPES, _arr, _cloud_max, _Exact, _inputs, _lib, _mlp64, _net, _P,
                                                 _part_ws, _rows_bytes, _signed_perm, _signed_rows, _stream, _valid_mask, _w)

pytestmark = pytest.mark.gpu

GLOBAL = {"fp32": "pcl_pointnet_seg_global_infer_f32", "bf16": "pcl_pointnet_seg_global_infer_bf16_f32"}
HEAD = {"fp32": "pcl_pointnet_seg_head_infer_f32", "bf16": "pcl_pointnet_seg_head_infer_bf16_f32"}


def _operands(Ws, precision):
    return [w.to(torch.bfloat16).contiguous() for w in Ws] if precision == "bf16" else list(Ws)


def _call_global(precision, F, nv, B, N, TT, P, slope, ldo=2048 + 8):
    """F [B*N, LDF] is updated in place (columns 320..831) -> out [B, ldo] prefilled with 7; the workspace starts as NaN"""
    Ws, sc, sh = P
    ops = _operands(Ws, precision)
    ws, need = _part_ws(B, N, 2048, F.device)
    out = torch.full((B, ldo), 7.0, device=F.device)
    _lib().call(GLOBAL[precision], _P(F), LDF, _rows_bytes(B, N), _P(nv), B, N, _P(TT), 2, _w([w.shape[0] for w in Ws]), _arr(ops), _arr(sc),
                _arr(sh), float(slope), _P(ws), need, _P(out), ldo, _stream())
    return out


def _call_head(precision, F, nv, B, N, bias, P, Wout, bout, part_num, slope, points_major=False):
    """-> the whole output buffer prefilled with 7: [B, part_num + 1, N + 3] with the logits in [:, :part_num, :N], or
    (points_major) [B, N + 3, part_num + 1] with the logits in [:, :N, :part_num]"""
    Ws, sc, sh = P
    ops = _operands(list(Ws) + [Wout], precision)
    if points_major:
        buf = torch.full((B, N + 3, part_num + 1), 7.0, device=F.device)
        out = buf[:, :N, :part_num].permute(0, 2, 1)
    else:
        buf = torch.full((B, part_num + 1, N + 3), 7.0, device=F.device)
        out = buf[:, :part_num, :N]
    _lib().call(HEAD[precision], _P(F), LDF, _rows_bytes(B, N), _P(nv), B, N, _P(bias), bias.stride(0), 4,
                _w([w.shape[0] for w in Ws] + [part_num]), _arr(ops), Wout.shape[0], _arr(sc), _arr(sh), _P(bout), float(slope), _P(out),
                out.stride(0), out.stride(1), out.stride(2), _stream())
    return buf


# ----------------------------------------------------------------------------------------------------------- exact data
@functools.lru_cache(maxsize=None)
def _exact_stack(spec, seed, nz, shift_max, negative):
    """Made once, read only: weight rows of ``nz`` entries of +-1, shift an integer in [-shift_max, shift_max], scale +-1/2 --
    ``negative``: the share of negative scales of the LAST layer (the others: half)."""
    g = torch.Generator().manual_seed(seed)
    Ws, scales, shifts = [], [], []
    for l, (cin, cout) in enumerate(zip(spec[:-1], spec[1:])):
        Ws.append(_signed_rows(g, cout, cin, nz).cuda())
        sign = torch.ones(cout)
        share = negative if l + 2 == len(spec) else 0.5
        sign[torch.randperm(cout, generator=g)[:int(cout * share)]] = -1.0
        scales.append((sign / 2).cuda())
        shifts.append(torch.randint(-shift_max, shift_max + 1, (cout,), generator=g).float().cuda())
    return Ws, scales, shifts


def _int_rows(B, N, C, n, seed, dev, amp):
    """[B*N, C] integers in [-amp, amp]; the same with NaN on the pad rows; the mask of valid rows"""
    g = torch.Generator().manual_seed(seed)
    clean = torch.randint(-amp, amp + 1, (B * N, C), generator=g).float().to(dev)
    valid = _valid_mask(B, N, n, dev)
    return clean, torch.where(valid[:, None], clean, torch.full_like(clean, NAN)), valid


def _representable(z, what):
    """A rounding point of the contract: the rounding must be the identity (taken on the CPU, where ldexp is exact)"""
    assert torch.equal(ys.round_bf16(z.cpu()), z.cpu()), f"{what} is not bf16-representable: the data does not test what it should"
    return z


@pytest.mark.parametrize("B,N,n_valid", SHAPES)
@pytest.mark.parametrize("slope", SLOPES)
def test_global_bf16_exact_bit_for_bit(dev, B, N, n_valid, slope):
    P = _exact_stack((128, 512, 2048), 24, 4, 2, 0.25)
    assert int((P[1][1] < 0).sum()) == 512                                           # a quarter of conv5's scales
    n = [N] * B if n_valid is None else n_valid
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32, device=dev)
    out3, out3_nan, valid = _int_rows(B, N, 128, n, B * 31 + N, dev, 4)
    g = torch.Generator().manual_seed(7 + B)
    T128 = torch.stack([_signed_perm(g, 128) for _ in range(B)]).to(dev)
    TT = T128.transpose(1, 2).contiguous()
    ex = _Exact()
    x2 = _representable(torch.bmm(ex.linear(out3.double(), torch.eye(128, device=dev)).view(B, N, 128), T128.double()), "x2")
    out4 = _representable(ex.stack(x2, ([P[0][0]], [P[1][0]], [P[2][0]]), slope), "out4")
    out5 = ex.stack(out4, ([P[0][1]], [P[1][1]], [P[2][1]]), slope, last_act=False)
    want = _cloud_max(out5, n).float()

    def run(precision):
        F = torch.full((B * N, LDF), NAN, device=dev)
        F[:, 192:320] = out3_nan
        return F, _call_global(precision, F, nv, B, N, TT, P, slope)

    F, got = run("bf16")
    F2, again = run("bf16")
    F32, got32 = run("fp32")
    torch.cuda.synchronize()
    assert bool((got[:, 2048:] == 7.0).all()), "wrote beyond column 2048"
    assert bool(torch.isnan(F[:, :192]).all()) and bool(torch.isnan(F[:, 832:]).all()) and bool(torch.isnan(F[~valid]).all())
    assert torch.equal(F[valid, 192:320], out3[valid]), "out3 changed"
    assert torch.equal(got, again) and torch.equal(F[valid, 320:832], F2[valid, 320:832]), "two calls differ"
    assert torch.equal(F[valid, 320:832], out4.reshape(B * N, 512).float()[valid]), "out4"
    assert torch.equal(F[valid, 320:832], F32[valid, 320:832]), "F[., 320:832] differs from the fp32 launch's"
    assert torch.equal(got[:, :2048], want), f"max |diff| {(got[:, :2048] - want).abs().max().item():.3e}"
    assert torch.equal(got, got32), "differs from the fp32 launch"


@pytest.mark.parametrize("B,N,n_valid", SHAPES)
@pytest.mark.parametrize("part_num", [50, 6])
@pytest.mark.parametrize("slope", SLOPES)
def test_head_bf16_exact_bit_for_bit(dev, B, N, n_valid, part_num, slope):
    # two entries per weight row, |F| <= 2, |shift| and |bias| <= 1: z_3 stays within 176 quanta, 8 significant bits
    P = _exact_stack((832, 256, 256, 128), 25, 2, 1, 0.5)
    n = [N] * B if n_valid is None else n_valid
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32, device=dev)
    rows, rows_nan, valid = _int_rows(B, N, 832, n, B * 37 + N, dev, 2)
    g = torch.Generator().manual_seed(9 + part_num)
    bias = torch.randint(-1, 2, (B, 256), generator=g).float().to(dev)
    padded_rows = -(-part_num // 32) * 32
    Wout = torch.full((padded_rows, 128), NAN, device=dev)                           # rows >= part_num reach no result
    Wout[:part_num] = _signed_rows(g, part_num, 128).to(dev)
    bout = torch.randint(-2, 3, (part_num,), generator=g).float().to(dev)
    ex = _Exact()
    z = _representable(rows.double().view(B, N, 832), "F")
    for l in range(3):
        y = ex.linear(z, P[0][l], add=bias.double()[:, None, :] if l == 0 else None)
        z = _representable(ex.affine(y, P[1][l], P[2][l], slope), f"z_{l + 1}")
    logits = ex.linear(z, Wout[:part_num], add=bout.double()).float()                # [B, N, part_num]
    want = torch.where(valid.view(B, N, 1), logits, torch.zeros_like(logits)).permute(0, 2, 1)

    def run(precision, points_major=False):
        F = torch.full((B * N, LDF), NAN, device=dev)
        F[:, :832] = rows_nan
        return _call_head(precision, F, nv, B, N, bias, P, Wout, bout, part_num, slope, points_major)

    buf, again, pm, buf32 = run("bf16"), run("bf16"), run("bf16", True), run("fp32")
    torch.cuda.synchronize()
    assert bool((buf[:, part_num:] == 7.0).all()) and bool((buf[:, :, N:] == 7.0).all()), "wrote outside [B, part_num, N]"
    assert bool((pm[:, N:] == 7.0).all()) and bool((pm[:, :, part_num:] == 7.0).all()), "wrote outside [B, N, part_num]"
    assert torch.equal(buf, again), "two calls differ"
    got = buf[:, :part_num, :N]
    assert torch.equal(pm[:, :N, :part_num].permute(0, 2, 1), got), "the two output layouts differ"
    assert bool((got.permute(0, 2, 1).reshape(B * N, part_num)[~valid] == 0.0).all()), "logits of pad points must be exact zeros"
    assert torch.equal(got, want), f"max |diff| {(got - want).abs().max().item():.3e}"
    assert torch.equal(buf, buf32), "differs from the fp32 launch"


# ----------------------------------------------------------------------------------------------------------- random data
@pytest.mark.parametrize("seed,slope", [(0, 0.0), (1, 0.2)])
def test_global_bf16_against_the_yardstick(dev, seed, slope):
    B, N = 4, 129
    out3, T128, Ws, sc, sh = ys.global_case(seed, B, N, dev)
    n = [N] * B
    Wl = ys.launch_weights(Ws)
    want, T, ref, worst, out4 = ys.global_want_and_bounds(out3, n, T128, Wl, sc, sh, slope)
    F = torch.full((B * N, LDF), NAN, device=dev)
    F[:, 192:320] = out3.reshape(B * N, 128)
    got = _call_global("bf16", F, None, B, N, T128.transpose(1, 2).contiguous(), (Ws, sc, sh), slope)
    torch.cuda.synchronize()
    ys.check(got[:, :2048], want, T, ref, worst, f"global seed {seed} slope {slope}")
    # out4 in F is the unrounded fp32 epilogue of one bf16 layer: within its worst-case bound of the fp64 restatement
    F4 = F.view(B, N, LDF)[:, :, 320:832].double()
    for b in range(B):
        a4, e4 = out4[b]
        assert bool(((F4[b] - a4).abs() <= e4).all()), f"cloud {b}: out4 beyond its worst-case bound"


@pytest.mark.parametrize("seed,slope", [(0, 0.0), (1, 0.2)])
def test_head_bf16_against_the_yardstick(dev, seed, slope):
    B, N, part_num = 4, 129, 50
    Fr, bias, Ws, sc, sh, Wout, bout = ys.head_case(seed, B, N, part_num, dev)
    Wp = torch.zeros(64, 128, device=dev)
    Wp[:part_num] = Wout
    want, T, ref, worst = ys.head_want_and_bounds(Fr, bias, ys.launch_weights(Ws), sc, sh, Wout.to(torch.bfloat16), bout, slope)
    F = torch.full((B * N, LDF), NAN, device=dev)
    F[:, :832] = Fr.reshape(B * N, 832)
    buf = _call_head("bf16", F, None, B, N, bias, (Ws, sc, sh), Wp, bout, part_num, slope)
    torch.cuda.synchronize()
    ys.check(buf[:, :part_num, :N].permute(0, 2, 1), want, T, ref, worst, f"head seed {seed} slope {slope}")


# ----------------------------------------------------------------------------------------------------------- the class
def test_bf16_ragged_equals_alone_and_front_equals_fp32(dev):
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    net = _net(dev, 3, 0.2)
    B, N = 5, 200
    pts, label = _inputs(B, N, 3)
    pts = pts.clone()
    for b in range(B):
        pts[b, RAGGED[b]:] = NAN
    fnet, f32 = FrozenPointNetPartseg(net, precision="bf16"), FrozenPointNetPartseg(net)
    assert fnet.plan == "fused" and fnet.precision == "bf16"
    T3, T128, out_max, logits = fnet.run(pts.transpose(1, 2), label, RAGGED)
    T3_32, T128_32, _, logits32 = f32.run(pts.transpose(1, 2), label, RAGGED)
    assert torch.equal(T3, T3_32) and torch.equal(T128, T128_32), "the front launches must not depend on the precision"
    assert not torch.equal(logits, logits32), "the bf16 instance ran the fp32 launches"
    assert logits.shape == (B, 50, N) and not bool(torch.isnan(logits).any()) and not bool(torch.isnan(out_max).any())
    for b in range(B):
        n = RAGGED[b]
        assert bool((logits[b, :, n:] == 0.0).all()), f"cloud {b}: logits of pad points must be exact zeros"
        _, _, alone_max, alone = fnet.run(pts[b:b + 1, :n].contiguous().transpose(1, 2), label[b:b + 1])
        assert torch.equal(alone[0], logits[b, :, :n]), f"cloud {b} alone: logits"
        assert torch.equal(alone_max[0], out_max[b]), f"cloud {b} alone: out_max"


def test_bf16_row_buffer_front_equals_fp32(dev, monkeypatch):
    """F[., :320] (out1 | out2 | out3) of a forward is the fp32 instance's; the row buffer is caught where the forward allocates it."""
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    net = _net(dev, 6, 0.0)
    B, N = 2, 100
    pts, label = _inputs(B, N, 6)
    real_empty, keep = torch.empty, {}

    def empty(*a, **kw):
        t = real_empty(*a, **kw)
        if t.dtype == torch.float32 and t.numel() == B * N * 832:
            keep["F"] = t
        return t

    monkeypatch.setattr(torch, "empty", empty)
    rows = {}
    for precision in ("fp32", "bf16"):
        FrozenPointNetPartseg(net, precision=precision)(pts.transpose(1, 2), label)
        torch.cuda.synchronize()
        rows[precision] = keep.pop("F").view(B * N, 832).clone()
    assert torch.equal(rows["bf16"][:, :320], rows["fp32"][:, :320])
    assert not torch.equal(rows["bf16"][:, 320:], rows["fp32"][:, 320:]) and not bool(torch.isnan(rows["bf16"]).any())


def test_bf16_network_against_fp32_instance(dev):
    """A perturbed network at B = 4, N = 300: the logits of both instances lie within the worst-case bf16 bound around an fp64
    evaluation -- the running bound of tests/bf16_bound.py over conv4, conv5 and the head's four layers, from the instances' common
    fp32 front (T3, T128) -- so they are within twice the bound of each other; the per-point top-1 agreement is printed."""
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    net = _net(dev, 1, 0.2)
    B, N = 4, 300
    pts, label = _inputs(B, N, 1)
    x = pts.transpose(1, 2)
    fnet, f32 = FrozenPointNetPartseg(net, precision="bf16"), FrozenPointNetPartseg(net)
    T3, T128, out_max, logits = fnet.run(x, label)
    _, _, out_max32, logits32 = f32.run(x, label)
    torch.cuda.synchronize()
    agree = (logits.argmax(dim=1) == logits32.argmax(dim=1)).double().mean().item()
    dist = (logits - logits32).abs().max().item()
    g, h, slope = fnet.glob, fnet.head, fnet.slope
    o1 = _mlp64(net.conv1, torch.bmm(pts.double(), T3.double()))
    o2 = _mlp64(net.conv2, o1)
    o3 = _mlp64(net.conv3, o2)
    Wg = fnet.Wglob.double()
    ref, bound, gref, gbound = [], [], [], []
    for b in range(B):
        a = o3[b] @ T128[b].double()
        e = 2 * 128 * ys.EPS * (o3[b].abs() @ T128[b].double().abs())
        a4, e4 = ys._bf16_layer(a, e, g.Ws[0], g.scales[0], g.shifts[0], slope)
        a5, e5 = ys._bf16_layer(a4, e4, g.Ws[1], g.scales[1], g.shifts[1], None)
        gmax, egmax = a5.max(dim=0)[0], e5.max(dim=0)[0]
        glob = torch.cat([gmax, label[b].double()])
        cb = Wg @ glob + fnet.c0.double()                                           # the per-cloud bias: an fp32 chain of 2064 terms
        ecb = Wg.abs()[:, :2048] @ egmax + 2064 * ys.EPS * (Wg.abs() @ glob.abs() + fnet.c0.double().abs())
        rows = torch.cat([o1[b], o2[b], o3[b], a4], dim=1)
        erows = torch.cat([torch.zeros_like(o1[b]), torch.zeros_like(o2[b]), torch.zeros_like(o3[b]), e4], dim=1)
        a1, e1 = ys._bf16_layer(rows, erows, h.Ws[0], h.scales[0], h.shifts[0], slope, add=cb[None, :])
        e1 = e1 + h.scales[0].double().abs() * ecb
        a2, e2 = ys._bf16_layer(a1, e1, h.Ws[1], h.scales[1], h.shifts[1], slope)
        a3, e3 = ys._bf16_layer(a2, e2, h.Ws[2], h.scales[2], h.shifts[2], slope)
        lo, elo = ys._bf16_layer(a3, e3, fnet.Wout[:fnet.part_num], None, fnet.bias_out, None)
        ref.append(lo.t()); bound.append(elo.t()); gref.append(gmax); gbound.append(egmax)
    ref, bound, gref, gbound = torch.stack(ref), torch.stack(bound), torch.stack(gref), torch.stack(gbound)
    r16, r32 = ys.bf16_bound.worst_ratio(logits, ref, bound), ys.bf16_bound.worst_ratio(logits32, ref, bound)
    rg = ys.bf16_bound.worst_ratio(out_max, gref, gbound)
    print(f"bf16 vs fp32 instance: top-1 agreement {100 * agree:.2f} %, max |logit distance| {dist:.3e} (max bound {bound.max().item():.3e}); "
          f"|logits - fp64| / bound: bf16 {r16:.4f}, fp32 {r32:.4f}; out_max bf16 {rg:.4f}")
    assert rg <= 1.0, f"out_max beyond the worst-case bound: ratio {rg:.3f}"
    assert r16 <= 1.0, f"logits beyond the worst-case bound: ratio {r16:.3f}"
    assert r32 <= 1.0 and bool(((logits.double() - logits32.double()).abs() <= 2 * bound).all())
