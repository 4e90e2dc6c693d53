"""The yardstick of the bf16 frozen-PointNet tests (``FrozenPointNet(net, precision="bf16")``, pcl_pointnet_stack_infer_bf16_f32).
TEST INFRASTRUCTURE, no test of its own; runs on any device.

The worst-case running bound of tests/bf16_bound.py compounds over four bf16 layers: at these widths a faithful emulation of the
contract sits at 0.0005 of it and one that drops 8 k of the last layer at 0.02 of it, so it would pass a mapping defect.  The
reference here is the numerics contract itself (csrc/infer_pointnet.hip), restated in fp64 WITH its roundings:

    the constants the launch is given (bf16 weights read as fp64; W0, scale, shift fp32 read as fp64); layer 1 in fp64; every
    z_1 .. z_4 rounded to bf16, round to nearest even, directly from fp64 (frexp / round(m * 256) / ldexp: no double rounding);
    want = max over each cloud's valid rows of z_5.

When no rounding decision differs between the kernel and this restatement, the only thing left to differ is the fp32
accumulation and epilogue of the last layer (eps = 2^-24, K = 128):

    e_y = 2 K eps (|z_4| |W_5|^T)            (2: an MFMA-internal add that truncates instead of rounding to nearest is allowed;
                                              the hardware's internal summation is not documented as round-to-nearest-even)
    e   = |sc| e_y + 4 eps (|sc y| + |sh| + |sc| e_y)
    T[c] = max of e over the cloud's valid rows

An fp32 value within its own rounding error of a bf16 midpoint may round the other way in the kernel than in fp64, which moves a
few outputs by about 2^-8 |z w|.  So |got - want| <= T must hold for all but at most CAP = 1 % of a case's B * 1024 outputs (a
cap, not a measurement), and each exception must still lie within the worst-case bound of ``bf16_bound.rows_ref_and_bound``, maxed
over the cloud's valid rows, around the UNROUNDED fp64 restatement.

``case`` is the data generator both the CPU and the GPU tests use; ``emulate_defect`` restates the contract in torch fp32 with one
defect each, for tests/test_inference_pointnet_bf16_cpu.py to show that the yardstick catches them."""
import torch

import bf16_bound

EPS = 2.0 ** -24
CAP = 0.01
SPEC = [3, 64, 64, 64, 128, 1024]


def round_bf16(x):
    """fp64 -> the nearest bf16 value (ties to even) as fp64, in one rounding."""
    m, e = torch.frexp(x)                                   # x = m * 2^e, 0.5 <= |m| < 1: 8 significant bits = round(m * 256)
    return torch.ldexp(torch.round(m * 256.0), e - 8)       # torch.round: half to even


def case(seed, B, N, device="cpu"):
    """-> (pts [B,N,3] fp32, Ws fp32 [C_l, C_{l-1}], scales, shifts): weights U(-1, 1) / sqrt(K), scale U(0.5, 1.5), shift
    N(0, 0.1), points N(0, 1) clamped to +-3."""
    g = torch.Generator().manual_seed(seed)
    Ws, scales, shifts = [], [], []
    for cin, cout in zip(SPEC[:-1], SPEC[1:]):
        Ws.append(((torch.rand(cout, cin, generator=g) * 2 - 1) / cin ** 0.5).to(device))
        scales.append((0.5 + torch.rand(cout, generator=g)).to(device))
        shifts.append((0.1 * torch.randn(cout, generator=g)).to(device))
    pts = torch.randn(B, N, 3, generator=g).clamp_(-3.0, 3.0).to(device)
    return pts, Ws, scales, shifts


def launch_weights(Ws):
    """The weights a bf16 launch is given: W0 fp32, W[l >= 1] rounded to bf16 once."""
    return [Ws[0]] + [w.to(torch.bfloat16).contiguous() for w in Ws[1:]]


def restate(pts, Wl, scales, shifts, slope):
    """The rounded restatement: pts [..., 3] (any float dtype), Wl the launch's constants -> (z_4 rounded, y_5, z_5), fp64."""
    W = [w.double() for w in Wl]
    sc, sh = [s.double() for s in scales], [s.double() for s in shifts]
    z = bf16_bound.act(sc[0] * (pts.double() @ W[0].t()) + sh[0], slope)
    for l in range(1, len(W) - 1):
        z = bf16_bound.act(sc[l] * (round_bf16(z) @ W[l].t()) + sh[l], slope)
    z4 = round_bf16(z)
    y5 = z4 @ W[-1].t()
    return z4, y5, bf16_bound.act(sc[-1] * y5 + sh[-1], slope)


def want_and_bounds(pts, n, Wl, scales, shifts, slope):
    """pts [B,N,3] (pad rows may hold anything), n per-cloud counts -> (want [B,1024], T [B,1024], unrounded fp64 restatement
    [B,1024], its worst-case bound [B,1024]), fp64."""
    want, T, ref, worst = [], [], [], []
    K = Wl[-1].shape[1]
    sc, sh, W5 = scales[-1].double(), shifts[-1].double(), Wl[-1].double()
    for b in range(pts.shape[0]):
        rows = pts[b, :n[b]]
        z4, y5, z5 = restate(rows, Wl, scales, shifts, slope)
        e_y = 2 * K * EPS * (z4.abs() @ W5.abs().t())
        e = sc.abs() * e_y + 4 * EPS * ((sc * y5).abs() + sh.abs() + sc.abs() * e_y)
        want.append(z5.max(dim=0)[0])
        T.append(e.max(dim=0)[0])
        a, ea = bf16_bound.rows_ref_and_bound(rows.double(), Wl, scales, shifts, slope)
        ref.append(a.max(dim=0)[0])
        worst.append(ea.max(dim=0)[0])
    return torch.stack(want), torch.stack(T), torch.stack(ref), torch.stack(worst)


def measure(got, want, T, ref, worst):
    """-> (worst |got - want| / T, share of the outputs over T, number of those beyond the worst-case bound)."""
    got = got.double()
    err = (got - want).abs()
    over = ~(err <= T)                                      # NaN counts as over
    outside = over & ~((got - ref).abs() <= worst)
    ratio = float(torch.where(err > 0, err / T, torch.zeros_like(err)).max())
    return ratio, float(over.double().mean()), int(outside.sum())


def check(got, want, T, ref, worst, label, cap=CAP):
    """Print the figures, then assert the yardstick."""
    ratio, share, outside = measure(got, want, T, ref, worst)
    print(f"{label}: worst |got - want| / T = {ratio:.3f}, share over T = {100 * share:.3f} %, beyond the worst-case bound: {outside}")
    assert share <= cap, f"{label}: {100 * share:.2f} % of the outputs over T (cap {100 * cap:g} %), worst ratio {ratio:.1f}"
    assert outside == 0, f"{label}: {outside} outputs beyond the worst-case bound"
    return ratio, share


def _trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate_defect(pts, Ws, scales, shifts, slope, defect):
    """``bf16_bound.emulate`` with one defect: "trunc" (activations truncated to bf16 instead of rounded to nearest), "drop_k4"
    (layer 4 loses one k, its busiest input channel), "fp32_w5" (the last layer's weights not rounded), "round_z5" (z_5 rounded to bf16).  pts [..., 3],
    Ws the fp32 weights -> rows [..., 1024] fp32."""
    rnd = _trunc_bf16 if defect == "trunc" else (lambda t: t.to(torch.bfloat16).float())
    a = bf16_bound.act(scales[0].float() * (pts.float() @ Ws[0].float().t()) + shifts[0].float(), slope)
    L = len(Ws)
    for l in range(1, L):
        Wb = Ws[l].float() if (defect == "fp32_w5" and l == L - 1) else Ws[l].float().to(torch.bfloat16).float()
        if defect == "drop_k4" and l == 3:
            Wb = Wb.clone()
            Wb[:, int(a.abs().reshape(-1, a.shape[-1]).mean(dim=0).argmax())] = 0.0       # the busiest input channel (a dead one shows nowhere)
        a = bf16_bound.act(scales[l].float() * (rnd(a) @ Wb.t()) + shifts[l].float(), slope)
    return a.to(torch.bfloat16).float() if defect == "round_z5" else a
