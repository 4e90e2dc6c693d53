"""The yardstick of the bf16 frozen PointNet part-seg tests (``FrozenPointNetPartseg(net, precision="bf16")``,
pcl_pointnet_seg_global_infer_bf16_f32 and pcl_pointnet_seg_head_infer_bf16_f32).  TEST INFRASTRUCTURE in the manner of
tests/pointnet_bf16_yardstick.py, no test of its own; runs on any device.

Per entry point the reference is the numerics contract itself (csrc/infer_pointnet_seg.hip), restated in fp64 WITH its roundings
(``round_bf16`` of tests/pointnet_bf16_yardstick.py: fp64 -> bf16 in one rounding, ties to even) on the constants the launch is
given (bf16 weights read as fp64; scale, shift, biases fp32 read as fp64):

    global   x2 = round(out3 . T128[b]);  z4 = act(sc4 * (x2 W4^T) + sh4), stored unrounded;  y5 = round(z4) W5^T;
             want[b] = max over the cloud's valid rows of sc5 * y5 + sh5                                     (no activation)
    head     z1 = act(sc1 * (round(F) W1^T + bias[b]) + sh1);  z2, z3 likewise on round(z1), round(z2);
             want = round(z3) Wout^T + bias_out                                                              (per point and part)

When no rounding decision differs between the kernel and the restatement, only the fp32 accumulation and epilogue of the LAST
layer are left to differ (eps = 2^-24; the 2: an MFMA-internal add that truncates is allowed):

    global   e_y = 2 * 512 eps (|z4| |W5|^T),  e = |sc| e_y + 4 eps (|sc y| + |sh| + |sc| e_y),  T = max of e over the cloud's rows
    head     T = 2 * 128 eps (|z3| |Wout|^T) + 2 eps (|y| + |bias_out|)                                       per logit

An fp32 value within its own rounding error of a bf16 midpoint may round the other way in the kernel than in fp64, which moves the
outputs downstream of it by about 2^-8 |z w|.  Every head row carries its own part_num logits, so one flip anywhere in the row
shows in all of them, and a faithful torch-fp32 emulation of the contract puts 0.2 - 1.3 % of a head case's outputs over T (645
rows) and 0.15 - 1.6 % of a global case's (129 rows): the classifier's 1 % is not safe here.  So |got - want| <= T must hold for
all but at most CAP = 5 % of a case's outputs -- a cap, not a measurement; tests/test_inference_pointnet_partseg_bf16_cpu.py holds
the emulation at or below 2.5 % on the seeds the GPU tests use -- and each exception must still lie within the worst-case
running bound of tests/bf16_bound.py (its per-layer formulas, ``_bf16_layer`` below) around the UNROUNDED fp64 restatement.

``global_case`` / ``head_case`` are the data generators both the CPU and the GPU tests use; ``emulate_global`` /
``emulate_head`` restate the contract in torch fp32, optionally with one defect, for the CPU tests to show that the yardstick
catches it."""
import torch

import bf16_bound
from bf16_bound import EPS, U, act
import pointnet_bf16_yardstick as _pn
from pointnet_bf16_yardstick import measure, round_bf16  # noqa: F401  (measure: re-exported for the tests)

CAP = 0.05
GLOBAL_SPEC = [128, 512, 2048]
HEAD_SPEC = [832, 256, 256, 128]


def check(got, want, T, ref, worst, label):
    """Print the figures, then assert the yardstick at this module's cap."""
    return _pn.check(got, want, T, ref, worst, label, cap=CAP)


def _layer(g, cin, cout, device, negate_quarter=False):
    W = ((torch.rand(cout, cin, generator=g) * 2 - 1) / cin ** 0.5).to(device)
    sc = 0.5 + torch.rand(cout, generator=g)
    if negate_quarter:
        sc[torch.randperm(cout, generator=g)[:cout // 4]] *= -1.0
    return W, sc.to(device), (0.1 * torch.randn(cout, generator=g)).to(device)


def _rows(g, *shape):
    return torch.randn(*shape, generator=g).abs_().clamp_(max=3.0)


def global_case(seed, B, N, device="cpu"):
    """-> (out3 [B,N,128], T128 [B,128,128], Ws [W4, W5] fp32, scales, shifts): weights and T128 U(-1, 1) / sqrt(K), scale
    U(0.5, 1.5) with a quarter of conv5's negated, shift N(0, 0.1), rows |N(0, 1)| clamped to 3."""
    g = torch.Generator().manual_seed(seed)
    L = [_layer(g, cin, cout, device, negate_quarter=cout == GLOBAL_SPEC[-1]) for cin, cout in zip(GLOBAL_SPEC[:-1], GLOBAL_SPEC[1:])]
    T128 = ((torch.rand(B, 128, 128, generator=g) * 2 - 1) / 128 ** 0.5).to(device)
    return _rows(g, B, N, 128).to(device), T128, [l[0] for l in L], [l[1] for l in L], [l[2] for l in L]


def head_case(seed, B, N, part_num, device="cpu"):
    """-> (F [B,N,832], bias [B,256], Ws [W1, W2, W3] fp32, scales, shifts, Wout [part_num,128], bias_out), as global_case."""
    g = torch.Generator().manual_seed(seed)
    L = [_layer(g, cin, cout, device) for cin, cout in zip(HEAD_SPEC[:-1], HEAD_SPEC[1:])]
    Wout = ((torch.rand(part_num, 128, generator=g) * 2 - 1) / 128 ** 0.5).to(device)
    bout = (0.1 * torch.randn(part_num, generator=g)).to(device)
    bias = (0.1 * torch.randn(B, 256, generator=g)).to(device)
    return _rows(g, B, N, 832).to(device), bias, [l[0] for l in L], [l[1] for l in L], [l[2] for l in L], Wout, bout


def launch_weights(Ws):
    """The weights a bf16 launch is given: every layer rounded to bf16 once (fp32 -> bf16 is one rounding)."""
    return [w.to(torch.bfloat16).contiguous() for w in Ws]


def _bf16_layer(a, e_a, W, sc, sh, slope, add=None):
    """One bf16 layer of tests/bf16_bound.py's running bound: (a*, e_a) of its fp64 input -> (a*, e_a) of its output.  ``sc``
    None: linear + ``sh``.  ``slope`` None: no activation (the identity is 1-Lipschitz too).  ``add``: a per-cloud fp32 bias added
    to the accumulator before the epilogue (one more fp32 rounding)."""
    W = W.double()
    K = W.shape[1]
    e_x = e_a + U * (a.abs() + e_a)
    Wu = (W.abs() * (1 + U)).t()
    y = a @ W.t()
    e_y = e_x @ Wu + U * (a.abs() @ W.abs().t()) + K * EPS * ((a.abs() + e_x) @ Wu)
    if add is not None:
        e_y = e_y + EPS * (y.abs() + add.abs() + e_y)
        y = y + add
    sc = torch.ones_like(sh, dtype=torch.float64) if sc is None else sc.double()
    sh = sh.double()
    e = sc.abs() * e_y + 4 * EPS * ((sc * y).abs() + sh.abs() + sc.abs() * e_y)
    z = sc * y + sh
    return (z if slope is None else act(z, slope)), e


# ------------------------------------------------------------------------------------------------------------- global
def restate_global(out3, T128, Wl, scales, shifts, slope):
    """One cloud: out3 [n,128], T128 [128,128], Wl the launch's constants -> (z4 unrounded, z4 rounded, y5, out5), fp64."""
    W4, W5 = [w.double() for w in Wl]
    sc, sh = [s.double() for s in scales], [s.double() for s in shifts]
    x2 = round_bf16(out3.double() @ T128.double())
    z4 = act(sc[0] * (x2 @ W4.t()) + sh[0], slope)
    z4r = round_bf16(z4)
    y5 = z4r @ W5.t()
    return z4, z4r, y5, sc[1] * y5 + sh[1]


def global_want_and_bounds(out3, n, T128, Wl, scales, shifts, slope):
    """out3 [B,N,128] (pad rows may hold anything), n per-cloud counts -> (want [B,2048], T, the unrounded fp64 restatement, its
    worst-case bound; then per cloud (out4 fp64 [n_b,512], its worst-case bound))."""
    want, T, ref, worst, out4 = [], [], [], [], []
    sc5, sh5, W5 = scales[1].double(), shifts[1].double(), Wl[1].double()
    for b in range(out3.shape[0]):
        rows = out3[b, :n[b]].double()
        _, z4r, y5, z5 = restate_global(rows, T128[b], Wl, scales, shifts, slope)
        e_y = 2 * W5.shape[1] * EPS * (z4r.abs() @ W5.abs().t())
        e = sc5.abs() * e_y + 4 * EPS * ((sc5 * y5).abs() + sh5.abs() + sc5.abs() * e_y)
        want.append(z5.max(dim=0)[0])
        T.append(e.max(dim=0)[0])
        # unrounded: x2 is an fp32 accumulation of 128 products (the 2 as above), then two bf16 layers
        a = rows @ T128[b].double()
        e_a = 2 * 128 * EPS * (rows.abs() @ T128[b].double().abs())
        a4, e4 = _bf16_layer(a, e_a, Wl[0], scales[0], shifts[0], slope)
        a5, e5 = _bf16_layer(a4, e4, Wl[1], scales[1], shifts[1], None)
        ref.append(a5.max(dim=0)[0])
        worst.append(e5.max(dim=0)[0])
        out4.append((a4, e4))
    return torch.stack(want), torch.stack(T), torch.stack(ref), torch.stack(worst), out4


def _trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _rnd(defect):
    return _trunc_bf16 if defect == "trunc" else (lambda t: t.to(torch.bfloat16).float())


def _busiest(a):
    return int(a.abs().reshape(-1, a.shape[-1]).mean(dim=0).argmax())       # a dead input channel shows nowhere


def emulate_global(out3, n, T128, Ws, scales, shifts, slope, defect=None):
    """The global launch's contract in torch fp32 (accumulation order aside) -> out_max [B,2048].  ``defect``: "trunc"
    (activations truncated to bf16), "drop_k" (conv4 loses one k, its busiest input channel), "fp32_w" (W5 not rounded),
    "round_out" (out5 rounded to bf16)."""
    rnd = _rnd(defect)
    out = []
    for b in range(out3.shape[0]):
        x2 = rnd(out3[b, :n[b]].float() @ T128[b].float())
        W4 = Ws[0].float().to(torch.bfloat16).float()
        if defect == "drop_k":
            W4 = W4.clone()
            W4[:, _busiest(x2)] = 0.0
        z4 = act(scales[0].float() * (x2 @ W4.t()) + shifts[0].float(), slope)
        W5 = Ws[1].float() if defect == "fp32_w" else Ws[1].float().to(torch.bfloat16).float()
        z5 = scales[1].float() * (rnd(z4) @ W5.t()) + shifts[1].float()
        if defect == "round_out":
            z5 = z5.to(torch.bfloat16).float()
        out.append(z5.max(dim=0)[0])
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------------------- head
def restate_head(F, bias, Wl, scales, shifts, Wout_l, bout, slope):
    """F [B,N,832], bias [B,256], Wl / Wout_l the launch's constants -> (z3 rounded [B,N,128], y = z3 Wout^T, logits), fp64."""
    sc, sh = [s.double() for s in scales], [s.double() for s in shifts]
    z = round_bf16(F.double())
    for l, W in enumerate(Wl):
        y = z @ W.double().t()
        if l == 0:
            y = y + bias.double()[:, None, :]
        z = round_bf16(act(sc[l] * y + sh[l], slope))
    y = z @ Wout_l.double().t()
    return z, y, y + bout.double()


def head_want_and_bounds(F, bias, Wl, scales, shifts, Wout_l, bout, slope):
    """-> (want [B,N,part_num], T, the unrounded fp64 restatement, its worst-case bound), fp64; every row of F is taken as valid."""
    z3, y, want = restate_head(F, bias, Wl, scales, shifts, Wout_l, bout, slope)
    Wo = Wout_l.double()
    T = 2 * Wo.shape[1] * EPS * (z3.abs() @ Wo.abs().t()) + 2 * EPS * (y.abs() + bout.double().abs())
    a, e = F.double(), torch.zeros_like(F, dtype=torch.float64)
    for l, W in enumerate(Wl):
        a, e = _bf16_layer(a, e, W, scales[l], shifts[l], slope, add=bias.double()[:, None, :] if l == 0 else None)
    ref, worst = _bf16_layer(a, e, Wo, None, bout, None)
    return want, T, ref, worst


def emulate_head(F, bias, Ws, scales, shifts, Wout, bout, slope, defect=None, W1_bf16=None):
    """The head launch's contract in torch fp32 -> logits [B,N,part_num].  ``defect``: "trunc", "drop_k" (layer 3 loses one k, its
    busiest input channel), "fp32_w" (Wout not rounded), "round_out" (the logits rounded to bf16).  ``W1_bf16``: the first
    weight as the launch is given it, when it is not ``Ws[0]`` rounded from fp32."""
    rnd = _rnd(defect)
    z = rnd(F.float())
    for l, W in enumerate(Ws):
        Wb = W.float().to(torch.bfloat16).float() if (l or W1_bf16 is None) else W1_bf16.float()
        if defect == "drop_k" and l == 2:
            Wb = Wb.clone()
            Wb[:, _busiest(z)] = 0.0
        y = z @ Wb.t()
        if l == 0:
            y = y + bias.float()[:, None, :]
        z = rnd(act(scales[l].float() * y + shifts[l].float(), slope))
    Wo = Wout.float() if defect == "fp32_w" else Wout.float().to(torch.bfloat16).float()
    out = z @ Wo.t() + bout.float()
    return out.to(torch.bfloat16).float() if defect == "round_out" else out


def double_rounding_wrow(seed, device="cpu"):
    """A folded first weight [256, 832] in fp64 of which EVERY entry is a double-rounding case: a bf16 value of even mantissa plus
    half a bf16 ulp plus 2^-30 of that -- one rounding gives the bf16 value above, fp64 -> fp32 lands on the tie and fp32 -> bf16
    then falls back to the even value below.  -> (Wrow fp64, rounded once (bf16), rounded through fp32 (bf16))"""
    g = torch.Generator().manual_seed(seed)
    w = ((torch.rand(256, 832, generator=g, dtype=torch.float64) * 2 - 1) / 832 ** 0.5)
    w = torch.where(w.abs() < 1e-3, torch.full_like(w, 1e-3), w)
    m, e = torch.frexp(w)
    even = torch.ldexp(torch.trunc(m * 128.0) * 2.0, e - 8)            # 8 significant bits, the last one 0
    half = torch.ldexp(torch.sign(m), e - 9)                            # half an ulp, away from zero
    W = (even + half + half * 2.0 ** -30).to(device)
    once = round_bf16(W).to(torch.bfloat16)
    twice = W.float().to(torch.bfloat16)
    assert bool((once.double() != twice.double()).all())
    return W, once, twice
