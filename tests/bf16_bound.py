"""The yardstick of the bf16 frozen-inference tests (``frozen(net, precision="bf16")``, pcl_sa_level_infer_bf16_f32).  TEST
INFRASTRUCTURE, no test of its own; runs on any device.

bf16 rounding cannot be held to the project's 1e-5 rule and a measured tolerance would be circular, so the tests use a DERIVED
one: a running forward error bound, computed in fp64 beside the fp64 restatement of one set-abstraction level, for a kernel that
keeps the numerics contract in csrc/infer.hip.  u = 2^-8 is the unit roundoff of bf16 (round to nearest even), eps = 2^-24 that
of fp32.  With a* the fp64 value, |.| elementwise and every product below a matrix product over the layer's fan-in:

    layer 1 (fp32 fmaf chain, epilogue)    e_a = 8 eps (|sc| (|x| |W|^T) + |sh|)
    a value rounded to bf16                e_x = e_a + u (|a*| + e_a)
    a bf16 layer of fan-in K               e_y = e_x (|W| (1 + u))^T + u (|a*| |W|^T) + K eps ((|a*| + e_x) (|W| (1 + u))^T)
                                           (the input's error through the rounded weights; the weights' own rounding; the fp32
                                           accumulation of K exact bf16 x bf16 products)
    its epilogue act(sc y + sh) in fp32    e_a = |sc| e_y + 4 eps (|sc y*| + |sh| + |sc| e_y)      (act is 1-Lipschitz, slope <= 1)
    the group max                          max of e_a over the group's rows

and the assertion is elementwise: |kernel - fp64| <= bound.  The restatement takes the constants the kernel is given (fp32
weights, scale and shift, read as fp64): the contract is about the launch, not about how its caller made the constants.

``emulate`` restates the contract in torch (fp32 accumulation order aside), optionally dropping the last k of the last layer:
tests/test_inference_bf16_cpu.py uses it to show that the bound is loose against rounding noise (the faithful emulation sits at
a few hundredths of it) and tight against a mapping defect (8 dropped k of one layer exceed it).
"""
import torch

U = 2.0 ** -8
EPS = 2.0 ** -24


def act(x, slope):
    return torch.where(x > 0, x, x * slope)


def rows_ref_and_bound(x, Ws, scales, shifts, slope):
    """x [..., Cin] fp64 (the first layer's exact input rows), Ws[l] [C_l, C_{l-1}], scales / shifts [C_l] (any float dtype)
    -> (a* [..., C_L] fp64, bound on |kernel row - a*| before the max)."""
    assert slope <= 1.0
    Ws = [w.double() for w in Ws]
    scales, shifts = [s.double() for s in scales], [s.double() for s in shifts]
    W, sc, sh = Ws[0], scales[0], shifts[0]
    a = act(sc * (x @ W.t()) + sh, slope)
    e_a = 8 * EPS * (sc.abs() * (x.abs() @ W.abs().t()) + sh.abs())
    for W, sc, sh in zip(Ws[1:], scales[1:], shifts[1:]):
        e_x = e_a + U * (a.abs() + e_a)
        K = W.shape[1]
        Wu = (W.abs() * (1 + U)).t()
        y = a @ W.t()
        e_y = e_x @ Wu + U * (a.abs() @ W.abs().t()) + K * EPS * ((a.abs() + e_x) @ Wu)
        e_a = sc.abs() * e_y + 4 * EPS * ((sc * y).abs() + sh.abs() + sc.abs() * e_y)
        a = act(sc * y + sh, slope)
    return a, e_a


def grouped_rows(xyz, new_xyz, feat, idx, cnt, use_xyz=True):
    """The rows of a ball-query level in fp64: x [B, m, ns, 3 use_xyz + C] and the mask of each group's max(cnt, 1) first slots."""
    B, m, ns = idx.shape
    bidx = torch.arange(B, device=idx.device).view(B, 1, 1)
    il = idx.long()
    parts = []
    if use_xyz:
        parts.append(xyz.double()[bidx, il] - new_xyz.double().unsqueeze(2))
    if feat is not None:
        parts.append(feat.double()[bidx, il])
    valid = torch.arange(ns, device=idx.device).view(1, 1, ns) < cnt.clamp(min=1).unsqueeze(-1)
    return torch.cat(parts, dim=-1), valid


def level_ref_and_bound(xyz, new_xyz, feat, idx, cnt, Ws, scales, shifts, slope, use_xyz=True):
    """-> (fp64 restatement [B, m, C_L] of the level, elementwise bound on |bf16 kernel - restatement|)."""
    x, valid = grouped_rows(xyz, new_xyz, feat, idx, cnt, use_xyz)
    a, e = rows_ref_and_bound(x, Ws, scales, shifts, slope)
    mask = ~valid.unsqueeze(-1)
    return a.masked_fill(mask, float("-inf")).max(dim=2)[0], e.masked_fill(mask, 0.0).max(dim=2)[0]


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 counts as 0)."""
    err = (got.double() - ref).abs()
    return float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())


def emulate(x, Ws, scales, shifts, slope, drop_last_k=0):
    """The numerics contract in torch: x [..., Cin] fp32 -> rows [..., C_L] fp32.  Layer 1 in fp32, rounded to bf16; every later
    layer bf16 x bf16 (exact in fp32) summed in fp32, epilogue in fp32, rounded to bf16 except after the last.  ``drop_last_k``:
    the last layer loses its last k inputs -- a mapping defect for the yardstick to catch."""
    x = x.float()
    a = act(scales[0].float() * (x @ Ws[0].float().t()) + shifts[0].float(), slope)
    L = len(Ws)
    for l in range(1, L):
        Wb = Ws[l].float().to(torch.bfloat16).float()
        if l == L - 1 and drop_last_k:
            Wb = Wb.clone()
            Wb[:, -drop_last_k:] = 0.0
        a = act(scales[l].float() * (a.to(torch.bfloat16).float() @ Wb.t()) + shifts[l].float(), slope)
    return a
