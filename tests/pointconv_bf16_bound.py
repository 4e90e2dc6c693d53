"""The yardstick of the bf16 frozen PointConv tests (``FrozenPointConv(net, precision="bf16")``,
pcl_pointconv_level_infer_bf16_f32).  TEST INFRASTRUCTURE, no test of its own; runs on any device.

As in tests/bf16_bound.py the tolerance is DERIVED, not measured: a running forward error bound, computed in fp64 beside the fp64
restatement of one k-NN level up to the contraction (tests/pointconv_infer_ref.py), for a kernel that keeps the numeric contract
in include/pcl_hip.h.  u = 2^-8 (bf16), eps = 2^-24 (fp32); a* is the fp64 value, |.| elementwise.

The feature MLP.  The rows are x = (d | points[idx]) with d = xyz[idx] - new_xyz in fp64; ``bf16_bound.rows_ref_and_bound`` gives
(z*, e_z) per row and channel: its recurrence is fp32 layer 1 (8 eps of the absolute sum covers the rounding of d, the fmaf chain
and the epilogue), the rounding of z1 to bf16, two bf16 layers with fp32 accumulation and fp32 epilogues, the rounding of z2, and
an unrounded last epilogue -- the contract of the launch.

The small nets (fp32 only).  Input error: e_d = eps |d*| (one __fsub_rn), 0 for the density (an fp32 input).  Per layer of fan-in K,
y = W x as an fmaf chain and relu(scale * y + shift) in two roundings (relu is 1-Lipschitz):

    e_y = |W| e_x + K eps |W| (|x*| + e_x)                         (the input's error; K roundings of the chain)
    e_a = |sc| e_y + 4 eps (|sc y*| + |sh| + |sc| e_y)             (as the epilogue of bf16_bound)

which gives (w*, e_w) [.., 16] and (rho*, e_rho) [.., 1].  Their product is one more rounding:

    e_rw = |rho*| e_w + |w*| e_rho + e_w e_rho + eps |rho* w*|

The contraction out[c, m] = sum_s z[s, c] rw[s, m] in fp32 (ns products, ns roundings of the accumulator), elementwise:

    e_out[c, m] = sum_s (e_z (|rw*| + e_rw) + |z*| e_rw)  +  ns eps sum_s (|z*| + e_z) (|rw*| + e_rw)

and the assertion is |kernel - fp64| <= e_out for every output.  The restatement takes the constants the launch is given (the fp32
weights, scale and shift of the feature MLP and the packed small nets, read as fp64): the contract is about the launch, not about
how its caller made the constants.  Second-order terms in eps are dropped except where a factor is not small (e_z is of order u).

``emulate`` restates the contract in torch (bf16 roundings, fp32 elsewhere, accumulation order aside), optionally dropping the
last k of layer 3: tests/test_inference_pointconv_bf16_cpu.py uses it to show that the bound holds for a faithful kernel and
is exceeded by a mapping defect."""
import torch

import bf16_bound as bb

EPS = bb.EPS
# (weight offset, out, in, scale offset, shift offset) per layer of the packed buffer (include/pcl_hip.h)
WEIGHTNET = [(0, 8, 3, 24, 32), (40, 8, 8, 104, 112), (120, 16, 8, 248, 264)]
DENSITYNET = [(280, 8, 1, 288, 296), (304, 8, 8, 368, 376), (384, 1, 8, 392, 393)]


def rows(xyz, new_xyz, points, idx, dtype=torch.float64):
    """-> (d [B,S,ns,3], x [B,S,ns,3 + D] = d | points[idx], density gather index) in ``dtype``."""
    B = idx.shape[0]
    bidx = torch.arange(B, device=idx.device).view(B, 1, 1)
    il = idx.long()
    d = xyz.to(dtype)[bidx, il] - new_xyz.to(dtype).unsqueeze(2)
    x = d if points is None else torch.cat([d, points.to(dtype)[bidx, il]], dim=-1)
    return d, x, (bidx, il)


def small_net_ref_and_bound(packed, layers, x, e_x):
    """One packed small net in fp64 with its running fp32 bound: x [.., K0] fp64, e_x the bound on the kernel's input -> (a*, e_a)."""
    p = packed.double().to(x.device)
    a, e_a = x, e_x
    for w0, cout, cin, s0, t0 in layers:
        W, sc, sh = p[w0:w0 + cout * cin].view(cout, cin), p[s0:s0 + cout], p[t0:t0 + cout]
        y = a @ W.t()
        e_y = e_a @ W.abs().t() + cin * EPS * ((a.abs() + e_a) @ W.abs().t())
        e_a = sc.abs() * e_y + 4 * EPS * ((sc * y).abs() + sh.abs() + sc.abs() * e_y)
        a = (sc * y + sh).clamp(min=0)
    return a, e_a


def level_ref_and_bound(feat, packed, xyz, new_xyz, points, idx, density, slope=0.0):
    """feat: [(W, scale, shift)] as handed to the launch (any float dtype), packed: the small nets' buffer
    -> (fp64 restatement [B, S, C3 * 16], elementwise bound on |bf16 kernel - restatement|)."""
    B, S, ns = idx.shape
    d, x, (bidx, il) = rows(xyz, new_xyz, points, idx)
    z, e_z = bb.rows_ref_and_bound(x, [l[0] for l in feat], [l[1] for l in feat], [l[2] for l in feat], slope)
    w, e_w = small_net_ref_and_bound(packed, WEIGHTNET, d, EPS * d.abs())
    dens = density.double()[bidx, il].unsqueeze(-1)
    rho, e_rho = small_net_ref_and_bound(packed, DENSITYNET, dens, torch.zeros_like(dens))
    rw = rho * w
    e_rw = rho.abs() * e_w + w.abs() * e_rho + e_w * e_rho + EPS * rw.abs()
    zt, ezt = z.abs().transpose(2, 3), e_z.transpose(2, 3)
    rwu = rw.abs() + e_rw
    ref = torch.matmul(z.transpose(2, 3), rw)
    bound = torch.matmul(ezt, rwu) + torch.matmul(zt, e_rw) + ns * EPS * torch.matmul(zt + ezt, rwu)
    return ref.reshape(B, S, -1), bound.reshape(B, S, -1)


def worst_ratio(got, ref, bound):
    return bb.worst_ratio(got, ref, bound)


def activations(feat, x, slope=0.0):
    """[z1, z2, z3] of the feature MLP on rows x, in x's dtype (fp64: the restatement's own activations)."""
    out = []
    for W, sc, sh in feat:
        x = bb.act(sc.to(x.dtype) * (x @ W.to(x.dtype).t()) + sh.to(x.dtype), slope)
        out.append(x)
    return out


def emulate(feat, packed, xyz, new_xyz, points, idx, density, slope=0.0, drop_last_k=0):
    """The numeric contract in torch -> [B, S, C3 * 16] fp32: d, layer 1 and the small nets in fp32; z1 and z2 rounded to bf16,
    layers 2 and 3 bf16 x bf16 summed in fp32 with fp32 epilogues (``bf16_bound.emulate``); z3 unrounded; rw and the contraction in
    fp32.  ``drop_last_k``: layer 3 loses its last k inputs -- a mapping defect for the yardstick to catch."""
    B, S, ns = idx.shape
    f32 = torch.float32
    d, x, (bidx, il) = rows(xyz.float(), new_xyz.float(), None if points is None else points.float(), idx, f32)
    z = bb.emulate(x, [l[0] for l in feat], [l[1] for l in feat], [l[2] for l in feat], slope, drop_last_k)
    p = packed.float().to(d.device)

    def net(a, layers):
        for w0, cout, cin, s0, t0 in layers:
            a = (p[s0:s0 + cout] * (a @ p[w0:w0 + cout * cin].view(cout, cin).t()) + p[t0:t0 + cout]).clamp(min=0)
        return a

    rw = net(density.float()[bidx, il].unsqueeze(-1), DENSITYNET) * net(d, WEIGHTNET)
    return torch.matmul(z.transpose(2, 3), rw).reshape(B, S, -1)
