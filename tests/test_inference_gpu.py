"""Frozen inference (pointcloudlib_amd/inference.py, csrc/infer.hip) on the GPU: the fused set-abstraction kernel through the C ABI,
whole SSG / MSG networks against an fp64 evaluation-mode restatement, the memory a forward needs, and the contract of ``frozen``.

Yardstick: the fused path may be no further from the fp64 restatement than the existing ``net.eval()`` path on the same inputs,
x 1.25, plus 1e-6."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _P(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _act(x, slope):
    return torch.where(x > 0, x, x * slope)


def _perturb(net, seed):
    """Running statistics, gamma and beta of every BatchNorm away from their initial values (some gamma < 0)."""
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in net.modules():
            pairs = []
            if isinstance(mod, PointwiseMLP) and mod.bn:
                pairs = [(mod.gammas[l], mod.betas[l], getattr(mod, f"running_mean_{l}"), getattr(mod, f"running_var_{l}")) for l in range(mod.n_layers)]
            elif isinstance(mod, torch.nn.BatchNorm1d):
                pairs = [(mod.weight, mod.bias, mod.running_mean, mod.running_var)]
            for gam, bet, rm, rv in pairs:
                c = gam.numel()
                sign = torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
                gam.copy_(sign * (0.5 + torch.rand(c, generator=g)))
                bet.copy_(0.1 * torch.randn(c, generator=g))
                rm.copy_(0.1 * torch.randn(c, generator=g))
                rv.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return net


def _consts64(mlp, l):
    W = mlp.weights[l].detach().double()
    bias = None if mlp.biases is None else mlp.biases[l].detach().double()
    if mlp.bn:
        rm, rv = getattr(mlp, f"running_mean_{l}").double(), getattr(mlp, f"running_var_{l}").double()
        scale = mlp.gammas[l].detach().double() / torch.sqrt(rv + mlp.eps)
        shift = mlp.betas[l].detach().double() - scale * rm
        if bias is not None:
            shift = shift + scale * bias
    else:
        scale = torch.ones_like(W[:, 0])
        shift = torch.zeros_like(W[:, 0]) if bias is None else bias
    return W, scale, shift


def _ref_grouped(mlp, xyz, new_xyz, feat, idx, cnt, use_xyz=True):
    """fp64 eval-mode restatement of one ball-query scale: conv/bn/act x L over the group's max(cnt, 1) first slots, max."""
    xyz, new_xyz = xyz.double(), new_xyz.double()
    B, m, ns = idx.shape
    bidx = torch.arange(B, device=idx.device).view(B, 1, 1)
    il = idx.long()
    parts = []
    if use_xyz:
        parts.append(xyz[bidx, il] - new_xyz.unsqueeze(2))
    if feat is not None:
        parts.append(feat.double()[bidx, il])
    x = torch.cat(parts, dim=-1)
    for l in range(mlp.n_layers):
        W, scale, shift = _consts64(mlp, l)
        x = _act(scale * (x @ W.t()) + shift, mlp.slope)
    valid = torch.arange(ns, device=idx.device).view(1, 1, ns) < cnt.clamp(min=1).unsqueeze(-1)
    return x.masked_fill(~valid.unsqueeze(-1), float("-inf")).max(dim=2)[0]


def _ref_group_all(mlp, xyz, feat):
    x = torch.cat([xyz.double(), feat.double()], dim=-1)
    for l in range(mlp.n_layers):
        W, scale, shift = _consts64(mlp, l)
        x = _act(scale * (x @ W.t()) + shift, mlp.slope)
    return x.max(dim=1, keepdim=True)[0]


def _ref_head(seq, x):
    x = x.double()
    for mod in seq:
        if isinstance(mod, torch.nn.Linear):
            x = x @ mod.weight.double().t() + (0 if mod.bias is None else mod.bias.double())
        elif isinstance(mod, torch.nn.BatchNorm1d):
            x = (x - mod.running_mean.double()) / torch.sqrt(mod.running_var.double() + mod.eps) * mod.weight.double() + mod.bias.double()
        elif isinstance(mod, torch.nn.ReLU):
            x = x.clamp(min=0)
    return x


def _ref_net(net, xyz, feat, sampling):
    """fp64 evaluation of the whole classifier on the index lists of ``sampling``: (per-level features, logits)."""
    feats = []
    for module, (new_xyz, idxs) in zip(net.pointnet_modules, sampling["levels"]):
        if new_xyz is None:
            f = _ref_group_all(module.mlps[0], xyz, feat)
        else:
            f = torch.cat([_ref_grouped(mlp, xyz, new_xyz, feat, ic[0], ic[1], grouper.use_xyz)
                           for mlp, grouper, ic in zip(module.mlps, module.groupers, idxs)], dim=-1)
            xyz = new_xyz
        feats.append(f)
        feat = f
    return feats, _ref_head(net.fc_layer, feat.squeeze(1))


def _eval_levels(net, xyz, feat, sampling):
    """The existing evaluation path (net.eval() + no_grad) on a copy, level by level."""
    ev = copy.deepcopy(net).eval()
    feats = []
    with torch.no_grad():
        for i, module in enumerate(ev.pointnet_modules):
            xyz, feat = module(xyz, feat, sampling["levels"][i])
            feats.append(feat)
        from pointcloudlib_amd.misc.head import fc_head
        return feats, fc_head(ev.fc_layer, feat.squeeze(1))


def _err(a, ref):
    return (a.double() - ref).abs().max().item()


# ----------------------------------------------------------------------------------------------------------- the kernel
# (ns, [C_in_features, C1, C2, C3], inline features) -- the rows of the shape table: SSG SA1/SA2, MSG SA1 x3, MSG SA2 x3
_SHAPES = [(64, [3, 64, 64, 128], True), (64, [128, 128, 128, 256], False),
           (16, [3, 32, 32, 64], True), (32, [3, 64, 64, 128], True), (128, [3, 64, 96, 128], True),
           (32, [320, 64, 64, 128], False), (64, [320, 128, 128, 256], False), (128, [320, 128, 128, 256], False)]


def _kernel_case(dev, ns, spec, slope, seed):
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.misc.ops import group_offsets
    torch.manual_seed(seed)
    B, N, m = 3, 700, 41                         # G = 123: not a multiple of any group tile
    C = spec[0]
    mlp = PointwiseMLP([3 + C] + spec[1:], bias=False, bn=True, slope=slope).to(dev)
    _perturb(mlp, seed)
    mlp.eval()
    xyz = torch.rand(B, N, 3, device=dev)
    new_xyz = torch.rand(B, m, 3, device=dev)
    feat = torch.randn(B, N, C, device=dev)
    # distinct neighbours per group (what ball query produces), padding repeats the first hit
    idx = torch.stack([torch.stack([torch.randperm(N, device=dev)[:ns] for _ in range(m)]) for _ in range(B)]).int()
    cnt = torch.randint(0, ns + 1, (B, m), device=dev, dtype=torch.int32)
    cnt.view(-1)[:3] = torch.tensor([0, 1, ns], dtype=torch.int32)
    first = idx[:, :, :1].expand(-1, -1, ns)
    slot = torch.arange(ns, device=dev).view(1, 1, ns)
    idx = torch.where(slot < cnt.clamp(min=1).unsqueeze(-1), idx, first).contiguous()
    return mlp, xyz, new_xyz, feat, idx, cnt, group_offsets(cnt)


def _fused_call(mlp, xyz, new_xyz, feat, idx, cnt, inline):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.inference import _eval_consts
    B, N, _ = xyz.shape
    m, ns = idx.shape[1], idx.shape[2]
    C = feat.shape[-1]
    W0 = mlp.weights[0].detach().contiguous()
    C1 = W0.shape[0]
    feat2 = feat.reshape(B * N, C).contiguous()
    Uf = None
    if not inline:
        Uf = torch.empty(B * N, C1, device=xyz.device)
        Wf = W0[:, 3:].contiguous()
        _lib.call("pcl_linear_fwd_rows_f32", _P(feat2), _P(Wf), None, None, None, 0.0, B * N, C, C1, _P(Uf), None, None, None, _stream())
    L = mlp.n_layers
    Ws = [None] + [mlp.weights[l].detach().contiguous() for l in range(1, L)]
    consts = [_eval_consts(mlp, l) for l in range(L)]
    widths = (ctypes.c_int32 * L)(*[w.shape[0] for w in mlp.weights])
    c_W = (ctypes.c_void_p * L)(*[_P(w) for w in Ws])
    c_sc = (ctypes.c_void_p * L)(*[_P(c[0]) for c in consts])
    c_sh = (ctypes.c_void_p * L)(*[_P(c[1]) for c in consts])
    CL = mlp.spec[-1]
    ldo, col0 = CL + 8, 5                       # a column slice of a wider output, as the multi-scale levels write it
    out = torch.full((B * m, ldo), 7.0, device=xyz.device)
    _lib.call("pcl_sa_level_infer_f32", _P(xyz), _P(new_xyz), _P(Uf), _P(W0), _P(feat2) if inline else None,
              _P(W0[:, 3:]) if inline else None, C if inline else 0, W0.shape[1], _P(idx), _P(cnt), B, N, m, ns, L, widths, c_W,
              c_sc, c_sh, float(mlp.slope), _P(out), ldo, col0, _stream())
    assert bool((out[:, :col0] == 7.0).all()) and bool((out[:, col0 + CL:] == 7.0).all()), "wrote outside its column slice"
    return out[:, col0:col0 + CL].reshape(B, m, CL)


@pytest.mark.parametrize("ns,spec,inline", _SHAPES)
@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_sa_level_kernel_against_fp64(dev, ns, spec, inline, slope):
    mlp, xyz, new_xyz, feat, idx, cnt, goff = _kernel_case(dev, ns, spec, slope, seed=ns + spec[1] + spec[2] + int(10 * slope))
    with torch.no_grad():
        got = _fused_call(mlp, xyz, new_xyz, feat, idx, cnt, inline)
        again = _fused_call(mlp, xyz, new_xyz, feat, idx, cnt, inline)
        want_eval = mlp.forward_grouped(xyz, new_xyz, feat, idx, cnt, goff, True)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two calls differ"
    ref = _ref_grouped(mlp, xyz, new_xyz, feat, idx, cnt)
    e_fused, e_eval = _err(got, ref), _err(want_eval, ref)
    assert e_fused <= 1.25 * e_eval + 1e-6, f"fused {e_fused:.3e} vs eval path {e_eval:.3e} from fp64"


# ----------------------------------------------------------------------------------------------------------- networks
def _net(kind, dev, seed=0):
    from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls, PointNetMSG
    torch.manual_seed(seed)
    net = (PointNet2_cls if kind == "ssg" else PointNetMSG)().to(dev)
    return _perturb(net, seed + 1)


def _clouds(dev, B, N=1024, seed=0):
    from pointcloudlib_amd import synth
    return (torch.from_numpy(synth.gauss_ball(B, N, seed)).to(dev), torch.from_numpy(synth.unit_normals(B, N, seed + 1)).to(dev))


@pytest.mark.parametrize("kind", ["ssg", "msg"])
def test_frozen_network_against_fp64(dev, kind):
    from pointcloudlib_amd.inference import frozen
    net = _net(kind, dev)
    xyz, nrm = _clouds(dev, 32)
    samp = net.precompute_sampling(xyz)
    fnet = frozen(net)
    feats, logits = fnet.run(xyz, nrm, sampling=samp)
    ev_feats, ev_logits = _eval_levels(net, xyz, nrm, samp)
    ref_feats, ref_logits = _ref_net(net, xyz, nrm, samp)
    torch.cuda.synchronize()
    for i, (f, e, r) in enumerate(zip(feats, ev_feats, ref_feats)):
        assert f.shape == e.shape
        ef, ee = _err(f, r), _err(e, r)
        assert ef <= 1.25 * ee + 1e-6, f"level {i}: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    ef, ee = _err(logits, ref_logits), _err(ev_logits, ref_logits)
    assert ef <= 1.25 * ee + 1e-6, f"logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    bound = 1.25 * ee + 1e-6
    top2 = ref_logits.topk(2, dim=1)[0]
    sure = (top2[:, 0] - top2[:, 1]) > 2 * bound
    assert bool((logits.argmax(1) == ref_logits.argmax(1))[sure].all())


def test_frozen_forward_memory(dev):
    from pointcloudlib_amd.inference import frozen
    net = _net("ssg", dev)
    B = 32
    xyz, nrm = _clouds(dev, B)
    samp = net.precompute_sampling(xyz)
    fnet = frozen(net)
    fnet(xyz, nrm, sampling=samp)                 # warm-up: one-time allocations (constants, plans)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fnet(xyz, nrm, sampling=samp)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    level_out = B * 512 * 128 + B * 128 * 256 + B * 1024
    uf = B * 512 * 128                            # SA2's per-point table (SA1's normals fold inline)
    group_all = B * 128 * (3 + 256 + 256 + 512 + 1024)
    bound = 2 * 4 * (level_out + uf + group_all)
    assert out.shape == (B, 40)
    assert peak <= bound, f"frozen forward peak +{peak / 2**20:.1f} MiB > bound {bound / 2**20:.1f} MiB"


def test_frozen_contract(dev):
    from pointcloudlib_amd.inference import frozen
    net = _net("ssg", dev).train()
    xyz, nrm = _clouds(dev, 8, seed=3)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = frozen(net)
    out_inline = fnet(xyz, nrm)
    out_handle = fnet(xyz, nrm, sampling=net.precompute_sampling(xyz))
    torch.cuda.synchronize()
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(out_inline, out_handle), "a precomputed sampling handle changes the output"
    # refresh() re-reads the running statistics
    with torch.no_grad():
        net.pointnet_modules[1].mlps[0].running_var_1.mul_(3.0)
    stale = fnet(xyz, nrm)
    fresh = fnet.refresh()(xyz, nrm)
    torch.cuda.synchronize()
    assert torch.equal(stale, out_inline)
    assert not torch.equal(fresh, out_inline)
    assert torch.equal(fresh, frozen(net)(xyz, nrm))


def test_frozen_falls_back_for_other_widths(dev):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.inference import frozen
    net = _net("ssg", dev)
    sa2, sa3 = net.pointnet_modules[1], net.pointnet_modules[2]
    assert not _lib.lib().pcl_sa_level_infer_supported(64, 3, 128, 128, 288, 0)
    torch.manual_seed(5)
    sa2.mlps[0] = sa2.build_mlps([128, 128, 128, 288]).to(dev)
    sa3.mlps[0] = sa3.build_mlps([288, 256, 512, 1024]).to(dev)
    _perturb(net, 9)
    xyz, nrm = _clouds(dev, 16, seed=4)
    samp = net.precompute_sampling(xyz)
    fnet = frozen(net)
    assert [k for k, _ in fnet.levels[1]] == ["module"]
    feats, logits = fnet.run(xyz, nrm, sampling=samp)
    ev_feats, ev_logits = _eval_levels(net, xyz, nrm, samp)
    ref_feats, ref_logits = _ref_net(net, xyz, nrm, samp)
    torch.cuda.synchronize()
    assert feats[1].shape == ev_feats[1].shape == (16, 128, 288)
    ef, ee = _err(logits, ref_logits), _err(ev_logits, ref_logits)
    assert ef <= 1.25 * ee + 1e-6, f"logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
