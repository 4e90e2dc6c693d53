"""Frozen part-seg inference (pointcloudlib_amd/inference.py, csrc/infer_fp.hip) on the GPU: the fused feature-propagation kernel
through the C ABI, whole SSG / MSG part-seg networks against an fp64 evaluation-mode restatement, the memory a forward needs, the
contract of ``frozen``, the fallback, and ``train_partseg.py --fast_eval``.

Yardstick: the fused path may be no further from the fp64 restatement than ``net.eval()`` with plain fp32 accumulation
(``set_accumulation(copy, 0)``) on the same inputs, x 1.25, plus 1e-6."""
import copy
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
            if isinstance(mod, PointwiseMLP) and mod.bn:
                for l in range(mod.n_layers):
                    gam, bet = mod.gammas[l], mod.betas[l]
                    rm, rv = getattr(mod, f"running_mean_{l}"), getattr(mod, f"running_var_{l}")
                    c = gam.numel()
                    sign = torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
                    gam.copy_(sign * (0.5 + torch.rand(c, generator=g)))
                    bet.copy_(0.1 * torch.randn(c, generator=g))
                    rm.copy_(0.1 * torch.randn(c, generator=g))
                    rv.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return net


def _mlp64(mlp, x):
    """fp64 eval-mode restatement of a PointwiseMLP on rows x [..., C0]."""
    x = x.double()
    for l in range(mlp.n_layers):
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
        x = scale * (x @ W.t()) + shift
        if l < mlp.n_layers - 1 or mlp.last_act:
            x = _act(x, mlp.slope)
    return x


def _fp64_fp(fp, xyz1, xyz2, points1, points2):
    """fp64 restatement of a PointNetFeaturePropagation level on the 3-NN lists the library produces."""
    from pointcloudlib_amd.misc.ops import three_nn
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    p2 = points2.double()
    if S == 1:
        interp = p2.expand(B, N, p2.shape[2])
    else:
        idx, w = three_nn(xyz1, xyz2)
        bidx = torch.arange(B, device=idx.device).view(B, 1, 1)
        interp = (p2[bidx, idx.long()] * w.double().unsqueeze(-1)).sum(2)
    x = interp if points1 is None else torch.cat([points1.double(), interp], -1)
    return _mlp64(fp.mlp, x)


def _ref_net(net, xyz, feat, onehot, sampling):
    """fp64 evaluation of the whole part-seg network on the index lists of ``sampling``: ([sa1..3, fp3, fp2, fp1], logits [B,N,P])."""
    B, N, _ = xyz.shape
    x, f = xyz, feat
    enc = []
    for module, (new_xyz, idxs) in zip(net.pointnet_modules, sampling["levels"]):
        if new_xyz is None:
            out = _mlp64(module.mlps[0], torch.cat([x.double(), f.double()], -1)).max(dim=1, keepdim=True)[0]
        else:
            parts = []
            bidx = torch.arange(B, device=xyz.device).view(B, 1, 1)
            for mlp, ic in zip(module.mlps, idxs):
                idx, cnt = ic[0].long(), ic[1]
                g = torch.cat([x.double()[bidx, idx] - new_xyz.double().unsqueeze(2), f.double()[bidx, idx]], -1)
                y = _mlp64(mlp, g)
                valid = torch.arange(idx.shape[2], device=idx.device).view(1, 1, -1) < cnt.clamp(min=1).unsqueeze(-1)
                parts.append(y.masked_fill(~valid.unsqueeze(-1), float("-inf")).max(dim=2)[0])
            out = torch.cat(parts, -1)
            x = new_xyz
        enc.append((x, out))
        f = out
    (l1_xyz, l1), (l2_xyz, l2), (_, l3) = enc
    l3_xyz = torch.zeros(B, 1, 3, device=xyz.device)
    f3 = _fp64_fp(net.fp3, l2_xyz, l3_xyz, l2, l3)
    f2 = _fp64_fp(net.fp2, l1_xyz, l2_xyz, l1, f3)
    skip = torch.cat([onehot.view(B, 1, 16).expand(B, N, 16), xyz, feat], 2)
    f1 = _fp64_fp(net.fp1, xyz, l1_xyz, skip, f2)
    return [l1, l2, l3, f3, f2, f1], _mlp64(net.head2, _mlp64(net.head1, f1))


def _eval_levels(net, xyz, feat, onehot, sampling, flush_k=0):
    """The existing evaluation path (net.eval() + no_grad) on a copy with the given accumulation, level by level."""
    from pointcloudlib_amd.misc.layers import set_accumulation
    ev = set_accumulation(copy.deepcopy(net).eval(), flush_k)
    B, N, _ = xyz.shape
    with torch.no_grad():
        lv = sampling["levels"]
        l1_xyz, l1 = ev.pointnet_modules[0](xyz, feat, lv[0])
        l2_xyz, l2 = ev.pointnet_modules[1](l1_xyz, l1, lv[1])
        _, l3 = ev.pointnet_modules[2](l2_xyz, l2, lv[2])
        l3_xyz = torch.zeros((B, 1, 3), device=xyz.device)
        f3 = ev.fp3(l2_xyz, l3_xyz, l2, l3)
        f2 = ev.fp2(l1_xyz, l2_xyz, l1, f3)
        f1 = ev.fp1(xyz, l1_xyz, torch.cat([onehot.view(B, 1, 16).expand(B, N, 16), xyz, feat], 2), f2)
        return [l1, l2, l3, f3, f2, f1], ev.head2(ev.head1(f1))


def _err(a, ref):
    return (a.double() - ref).abs().max().item()


# ----------------------------------------------------------------------------------------------------------- the kernel
# (name, skip channels D1 (one-hot included), coarse channels D2, FP widths, head) -- the rows of the shape table
_SHAPES = [("fp3", 256, 1024, [256, 256], False), ("fp2", 128, 256, [256, 128], False),
           ("fp1", 22, 128, [128, 128, 128], False), ("fp1_head", 22, 128, [128, 128, 128], True)]
_PART = 50


def _kernel_case(dev, D1, D2, widths, head, slope, S, seed):
    from pointcloudlib_amd.misc.layers import PointwiseMLP, set_accumulation
    from pointcloudlib_amd.misc.ops import PointNetFeaturePropagation
    torch.manual_seed(seed)
    B, N = 3, 700                                    # odd B; B * N not a multiple of the 64-row tile
    fp = PointNetFeaturePropagation(D1 + D2, widths)
    fp.mlp.slope = slope
    heads = ()
    if head:
        heads = (PointwiseMLP([128, 128], bias=True, slope=slope, last_act=False),
                 PointwiseMLP([128, _PART], bias=True, bn=False, last_act=False))
    mods = torch.nn.ModuleList([fp, *heads]).to(dev)
    _perturb(mods, seed)
    set_accumulation(mods, 0)
    mods.eval()
    xyz1 = torch.rand(B, N, 3, device=dev)
    xyz2 = torch.rand(B, S, 3, device=dev)
    skip = torch.randn(B, N, D1, device=dev)
    if D1 == 22:                                     # FP1: a one-hot class label, then xyz + normal
        skip[:, :, :16] = 0.0
        for b in range(B):
            skip[b, :, (5 * b + 3) % 16] = 1.0
    coarse = torch.randn(B, S, D2, device=dev).abs()                 # post-ReLU features
    return fp, heads, xyz1, xyz2, skip, coarse


def _fused_call(fp, heads, xyz1, xyz2, skip, coarse):
    """The plan's snapshot, the tables computed here, and ONE pcl_fp_level_infer_f32 call through the C ABI into a wider output
    (and tap) pre-filled with a sentinel."""
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.inference import _FusedFP
    from pointcloudlib_amd.misc.ops import three_nn
    B, N, D1 = skip.shape
    S = coarse.shape[1]
    n_oh = 16 if D1 == 22 else 0
    plan = _FusedFP(fp.mlp, D1, n_oh, heads)
    rows = _FusedFP._rows
    Uc = rows(coarse.reshape(B * S, -1).contiguous(), plan.Wc, B * S)
    idx3, w3 = three_nn(xyz1, xyz2)                  # S = 1 too: (0, 0, 0) with weights (1, 0, 0)
    cb = rows(skip[:, 0, :16].contiguous(), plan.Woh, B) if n_oh else None
    fs = skip[:, :, n_oh:].reshape(B * N, -1).contiguous()
    Us = None
    if not plan.inline:
        Us, fs = rows(fs, plan.Wsk, B * N), None
    CL = plan.widths[-1]
    ldo = CL + 9
    out = torch.full((B * N, ldo), 7.0, device=xyz1.device)
    tap = ldt = None
    if plan.tap_layer is not None:
        ldt = plan.widths[plan.tap_layer] + 5
        tap = torch.full((B * N, ldt), 7.0, device=xyz1.device)
    _lib.call("pcl_fp_level_infer_f32", _P(Us), _P(fs), _P(plan.Wsk) if fs is not None else None, 0 if fs is None else fs.shape[1],
              plan.W0.shape[1], _P(Uc), _P(idx3), _P(w3), S, _P(cb), B, N, len(plan.widths), plan.c_widths, plan.c_W, plan.c_scale,
              plan.c_shift, plan.act_mask, plan.slope, _P(out), ldo, _P(tap), -1 if tap is None else plan.tap_layer,
              0 if tap is None else ldt, _stream())
    assert bool((out[:, CL:] == 7.0).all()), "wrote outside its ldo slice"
    res = [out[:, :CL].reshape(B, N, CL)]
    if tap is not None:
        tw = plan.widths[plan.tap_layer]
        assert bool((tap[:, tw:] == 7.0).all()), "tap: wrote outside its ldt slice"
        res.append(tap[:, :tw].reshape(B, N, tw))
    return res


@pytest.mark.parametrize("name,D1,D2,widths,head", _SHAPES, ids=[s[0] for s in _SHAPES])
@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("S", [1, 2, 128, 512])
def test_fp_level_kernel_against_fp64(dev, name, D1, D2, widths, head, slope, S):
    fp, heads, xyz1, xyz2, skip, coarse = _kernel_case(dev, D1, D2, widths, head, slope, S, seed=S + D1 + int(10 * slope))
    with torch.no_grad():
        got = _fused_call(fp, heads, xyz1, xyz2, skip, coarse)
        again = _fused_call(fp, heads, xyz1, xyz2, skip, coarse)
        ev = [fp(xyz1, xyz2, skip, coarse)]
        if heads:
            ev = [heads[1](heads[0](ev[0])), ev[0]]
    torch.cuda.synchronize()
    assert all(torch.equal(g, a) for g, a in zip(got, again)), "two calls differ"
    ref = [_fp64_fp(fp, xyz1, xyz2, skip, coarse)]
    if heads:
        ref = [_mlp64(heads[1], _mlp64(heads[0], ref[0])), ref[0]]
    for g, e, r in zip(got, ev, ref):
        assert g.shape == e.shape
        ef, ee = _err(g, r), _err(e, r)
        assert ef <= 1.25 * ee + 1e-6, f"fused {ef:.3e} vs eval path {ee:.3e} from fp64"


# ----------------------------------------------------------------------------------------------------------- networks
def _net(kind, dev, seed=0, **kw):
    from pointcloudlib_amd.networks.seg.pointnet2_partseg import PointNet2_partseg, PointNetMSG
    torch.manual_seed(seed)
    net = (PointNet2_partseg if kind == "ssg" else PointNetMSG)(**kw).to(dev)
    return _perturb(net, seed + 1)


def _clouds(dev, B, N=2048, seed=0):
    from pointcloudlib_amd import synth
    xyz = torch.from_numpy(synth.gauss_ball(B, N, seed)).to(dev)
    nrm = torch.from_numpy(synth.unit_normals(B, N, seed + 1)).to(dev)
    onehot = torch.zeros(B, 16, device=dev)
    onehot[torch.arange(B), torch.arange(B) % 16] = 1.0
    return xyz, nrm, onehot


def _check_network(net, xyz, nrm, onehot, report=None):
    from pointcloudlib_amd.inference import frozen
    samp = net.precompute_sampling(xyz)
    fnet = frozen(net)
    levels, logits = fnet.run(xyz, nrm, onehot, sampling=samp)
    ev_levels, ev_logits = _eval_levels(net, xyz, nrm, onehot, samp, 0)
    ref_levels, ref_logits = _ref_net(net, xyz, nrm, onehot, samp)
    torch.cuda.synchronize()
    names = ["sa1", "sa2", "sa3", "fp3", "fp2", "fp1"]
    rows = {}
    for n, f, e, r in zip(names, levels, ev_levels, ref_levels):
        assert f.shape == e.shape, n
        ef, ee = _err(f, r), _err(e, r)
        rows[n] = (ef, ee)
        assert ef <= 1.25 * ee + 1e-6, f"{n}: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    assert logits.shape == (xyz.shape[0], net.part_num, xyz.shape[1])
    lg = logits.permute(0, 2, 1)
    ef, ee = _err(lg, ref_logits), _err(ev_logits, ref_logits)
    rows["logits"] = (ef, ee)
    assert ef <= 1.25 * ee + 1e-6, f"logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    bound = 1.25 * ee + 1e-6
    top2 = ref_logits.topk(2, dim=2)[0]
    sure = (top2[..., 0] - top2[..., 1]) > 2 * bound
    assert bool((lg.argmax(2) == ref_logits.argmax(2))[sure].all())
    if report is not None:
        _, ev32_logits = _eval_levels(net, xyz, nrm, onehot, samp, 32)
        rows["logits_vs_eval_flush32"] = (ef, _err(ev32_logits, ref_logits))
        report.update(rows)
    return fnet


@pytest.mark.parametrize("kind", ["ssg", "msg"])
def test_frozen_partseg_network_against_fp64(dev, kind):
    net = _net(kind, dev)
    xyz, nrm, onehot = _clouds(dev, 16)
    report = {}
    _check_network(net, xyz, nrm, onehot, report)
    # (frozen, eval) max-abs distance from fp64 per tensor; the last row against the default flush-32 eval path
    print(f"\n[partseg {kind} B=16 N=2048 err vs fp64] " + ", ".join(f"{k}: {a:.3e}/{b:.3e}" for k, (a, b) in report.items()))


def test_frozen_partseg_forward_memory(dev):
    from pointcloudlib_amd.inference import frozen
    net = _net("msg", dev)
    B, N, P = 16, 2048, 50
    xyz, nrm, onehot = _clouds(dev, B)
    samp = net.precompute_sampling(xyz)
    fnet = frozen(net)
    fnet(xyz, nrm, onehot, sampling=samp)                 # warm-up: one-time allocations (constants, plans)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fnet(xyz, nrm, onehot, sampling=samp)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    level_out = B * 512 * 320 + B * 128 * 640 + B * 1024 + B * 128 * 256 + B * 512 * 128 + B * N * 128
    tables = B * 512 * (64 + 128 + 128) + B * 128 * 256 + B * 256 + B * 512 * 256 + B * 128 * 256 + B * 512 * 128 + B * 128
    three = 2 * 3 * (B * 512 + B * N)
    group_all = B * 128 * (3 + 640 + 256 + 512 + 1024)
    logits = B * N * P + B * N * 6                          # (+ FP1's inline skip, xyz and normal)
    bound = 2 * 4 * (level_out + tables + three + group_all + logits)
    assert out.shape == (B, P, N)
    assert peak <= bound, f"frozen forward peak +{peak / 2**20:.1f} MiB > bound {bound / 2**20:.1f} MiB"
    assert peak < 4 * B * 512 * 128 * 64, "a B*m*ns*C grouped tensor was materialised"


def test_frozen_partseg_contract(dev):
    from pointcloudlib_amd.inference import frozen
    net = _net("ssg", dev).train()
    xyz, nrm, onehot = _clouds(dev, 4, N=1024, seed=3)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = frozen(net)
    out_inline = fnet(xyz, nrm, onehot)
    out_handle = fnet(xyz, nrm, onehot, sampling=net.precompute_sampling(xyz))
    torch.cuda.synchronize()
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(out_inline, out_handle), "a precomputed sampling handle changes the output"
    with torch.no_grad():
        ref = net.eval()(xyz, nrm, onehot)
    net.train()
    assert out_inline.shape == ref.shape and out_inline.stride() == ref.stride(), "not the network's layout / view"
    # refresh() re-reads the running statistics (a decoder one)
    with torch.no_grad():
        net.fp2.mlp.running_var_1.mul_(3.0)
    stale = fnet(xyz, nrm, onehot)
    fresh = fnet.refresh()(xyz, nrm, onehot)
    torch.cuda.synchronize()
    assert torch.equal(stale, out_inline)
    assert not torch.equal(fresh, out_inline)
    assert torch.equal(fresh, frozen(net)(xyz, nrm, onehot))


def test_frozen_partseg_falls_back_for_other_widths(dev):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.misc.ops import PointNetFeaturePropagation
    assert not _lib.lib().pcl_fp_level_infer_supported(2, 200, 100, 0, 0, 0)
    net = _net("msg", dev)
    torch.manual_seed(5)
    net.fp2 = PointNetFeaturePropagation(576, [200, 100]).to(dev)
    net.fp1 = PointNetFeaturePropagation(100 + 22, [128, 128, 128]).to(dev)
    _perturb(net, 9)
    xyz, nrm, onehot = _clouds(dev, 16, seed=4)
    fnet = _check_network(net, xyz, nrm, onehot)
    assert [fnet.fp[k][0] for k in ("fp3", "fp2", "fp1")] == ["fused", "module", "fused"]


def test_train_partseg_fast_eval(dev):
    cmd = [sys.executable, os.path.join(ROOT, "train_partseg.py"), "--model", "pointnet2_msg", "--fast_eval", "--epochs", "1",
           "--batch_size", "8", "--num_points", "512"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Test 0," in r.stdout
