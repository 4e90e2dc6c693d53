"""PointNet, its T-Nets and PointNet part segmentation on ragged batches through packed rows on the GPU.

The classifier is held to the project's own yardstick (oracle/parity.py, unmodified rules, no waiver) against a ragged restatement
built from ``oracle.cpu_pointnet.PointNetClsCPU``'s own pieces; at the bit level every packed path is compared with a composite of
the EXISTING operators on the concatenated valid rows: the un-pooled ``PointwiseMLP``, a per-cloud ``torch.max`` over the slice,
``v[row_cloud]`` indexing, ``torch.cat``.  Forward values, the loss and the running statistics must agree bit for bit (the same
GEMMs and BatchNorm statistics, the same fmaf + lrelu expression, and a max is exact); parameter gradients within GRAD_FLOOR
(relative L2): the winners are the same, the fp64 BatchNorm-backward partial sums are partitioned differently."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, LENGTHS = 300, [300, 1, 129, 257]
B, R = len(LENGTHS), sum(LENGTHS)


def _same(a, b):
    """Bit equality (NaN-safe, -0.0 != +0.0)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _perturb(net, seed):
    """Running statistics, gamma and beta of every BatchNorm of the conv stacks away from their initial values (some gamma < 0)."""
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in net.modules():
            if not (isinstance(mod, PointwiseMLP) and mod.bn):
                continue
            for l in range(mod.n_layers):
                c = mod.gammas[l].numel()
                sign = torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
                mod.gammas[l].copy_(sign * (0.5 + torch.rand(c, generator=g)))
                mod.betas[l].copy_(0.1 * torch.randn(c, generator=g))
                getattr(mod, f"running_mean_{l}").copy_(0.1 * torch.randn(c, generator=g))
                getattr(mod, f"running_var_{l}").copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return net


def _fill(x, lengths, how):
    """x [B,N,3] numpy with its pad rows replaced."""
    out = x.copy()
    for b, n in enumerate(lengths):
        k = out.shape[1] - n
        if k == 0:
            continue
        if how == "copies":
            out[b, n:] = np.resize(x[b, :n][::-1], (k, 3))
        else:
            out[b, n:] = {"zeros": 0.0, "nan": np.nan}[how]
    return out


def _cloud(dev, how, lengths=LENGTHS, n=N, seed=7):
    """[B,3,N] on the device, pads filled."""
    from pointcloudlib_amd import synth
    x = _fill(synth.gauss_ball(len(lengths), n, seed), lengths, how)
    return torch.from_numpy(x).transpose(1, 2).contiguous().to(dev)


def _valid_rows(x, lengths=LENGTHS):
    """x [B,3,N] -> the valid points of every cloud, cloud after cloud [R,3] (plain indexing)."""
    return torch.cat([x[b, :, :n].t() for b, n in enumerate(lengths)], 0).contiguous()


def _seg_max(rows, lengths=LENGTHS):
    out, o = [], 0
    for n in lengths:
        out.append(rows[o:o + n].max(dim=0)[0])
        o += n
    return torch.stack(out)


def _snapshot(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def _check_grads(got, want, what, zero_in_theory=()):
    """Every parameter gradient within GRAD_FLOOR (relative L2, oracle.parity.rel) of the composite's.  ``zero_in_theory`` NAMES the
    tensors whose gradient vanishes in exact arithmetic -- a conv bias under BatchNorm (``*.biases.*`` of a BatchNorm stack); the beta of
    part-seg's conv5, whose shift of out5 and of its max the next BatchNorm removes.  Both sides are rounding noise there and a
    relative error of it means nothing, so those, and only those, are held to Report.grads' noise-floor rule instead: |error| and
    both values <= ABS_FLOOR of the model's largest gradient entry.  The exempted names are printed."""
    from oracle.parity import ABS_FLOOR, GRAD_FLOOR, rel
    assert set(got) == set(want)
    assert all(k in want for k in zero_in_theory), f"{what}: unknown parameter among {zero_in_theory}"
    worst, n_rel = 0.0, 0
    gscale = max(g.abs().max().item() for g in want.values())
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), f"{what}: gradient of {k} is not finite"
        if k in zero_in_theory:
            for side, g in (("packed", got[k]), ("composite", want[k])):
                assert g.abs().max().item() <= ABS_FLOOR * gscale, (f"{what}: gradient of {k} ({side}) should vanish: "
                                                                    f"{g.abs().max().item():.2e} vs {ABS_FLOOR} x {gscale:.2e}")
            continue
        e = rel(got[k].double(), want[k].double())[0]
        worst, n_rel = max(worst, e), n_rel + 1
        assert e <= GRAD_FLOOR, f"{what}: gradient of {k}: relative L2 {e:.3e} vs the composite's (GRAD_FLOOR {GRAD_FLOOR})"
    assert n_rel + len(zero_in_theory) == len(want)
    print(f"{what}: {n_rel} parameter gradients within GRAD_FLOOR of the composite's, worst relative L2 {worst:.2e}; "
          f"zero in theory, held to the noise floor: {sorted(zero_in_theory)}")


def _spy_links(monkeypatch):
    """Record the ``link`` of every ``ops.segment_max`` call: a DeferLink = the training form (the stack stopped at its pre-BatchNorm
    output, the activated [R, C] tensor is never written), None = the plain form."""
    from pointcloudlib_amd.misc import ops
    seen, real = [], ops.segment_max

    def spy(*a, **k):
        seen.append(k.get("link"))
        return real(*a, **k)
    monkeypatch.setattr(ops, "segment_max", spy)
    return seen


def _assert_training_form(links, n):
    """``n`` poolings took the training form and each handed its stack du's BatchNorm-backward stats rows in the backward."""
    taken = [l for l in links if l is not None]
    assert len(taken) == n, f"{len(taken)} of the expected {n} poolings took the training form (DeferLink)"
    assert all(1 <= l.rows <= 1024 and l.stats is None for l in taken), "a DeferLink's stats rows were not produced and consumed"


def _bn_biases(net):
    """Names of the conv biases that sit under a BatchNorm (every PointwiseMLP of these networks has one)."""
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    assert all(m.bn for m in net.modules() if isinstance(m, PointwiseMLP))
    return tuple(k for k, _ in net.named_parameters() if ".biases." in k)


# ------------------------------------------------------------------------------------------------- 1. parity of the classifier
def test_ragged_pointnet_cls_parity_by_the_projects_yardstick(dev):
    from oracle.cpu_pointnet import PointNetClsCPU
    from oracle.parity import Report
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    from pointcloudlib_amd.train_utils import soft_cross_entropy_loss
    Bp, Np = 8, 1024
    lengths = [1024, 1, 512, 513, 777, 257, 300, 64]
    pts, lab = synth.gauss_ball(Bp, Np, 20241), torch.from_numpy(synth.labels(Bp, 40, 21141))
    torch.manual_seed(0)
    net = PointNet().to(dev).train()
    net.dp1.p = 0.0                                              # dropout off on both sides
    state = net.state_dict()

    def restatement(r):
        """PointNetClsCPU.forward with the max per cloud over its own rows, from the restatement's own pieces."""
        rows = torch.cat([torch.from_numpy(pts[b, :n]) for b, n in enumerate(lengths)], 0).to(r.dtype)
        y = r.mlp("convs.", rows)
        pooled = _seg_max(y, lengths)
        z = r.fc_bn_act(pooled, "linear1", "bn6", 0.0)
        return r.fc_bn_act(z, "linear2")

    r32, r64 = PointNetClsCPU(state), PointNetClsCPU(state, dtype=torch.float64)
    o32, o64 = restatement(r32), restatement(r64)
    soft_cross_entropy_loss(o32, lab).backward()
    soft_cross_entropy_loss(o64, lab).backward()
    x = torch.from_numpy(_fill(pts, lengths, "nan")).transpose(1, 2).contiguous().to(dev)        # pad rows NaN on the GPU side
    out = net(x, lengths=lengths)
    assert out.shape == (Bp, 40)
    soft_cross_entropy_loss(out, lab.to(dev)).backward()
    rep = Report(f"PointNet cls ragged B={Bp} N={Np}")
    rep.feature(out, o32, o64, "logits")
    g_hip = {n: p.grad for n, p in net.named_parameters()}
    rep.grads(g_hip, {n: r32.grad(n) for n in g_hip}, {n: r64.grad(n) for n in g_hip})
    rep.finish()
    assert not rep.waived


# ------------------------------------------------------------------------------------------------- 2. bit level, classifier
def _cls_net(dev):
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    torch.manual_seed(0)
    net = _perturb(PointNet().to(dev), 1)
    net.dp1.p = 0.0
    return net


def _cls_labels(dev):
    from pointcloudlib_amd import synth
    return torch.from_numpy(synth.labels(B, 40, 11)).to(dev)


def _cls_step(net, x, dev, ragged=True):
    from pointcloudlib_amd.train_utils import soft_cross_entropy_loss
    out = net(x, lengths=LENGTHS) if ragged else net(x)
    loss = soft_cross_entropy_loss(out, _cls_labels(dev))
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.detach().clone()


def _cls_composite_step(net, x, dev):
    """The same step from the existing operators: un-pooled conv stack on the concatenated valid rows, torch.max per cloud."""
    from pointcloudlib_amd.misc.head import fc_head
    from pointcloudlib_amd.train_utils import soft_cross_entropy_loss
    feat = net.convs(_valid_rows(x))
    assert feat.shape == (R, 1024)
    out = fc_head([net.linear1, net.bn6, net.relu, net.dp1, net.linear2], _seg_max(feat))
    loss = soft_cross_entropy_loss(out, _cls_labels(dev))
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.detach().clone()


def test_ragged_pointnet_cls_equals_the_composite_of_existing_operators(dev, monkeypatch):
    links = _spy_links(monkeypatch)
    base = _cls_net(dev)
    a, b = copy.deepcopy(base).train(), copy.deepcopy(base).train()
    before = _snapshot(base)
    x = _cloud(dev, "zeros")
    out, loss = _cls_step(a, x, dev)
    _assert_training_form(links, 1)
    assert len(links) == 1
    want, want_loss = _cls_composite_step(b, x, dev)
    assert _same(out, want), f"logits: max |diff| {(out - want).abs().max().item():.3e}"
    assert _same(loss, want_loss), f"loss {loss.item()!r} vs {want_loss.item()!r}"
    sa, sb = _snapshot(a), _snapshot(b)
    moved = 0
    for k in sa:
        if "running" in k:
            assert _same(sa[k], sb[k]), f"running statistic {k}"
            moved += int(not torch.equal(sa[k], before[k]))
    assert moved >= 10, "running statistics did not move"
    _check_grads(_grads(a), _grads(b), "PointNet cls")


# ------------------------------------------------------------------------------------------------- 3. nothing leaks
def test_ragged_pointnet_cls_ignores_pads_and_other_clouds(dev):
    base = _cls_net(dev)
    # evaluation mode: cloud 0 alone decides its logits
    net = copy.deepcopy(base).eval()
    with torch.no_grad():
        x = _cloud(dev, "nan")
        ref = net(x, lengths=LENGTHS)
        other = _cloud(dev, "zeros", seed=8)                     # other points everywhere ...
        other[0, :, :LENGTHS[0]] = x[0, :, :LENGTHS[0]]          # ... except cloud 0's own
        got = net(other, lengths=LENGTHS)
    assert bool(torch.isfinite(ref).all())
    assert _same(got[0], ref[0]), "evaluation: cloud 0's logits depend on other clouds or on pad rows"
    assert not _same(got[1:], ref[1:])
    # training mode: pads of any kind change nothing
    runs = {}
    for how in ("zeros", "nan", "copies"):
        net = copy.deepcopy(base).train()
        runs[how] = _cls_step(net, _cloud(dev, how), dev)
        assert all(bool(torch.isfinite(g).all()) for g in _grads(net).values()), f"pads = {how}: a gradient is not finite"
    for how in ("nan", "copies"):
        assert _same(runs[how][0], runs["zeros"][0]), f"pads = {how} changed the training logits"
        assert _same(runs[how][1], runs["zeros"][1]), f"pads = {how} changed the training loss"
    # not vacuous: the dense forward on the zero-padded batch counts the pads
    dense = copy.deepcopy(base).train()
    _, dense_loss = _cls_step(dense, _cloud(dev, "zeros"), dev, ragged=False)
    assert not _same(dense_loss, runs["zeros"][1]) and abs(dense_loss.item() - runs["zeros"][1].item()) > 1e-4
    # device lengths with n_rows: the same step without a read-back
    net = copy.deepcopy(base).train()
    out = net(_cloud(dev, "nan"), lengths=torch.tensor(LENGTHS, dtype=torch.int32, device=dev), n_rows=R)
    assert _same(out.detach(), runs["zeros"][0])


# ------------------------------------------------------------------------------------------------- 4. T-Nets and part-seg
@pytest.mark.parametrize("k", [3, 128])
def test_stn_forward_packed_equals_its_composite(dev, k, monkeypatch):
    links = _spy_links(monkeypatch)
    from pointcloudlib_amd.misc import ops
    from pointcloudlib_amd.misc.stn import STNkd
    torch.manual_seed(k)
    base = _perturb(STNkd(k).to(dev), 2)
    a, b = copy.deepcopy(base).train(), copy.deepcopy(base).train()
    rows = torch.randn(R, k, generator=torch.Generator().manual_seed(5)).to(dev)
    _, row_off, rows_n, rc = ops.packed_layout(LENGTHS, B, N, dev)
    assert rows_n == R
    ra, rb = rows.clone().requires_grad_(True), rows.clone().requires_grad_(True)
    got = a.forward_packed(ra, row_off, rc, B)
    g = _seg_max(b.convs(rb))
    want = (b.fc3(b.fcs(g)) + torch.eye(k, device=dev).reshape(1, k * k)).reshape(B, k, k)
    assert got.shape == (B, k, k)
    assert _same(got.detach(), want.detach()), f"max |diff| {(got - want).abs().max().item():.3e}"
    w = torch.randn(B, k, k, generator=torch.Generator().manual_seed(6)).to(dev)
    (got * w).sum().backward()
    (want * w).sum().backward()
    _assert_training_form(links, 1)
    sa, sb = _snapshot(a), _snapshot(b)
    assert all(_same(sa[n], sb[n]) for n in sa if "running" in n)
    _check_grads(_grads(a), _grads(b), f"STNkd k={k}", _bn_biases(a))
    from oracle.parity import GRAD_FLOOR, rel
    assert rel(ra.grad.double(), rb.grad.double())[0] <= GRAD_FLOOR, "gradient reaching the rows"


def _seg_net(dev):
    from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
    torch.manual_seed(0)
    return _perturb(PointNet_partseg(50).to(dev), 3)


def _onehot(dev):
    onehot = torch.zeros(B, 16, device=dev)
    onehot[torch.arange(B), (5 * torch.arange(B) + 3) % 16] = 1.0
    return onehot


def _seg_labels(dev):
    return torch.randint(0, 50, (B, N), generator=torch.Generator().manual_seed(5)).to(dev)


def _seg_step(net, x, dev):
    from pointcloudlib_amd.misc import ops
    from pointcloudlib_amd.train_utils import seg_cross_entropy_loss
    logits, row_off = net.forward_packed(x, _onehot(dev), lengths=LENGTHS)
    loss = seg_cross_entropy_loss(logits, ops.pack_rows(_seg_labels(dev), LENGTHS, row_off, R))
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach().clone()


def _seg_composite_step(net, x, dev):
    """PointNet_partseg.forward on the concatenated valid rows from the existing modules and operators."""
    from pointcloudlib_amd.misc import ops
    from pointcloudlib_amd.train_utils import seg_cross_entropy_loss
    row_off, _ = ops.row_offsets(LENGTHS, B, N, dev)
    cloud_of = torch.repeat_interleave(torch.arange(B), torch.tensor(LENGTHS)).to(dev)
    seg = _seg_labels(dev)

    def tnet(stn, rows):
        g = _seg_max(stn.convs(rows))
        return (stn.fc3(stn.fcs(g)) + torch.eye(stn.k, device=dev).reshape(1, -1)).reshape(B, stn.k, stn.k)

    def transform(rows, T):
        return ops.pack_rows(torch.bmm(ops.unpack_rows(rows, LENGTHS, row_off, N), T), LENGTHS, row_off, R)

    pc = _valid_rows(x)
    pc = transform(pc, tnet(net.stn, pc))
    out1 = net.conv1(pc)
    out2 = net.conv2(out1)
    out3 = net.conv3(out2)
    out4 = net.conv4(transform(out3, tnet(net.fstn, out3)))
    out5 = net.conv5(out4)
    expand = torch.cat((_seg_max(out5), _onehot(dev)), 1)[cloud_of]
    logits = net.convs4(net.convs(torch.cat([expand, out1, out2, out3, out4, out5], 1)))
    loss = seg_cross_entropy_loss(logits, torch.cat([seg[b, :n] for b, n in enumerate(LENGTHS)]))
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach().clone()


def test_pointnet_partseg_forward_packed_equals_the_composite_and_ignores_pads(dev, monkeypatch):
    from pointcloudlib_amd.train_utils import seg_cross_entropy_loss
    links = _spy_links(monkeypatch)
    base = _seg_net(dev)
    before = _snapshot(base)
    a, b = copy.deepcopy(base).train(), copy.deepcopy(base).train()
    logits, loss = _seg_step(a, _cloud(dev, "zeros"), dev)
    _assert_training_form(links, 2)                              # the two T-Nets; out5 is needed as rows and pooled as it is
    assert [l is None for l in links] == [False, False, True]
    want, want_loss = _seg_composite_step(b, _cloud(dev, "zeros"), dev)
    assert logits.shape == (R, 50)
    assert _same(logits, want), f"logits: max |diff| {(logits - want).abs().max().item():.3e}"
    assert _same(loss, want_loss), f"loss {loss.item()!r} vs {want_loss.item()!r}"
    sa, sb = _snapshot(a), _snapshot(b)
    moved = 0
    for k in sa:
        if "running" in k:
            assert _same(sa[k], sb[k]), f"running statistic {k}"
            moved += int(not torch.equal(sa[k], before[k]))
    assert moved >= 30, "running statistics did not move"
    _check_grads(_grads(a), _grads(b), "PointNet part-seg", _bn_biases(a) + ("conv5.betas.0",))
    # nothing leaks, training mode: pads of any kind change nothing and every gradient is finite
    for how in ("nan", "copies"):
        net = copy.deepcopy(base).train()
        l2, loss2 = _seg_step(net, _cloud(dev, how), dev)
        assert _same(l2, logits) and _same(loss2, loss), f"pads = {how} changed the training step"
        assert all(bool(torch.isfinite(g).all()) for g in _grads(net).values()), f"pads = {how}: a gradient is not finite"
    # not vacuous: the dense forward on the zero-padded batch, seg labels on every padded point, counts the pads
    dense = copy.deepcopy(base).train()
    dense_loss = seg_cross_entropy_loss(dense(_cloud(dev, "zeros"), _onehot(dev)), _seg_labels(dev)).detach()
    assert not _same(dense_loss, loss) and abs(dense_loss.item() - loss.item()) > 1e-4
    # evaluation mode: cloud 0's rows depend on cloud 0 alone
    net = copy.deepcopy(base).eval()
    with torch.no_grad():
        x = _cloud(dev, "nan")
        ref, _ = net.forward_packed(x, _onehot(dev), lengths=LENGTHS)
        other = _cloud(dev, "zeros", seed=8)
        other[0, :, :LENGTHS[0]] = x[0, :, :LENGTHS[0]]
        got, _ = net.forward_packed(other, _onehot(dev), lengths=LENGTHS)
    assert bool(torch.isfinite(ref).all())
    assert _same(got[:LENGTHS[0]], ref[:LENGTHS[0]]), "evaluation: cloud 0's logits depend on other clouds or on pad rows"
    assert not _same(got[LENGTHS[0]:], ref[LENGTHS[0]:])


def test_pointnet_partseg_forward_packed_without_lengths_is_the_dense_forward(dev):
    from oracle.parity import ATOL, RTOL
    base = _seg_net(dev)
    a, b = copy.deepcopy(base).train(), copy.deepcopy(base).train()
    x = _cloud(dev, "zeros", lengths=[N] * B)
    rows, row_off = a.forward_packed(x, _onehot(dev))
    assert rows.shape == (B * N, 50) and row_off.tolist() == [0, N, 2 * N, 3 * N, 4 * N]
    dense = b(x, _onehot(dev))                                   # [B, 50, N]
    got, want = rows.detach().view(B, N, 50).permute(0, 2, 1).double(), dense.detach().double()
    err = (got - want).abs()
    bound = ATOL + RTOL * want.abs()
    print(f"forward_packed without lengths vs forward: worst err / bound = {(err / bound).max().item():.3g}")
    assert bool((err <= bound).all()), f"worst err / bound = {(err / bound).max().item():.3g}"
