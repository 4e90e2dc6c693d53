"""Whole PointNet++ networks on ragged batches (``lengths=``) on the GPU.

Truth for cloud b is the same network on ``x[b:b+1, :n_b]``.  Raggedness lives in the first level only: the sampling handle of the
ragged batch must equal the per-cloud handles bit for bit, level by level (which is also the test that the set-abstraction and
grouped kernels need no count: they reach the cloud through idx, and idx never names a pad row), and because the MFMA products are
row-wise the frozen outputs are asserted bit-identical to the per-cloud runs.  Every sampler gets an explicit ``tie_stride`` (the
default is a function of B, so a B = 1 run would use another tie rule than the batch)."""
import numpy as np
import pytest
import torch

from test_inference_gpu import _perturb

pytestmark = pytest.mark.gpu

TIE = 4
FILLS = ("copies", "nan", "huge")
CLS_N, CLS_LENGTHS = 1024, [1024, 1000, 777, 640, 513, 512]          # N, n_samples + 1, n_samples, not multiples of 64
SEG_N, SEG_LENGTHS = 2048, [2048, 512, 513, 2011, 1281, 1500]        # (cloud 1: 24 of its 32 FP1 tiles hold pad rows only)


def _net(task, kind, dev, seed=0):
    from pointcloudlib_amd.networks.cls import pointnet2 as cls_nets
    from pointcloudlib_amd.networks.seg import pointnet2_partseg as seg_nets
    torch.manual_seed(seed)
    mod = cls_nets if task == "cls" else seg_nets
    net = (getattr(mod, "PointNet2_cls" if task == "cls" else "PointNet2_partseg") if kind == "ssg" else mod.PointNetMSG)().to(dev)
    for m in net.pointnet_modules:
        if m.sampler is not None:
            m.sampler.tie_stride = TIE
    return _perturb(net, seed + 1)


def _fill(x, lengths, how):
    out = x.copy()
    N = x.shape[1]
    for b, n in enumerate(lengths):
        k = N - n
        if k == 0:
            continue
        if how == "copies":
            out[b, n:] = x[b, :k][::-1] if k <= n else np.resize(x[b, :n][::-1], (k, 3))
        elif how == "zeros":
            out[b, n:] = 0.0
        elif how == "nan":
            out[b, n:] = np.nan
        else:
            out[b, n:] = 1e30
    return out


def _clouds(dev, lengths, N, how, seed=7):
    from pointcloudlib_amd import synth
    B = len(lengths)
    xyz, nrm = synth.gauss_ball(B, N, seed), synth.unit_normals(B, N, seed + 1)
    return torch.from_numpy(_fill(xyz, lengths, how)).to(dev), torch.from_numpy(_fill(nrm, lengths, how)).to(dev)


def _onehot(dev, B):
    onehot = torch.zeros(B, 16, device=dev)
    onehot[torch.arange(B), (5 * torch.arange(B) + 3) % 16] = 1.0
    return onehot


def _same(a, b):
    """Bit equality (NaN-safe, -0.0 != +0.0)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_handles_equal(net, batch, singles):
    """The ragged batch's sampling handle against the per-cloud handles, level by level, bit for bit."""
    for i, (new_xyz, idxs) in enumerate(batch["levels"]):
        for b, one in enumerate(singles):
            o_xyz, o_idxs = one["levels"][i]
            if new_xyz is None:
                assert o_xyz is None and all(ic is None for ic in idxs) and all(ic is None for ic in o_idxs)
                continue
            m = new_xyz.shape[1]
            assert _same(new_xyz[b:b + 1], o_xyz), f"level {i}, cloud {b}: centres"
            for j, (ic, oc) in enumerate(zip(idxs, o_idxs)):
                assert torch.equal(ic[0][b:b + 1], oc[0]), f"level {i} scale {j}, cloud {b}: neighbour lists"
                assert torch.equal(ic[1][b:b + 1], oc[1]), f"level {i} scale {j}, cloud {b}: counts"
                if ic[2] is not None:           # group offsets: an exclusive scan over the whole batch -> compare relative to the cloud
                    off = ic[2][b * m:(b + 1) * m + 1]
                    assert torch.equal(off - off[0], oc[2]), f"level {i} scale {j}, cloud {b}: group offsets"


def _no_pad_index(handle, lengths):
    new_xyz, idxs = handle["levels"][0]
    for ic in idxs:
        for b, n in enumerate(lengths):
            assert int(ic[0][b].max()) < n and int(ic[0][b].min()) >= 0


# ------------------------------------------------------------------------------------------------------- classification
@pytest.mark.parametrize("kind", ["ssg", "msg"])
def test_frozen_cls_ragged_equals_every_cloud_alone(dev, kind):
    from pointcloudlib_amd.inference import frozen
    net = _net("cls", kind, dev)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    lengths, N = CLS_LENGTHS, CLS_N
    B = len(lengths)
    fnet = frozen(net)
    runs = {}
    for how in FILLS:
        xyz, nrm = _clouds(dev, lengths, N, how)
        runs[how] = fnet.run(xyz, nrm, lengths=lengths)
    for how in FILLS[1:]:                                                # pad invariance of the whole forward
        assert all(_same(a, b) for a, b in zip(runs[how][0], runs["copies"][0])) and _same(runs[how][1], runs["copies"][1]), how
    feats, logits = runs["copies"]
    assert bool(torch.isfinite(logits).all())
    xyz, nrm = _clouds(dev, lengths, N, "nan")
    handle = net.precompute_sampling(xyz, lengths=lengths)
    assert handle["lengths"].dtype == torch.int32 and handle["lengths"].tolist() == lengths
    _no_pad_index(handle, lengths)
    singles = []
    for b, n in enumerate(lengths):
        xb, fb = xyz[b:b + 1, :n].contiguous(), nrm[b:b + 1, :n].contiguous()
        singles.append(net.precompute_sampling(xb))
        assert singles[-1]["lengths"] is None
        o_feats, o_logits = fnet.run(xb, fb)
        for i, (f, o) in enumerate(zip(feats, o_feats)):
            assert _same(f[b:b + 1], o), f"cloud {b} (n={n}): level {i} feature differs from the cloud alone"
        assert _same(logits[b:b + 1], o_logits), f"cloud {b} (n={n}): logits differ from the cloud alone"
    _assert_handles_equal(net, handle, singles)
    # the handle carries the lengths; the same lengths given twice are accepted, different ones are not
    h_feats, h_logits = fnet.run(xyz, nrm, sampling=handle)
    assert _same(h_logits, logits) and all(_same(a, b) for a, b in zip(h_feats, feats))
    assert _same(fnet(xyz, nrm, sampling=handle, lengths=torch.tensor(lengths, dtype=torch.int32, device=dev)), logits)
    with pytest.raises(ValueError, match="differ"):
        fnet(xyz, nrm, sampling=handle, lengths=[N] * B)
    # lengths = [N] * B is the dense frozen forward
    xd, fd = _clouds(dev, [N] * B, N, "copies")
    assert _same(fnet(xd, fd, lengths=[N] * B), fnet(xd, fd))
    # against dense padding (the test is not vacuous).  Copies are the benign filling for a max-pooling network -- a copy has its
    # original's coordinates and feature, so centres and group maxima come out the same although the index lists differ -- so the
    # dense forward is given pad points away from the cloud: FPS draws one as a centre and every short cloud's logits change
    xc, fc = _clouds(dev, lengths, N, "copies")
    for b, n in enumerate(lengths):
        xc[b, n:] = 3.0
    dense = fnet(xc, fc)
    assert all(not _same(dense[b], logits[b]) for b, n in enumerate(lengths) if n < N)
    assert _same(dense[0], logits[0])
    torch.cuda.synchronize()
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "frozen() modified the network"


# ---------------------------------------------------------------------------------------------------- part segmentation
@pytest.mark.parametrize("kind", ["ssg", "msg"])
def test_frozen_partseg_ragged_equals_every_cloud_alone(dev, kind):
    from pointcloudlib_amd.inference import frozen
    net = _net("seg", kind, dev)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    lengths, N = SEG_LENGTHS, SEG_N
    B = len(lengths)
    onehot = _onehot(dev, B)
    fnet = frozen(net)
    assert fnet.fp["fp1"][0] == "fused" and fnet.head_fused
    runs = {}
    for how in FILLS:
        xyz, nrm = _clouds(dev, lengths, N, how)
        runs[how] = fnet.run(xyz, nrm, onehot, lengths=lengths)
    for how in FILLS[1:]:
        assert all(_same(a, b) for a, b in zip(runs[how][0], runs["copies"][0])) and _same(runs[how][1], runs["copies"][1]), how
    levels, logits = runs["copies"]
    assert logits.shape == (B, net.part_num, N)
    names = ["sa1", "sa2", "sa3", "fp3", "fp2", "fp1"]
    xyz, nrm = _clouds(dev, lengths, N, "nan")
    handle = net.precompute_sampling(xyz, lengths=lengths)
    _no_pad_index(handle, lengths)
    singles = []
    for b, n in enumerate(lengths):
        xb, fb = xyz[b:b + 1, :n].contiguous(), nrm[b:b + 1, :n].contiguous()
        singles.append(net.precompute_sampling(xb))
        o_levels, o_logits = fnet.run(xb, fb, onehot[b:b + 1])
        for name, f, o in zip(names, levels, o_levels):
            rows = n if name == "fp1" else f.shape[1]
            assert _same(f[b:b + 1, :rows], o), f"cloud {b} (n={n}): {name} differs from the cloud alone"
        assert _same(logits[b:b + 1, :, :n], o_logits), f"cloud {b} (n={n}): logits differ from the cloud alone"
        # pad points: exact zeros (bit pattern 0: not -0.0, not NaN)
        assert not logits[b, :, n:].contiguous().view(torch.int32).any(), f"cloud {b}: logits of pad points"
        assert not levels[5][b, n:].contiguous().view(torch.int32).any(), f"cloud {b}: fp1 of pad points"
    _assert_handles_equal(net, handle, singles)
    assert _same(fnet(xyz, nrm, onehot, sampling=handle), logits)
    with pytest.raises(ValueError, match="differ"):
        fnet(xyz, nrm, onehot, sampling=handle, lengths=[N] * B)
    xd, fd = _clouds(dev, [N] * B, N, "copies")
    d_levels, d_logits = fnet.run(xd, fd, onehot)
    f_levels, f_logits = fnet.run(xd, fd, onehot, lengths=[N] * B)
    assert _same(d_logits, f_logits) and all(_same(a, b) for a, b in zip(d_levels, f_levels)), "lengths = [N] * B is not the dense forward"
    assert logits.stride() == d_logits.stride(), "not the network's layout / view"
    with pytest.raises(NotImplementedError, match="frozen"):
        net(xyz, nrm, onehot, sampling=handle)
    torch.cuda.synchronize()
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "frozen() modified the network"


def test_frozen_partseg_ragged_module_fallbacks(dev):
    """FP levels and heads without a fused kernel run eval-mode copies of their modules: the same contract."""
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.misc.ops import PointNetFeaturePropagation
    net = _net("seg", "ssg", dev)
    torch.manual_seed(5)
    net.fp1 = PointNetFeaturePropagation(128 + 22, [128, 96]).to(dev)                   # no kernel for 128/96: module FP1, module head
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    net.head1 = PointwiseMLP([96, 128], bias=True, slope=0.0, last_act=False).to(dev)
    _perturb(net, 9)
    lengths, N = SEG_LENGTHS, SEG_N
    B = len(lengths)
    onehot = _onehot(dev, B)
    fnet = frozen(net)
    assert fnet.fp["fp1"][0] == "module" and not fnet.head_fused
    outs = []
    for how in FILLS:
        xyz, nrm = _clouds(dev, lengths, N, how)
        outs.append(fnet.run(xyz, nrm, onehot, lengths=lengths))
    assert all(_same(o[1], outs[0][1]) and _same(o[0][5], outs[0][0][5]) for o in outs[1:]), "pad rows influence the result"
    levels, logits = outs[0]
    for b, n in enumerate(lengths):
        assert not logits[b, :, n:].contiguous().view(torch.int32).any() and not levels[5][b, n:].contiguous().view(torch.int32).any()
        assert bool(torch.isfinite(logits[b, :, :n]).all())
        # the module path is row-wise too (stats-free GEMMs in evaluation mode): the cloud alone, bit for bit
        o_levels, o_logits = fnet.run(xyz[b:b + 1, :n].contiguous(), nrm[b:b + 1, :n].contiguous(), onehot[b:b + 1])
        assert _same(levels[2][b:b + 1], o_levels[2]), f"cloud {b}: encoder"
        assert _same(levels[5][b:b + 1, :n], o_levels[5]), f"cloud {b} (n={n}): fp1 differs from the cloud alone"
        assert _same(logits[b:b + 1, :, :n], o_logits), f"cloud {b} (n={n}): logits differ from the cloud alone"


# -------------------------------------------------------------------------------------------- classifier training path
def test_cls_training_on_a_ragged_batch(dev):
    """One forward + backward of PointNet2_cls in training mode on a ragged batch: loss, every parameter gradient and the running
    statistics do not depend on the (finite) pad filling, and equal the run whose handle is assembled from per-cloud sampling."""
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.misc import ops
    from pointcloudlib_amd.train_utils import soft_cross_entropy_loss
    lengths, N = CLS_LENGTHS, CLS_N
    B = len(lengths)
    lab = torch.from_numpy(synth.labels(B, 40, 3)).to(dev)
    base = _net("cls", "ssg", dev)
    base.fc_layer[6].p = 0.0
    state = {k: v.clone() for k, v in base.state_dict().items()}

    def step(how, assembled=False):
        net = _net("cls", "ssg", dev)
        net.fc_layer[6].p = 0.0
        net.load_state_dict(state)
        net.train()
        xyz, nrm = _clouds(dev, lengths, N, how)
        sampling = None
        if assembled:                                                  # the handle of the batch from B calls on the clouds alone
            per = [net.precompute_sampling(xyz[b:b + 1, :n].contiguous())["levels"] for b, n in enumerate(lengths)]
            levels = []
            for i in range(len(per[0])):
                if per[0][i][0] is None:
                    levels.append((None, [None]))
                    continue
                new_xyz = torch.cat([p[i][0] for p in per])
                idx = torch.cat([p[i][1][0][0] for p in per])
                cnt = torch.cat([p[i][1][0][1] for p in per])
                levels.append((new_xyz, [(idx, cnt, ops.group_offsets(cnt))]))
            sampling = {"levels": levels}
            out = net(xyz, nrm, sampling=sampling)
        else:
            out = net(xyz, nrm, lengths=lengths)
        loss = soft_cross_entropy_loss(out, lab)
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in net.named_parameters()}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        return loss.detach().clone(), grads, {k: v.clone() for k, v in net.state_dict().items()}

    l0, g0, s0 = step("zeros")
    for how, assembled in (("copies", False), ("zeros", True)):
        l1, g1, s1 = step(how, assembled)
        what = f"pads = {how}" + (", handle assembled from per-cloud sampling" if assembled else "")
        assert _same(l0, l1), f"loss ({what})"
        for k in g0:
            assert _same(g0[k], g1[k]), f"gradient of {k} ({what})"
        for k in s0:
            assert torch.equal(s0[k], s1[k]), f"state {k} ({what})"
    moved = [k for k in s0 if "running" in k and not torch.equal(s0[k], state[k])]
    assert moved, "no running statistic moved: the step trained nothing"
