"""Frozen inference for PointConv part segmentation on the GPU (pointcloudlib_amd/inference.py: FrozenPointConvPartseg;
csrc/infer_pointconv.hip through pcl_pointconv_seg_level_infer_f32): the level kernel's new shapes through the C ABI -- against the
fp64 restatement of tests/pointconv_infer_ref.py, bit for bit on exactly representable data, group by group -- then the whole
network, the contract of the evaluator, the fallback for a level without a kernel and the memory a forward needs.

Yardstick (tests/test_inference_gpu.py): the fused path may be no further from the fp64 restatement than the existing path on the
same inputs (max |difference|), x 1.25, plus 1e-6.  The existing path of the level kernel is the composite ``index_points`` +
eval-mode ``PointwiseMLP`` copies + ``pointconv_contract``; of the network, ``net.eval()`` under ``no_grad``."""
import copy
import functools

import pytest
import torch

import pointconv_infer_ref as R
import pointconv_partseg_infer_ref as RS
from pointconv_partseg_infer_ref import EXACT_SEED, MANY, SHAPES
from test_inference_gpu import _err, _perturb
from test_inference_pointconv_gpu import _alive, _composite, _frozen_stacks
from test_inference_pointconv_gpu import _level_call as _cls_level_call

pytestmark = pytest.mark.gpu

NEW = sorted(SHAPES)
STOCK = ["fused", "fused", "fused", "module", "module", "fused", "fused", "fused"]


_level_call = functools.partial(R.level_call, entry="pcl_pointconv_seg_level_infer_f32")


def _case_args(c):
    return c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"]


# ------------------------------------------------------------------------------------------------- 1. against fp64
@functools.lru_cache(maxsize=None)
def _module_case(name):
    """Perturbed eval-mode modules of one level and random inputs (on the device), shared by the tests that read them."""
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.misc.pointconv_utils import DensityNet, WeightNet
    dev = torch.device("cuda:0")
    ns, widths, D, B, N, m = SHAPES[name]
    seed = 300 + NEW.index(name)
    torch.manual_seed(seed)
    mods = torch.nn.ModuleDict({"mlp": PointwiseMLP([3 + D] + widths, bias=True), "wn": WeightNet(3, 16), "dn": DensityNet()}).to(dev)
    _alive(_perturb(mods, seed + 7)).eval()
    g = torch.Generator().manual_seed(seed)
    case = {"xyz": torch.rand(B, N, 3, generator=g), "new_xyz": torch.rand(B, m, 3, generator=g),
            "points": None if D == 0 else torch.randn(B, N, D, generator=g), "density": 3 * torch.rand(B, N, generator=g).clamp(min=1e-3),
            "idx": R.knn_lists(B, N, m, ns, g)}
    return mods, {k: None if v is None else v.to(dev) for k, v in case.items()}


@pytest.mark.parametrize("name", NEW)
def test_level_kernel_against_fp64(dev, name):
    mods, c = _module_case(name)
    feat, nets = _frozen_stacks(mods)
    got = _level_call(dev, feat, nets, *_case_args(c))
    again = _level_call(dev, feat, nets, *_case_args(c))
    assert torch.equal(got, again), "two calls differ"
    want_eval = _composite(mods, c)
    ref = R.level(R.stack_of(mods["mlp"]), R.stack_of(mods["wn"].mlp), R.stack_of(mods["dn"].mlp), *_case_args(c))
    assert got.shape == ref.shape == (SHAPES[name][3], SHAPES[name][5], 16 * SHAPES[name][1][-1])
    assert float((ref != 0).double().mean()) > 0.3, "a trivial level"
    e_fused, e_eval = _err(got, ref), _err(want_eval, ref)
    print(f"{name}: fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64 (largest |value| {float(ref.abs().max()):.3e})")
    assert e_fused <= 1.25 * e_eval + 1e-6, f"fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64"


# ------------------------------------------------------------------------------------------------- 2. exactly representable data
@pytest.mark.parametrize("name", NEW)
def test_level_kernel_exact_data_bit_for_bit(dev, name):
    c = R.exact_case(*SHAPES[name], EXACT_SEED)
    want = R.level(c["feat"], c["wn"], c["dn"], *_case_args(c))
    got = _level_call(dev, c["feat"], R.pack_nets(c["wn"], c["dn"], 400), *_case_args(c))
    assert torch.equal(got.cpu(), want.float()), f"{int((got.cpu() != want.float()).sum())} of {want.numel()} outputs differ"


# ------------------------------------------------------------------------------------------------- 3. group independence, ns = 16
def test_level_kernel_groups_are_independent_at_16_neighbours(dev):
    mods, c = _module_case("in2")
    feat, nets = _frozen_stacks(mods)
    full = _level_call(dev, feat, nets, *_case_args(c))
    one = _level_call(dev, feat, nets, c["xyz"][1:2], c["new_xyz"][1:2], c["points"][1:2], c["idx"][1:2], c["density"][1:2])
    assert torch.equal(full[1:2], one), "cloud 1 alone differs from cloud 1 in the batch"
    perm = [2, 1, 0]                                                       # clouds 0 and 2 swapped: every group moves
    swapped = _level_call(dev, feat, nets, c["xyz"][perm], c["new_xyz"][perm], c["points"][perm], c["idx"][perm], c["density"][perm])
    assert torch.equal(swapped, full[perm])
    gp = [0, 3, 2, 1, 4]                                                   # two groups of one cloud swapped (centres and lists together)
    moved = _level_call(dev, feat, nets, c["xyz"], c["new_xyz"][:, gp], c["points"], c["idx"][:, gp], c["density"])
    assert torch.equal(moved, full[:, gp])
    # the last tile with 1, 2 and 3 live groups of 4: the first m = 5, 6, 7 groups of ONE cloud against the same groups in a launch
    # of eight (two full tiles)
    g = torch.Generator().manual_seed(5)
    ns, N = SHAPES["in2"][0], SHAPES["in2"][4]
    more_xyz = torch.rand(1, 8, 3, generator=g).to(dev)
    more_idx = R.knn_lists(1, N, 8, ns, g).to(dev)
    eight = _level_call(dev, feat, nets, c["xyz"][:1], more_xyz, c["points"][:1], more_idx, c["density"][:1])
    assert eight[0].unique(dim=0).shape[0] == 8, "the eight groups are to differ"
    for m in (5, 6, 7):
        part = _level_call(dev, feat, nets, c["xyz"][:1], more_xyz[:, :m], c["points"][:1], more_idx[:, :m], c["density"][:1])
        assert torch.equal(part, eight[:, :m]), f"m = {m}: {m - 4} live group(s) in the last tile"


# ------------------------------------------------------------------------------------------------- 4. several tiles per workgroup
@pytest.mark.parametrize("name", sorted(MANY))
def test_level_kernel_many_tiles_per_workgroup(dev, name):
    """A launch whose workgroups walk several tiles on the exactly representable data: every cloud bit for bit a B = 1 launch of that
    cloud, whose workgroups own fewer tiles, and the first and last 100 groups bit for bit the fp64 restatement."""
    from pointcloudlib_amd import _lib
    ns, widths, D, B, N, m = MANY[name]
    gpt = 64 // ns
    gt_all, gt_one = (_lib.lib().pcl_pointconv_seg_level_infer_group_tile(ns, G) for G in (B * m, m))
    assert gt_all >= 2 * gpt and gt_all > gt_one >= gpt, f"workgroups own {gt_all} groups in the large launch, {gt_one} in the B = 1 launch"
    assert (B * m) % gpt != 0, "the last tile is to be partly filled"
    c = R.exact_case(ns, widths, D, B, N, m, EXACT_SEED)
    nets = R.pack_nets(c["wn"], c["dn"], 400)
    pts = lambda b: None if c["points"] is None else c["points"][b]
    full = _level_call(dev, c["feat"], nets, *_case_args(c))
    assert bool(torch.isfinite(full).all())
    for b in range(B):
        bs = slice(b, b + 1)
        one = _level_call(dev, c["feat"], nets, c["xyz"][bs], c["new_xyz"][bs], pts(bs), c["idx"][bs], c["density"][bs])
        assert torch.equal(full[bs], one), f"cloud {b} alone differs from cloud {b} in the batch"
    for b, sl in ((0, slice(0, 100)), (B - 1, slice(m - 100, m))):
        bs = slice(b, b + 1)
        audit = []
        want = R.level(c["feat"], c["wn"], c["dn"], c["xyz"][bs], c["new_xyz"][bs, sl], pts(bs), c["idx"][bs, sl], c["density"][bs], audit=audit)
        assert max(audit) < 2.0 ** 24 and float((want != 0).double().mean()) > 0.3       # exact in any order, and no trivial result
        assert torch.equal(full[bs, sl].cpu(), want.float()), f"cloud {b}, groups {sl}: differs from fp64"


# ------------------------------------------------------------------------------------------------- 5. the two shared shapes
@pytest.mark.parametrize("ns", [32, 64])
def test_shared_shapes_give_the_bits_of_the_cls_entry_point(dev, ns):
    from test_inference_pointconv_gpu import _module_case as cls_case
    mods, c = cls_case(ns)
    feat, nets = _frozen_stacks(mods)
    want = _cls_level_call(dev, feat, nets, *_case_args(c))
    got = _level_call(dev, feat, nets, *_case_args(c))
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------- 6.-9. the network
@functools.lru_cache(maxsize=None)
def _net(seed=0):
    from pointcloudlib_amd.networks.seg.pointconv_partseg import PointConvDensity_partseg
    torch.manual_seed(seed)
    return _alive(_perturb(PointConvDensity_partseg().to("cuda:0"), seed + 1))


def _clouds(dev, B, N=2048, seed=0):
    from pointcloudlib_amd import synth
    return torch.from_numpy(synth.gauss_ball(B, N, seed)).to(dev).contiguous()                              # [B,N,3]


def _start_idx(dev, B):
    """Eight FPS starts in call order: each below its level's point count (2048, 1024, 256, 64 down; 64, 256, 1024, 2048 up)."""
    g = torch.Generator().manual_seed(11)
    return [torch.randint(0, n, (B,), generator=g, dtype=torch.int32).to(dev) for n in (2048, 1024, 256, 64, 64, 256, 1024, 2048)]


def _eval_run(net, x, sampling):
    """The existing evaluation path (net.eval() + no_grad) on a copy, level by level -> (channel-last outputs, logits)."""
    ev = copy.deepcopy(net).eval()
    lv = sampling["levels"]
    with torch.no_grad():
        x0 = x.permute(0, 2, 1).contiguous()
        x1, p1 = ev.sa0(x0, None, sampling=lv[0])
        x2, p2 = ev.sa1(x1, p1, sampling=lv[1])
        x3, p3 = ev.sa2(x2, p2, sampling=lv[2])
        x4, p4 = ev.sa3(x3, p3, sampling=lv[3])
        q3 = ev.in0(x3, x4, p3, p4, sampling=lv[4])
        q2 = ev.in1(x2, x3, p2, q3, sampling=lv[5])
        q1 = ev.in2(x1, x2, p1, q2, sampling=lv[6])
        q0 = ev.in3(x0, x1, x0, q1, sampling=lv[7])
        feats = [p.permute(0, 2, 1) for p in (p1, p2, p3, p4, q3, q2, q1, q0)]
        return feats, ev(x, sampling=sampling)


def _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, what):
    """-> the larger of the two measured logit errors."""
    assert len(feats) == len(ev_feats) == len(ref_feats) == 8
    for name, f, e, r in zip(RS.LEVELS, feats, ev_feats, ref_feats):
        assert f.shape == e.shape == r.shape, (name, f.shape, e.shape, r.shape)
        ef, ee = _err(f, r), _err(e, r)
        print(f"{what} {name}: frozen {ef:.3e} vs eval {ee:.3e} from fp64 (largest |value| {float(r.abs().max()):.3e})")
        assert ef <= 1.25 * ee + 1e-6, f"{what} {name}: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    assert logits.shape == ev_logits.shape == ref_logits.shape
    ef, ee = _err(logits, ref_logits), _err(ev_logits, ref_logits)
    print(f"{what} logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64")
    assert ef <= 1.25 * ee + 1e-6, f"{what} logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    return max(ef, ee)


def test_frozen_partseg_against_fp64(dev):
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    net = _net()
    B, N = 2, 2048
    x = _clouds(dev, B, N)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    assert len(samp["levels"]) == 8 and samp["event"] is None
    fnet = FrozenPointConvPartseg(net)
    assert fnet.levels == STOCK
    feats, logits = fnet.run(x, sampling=samp)
    ev_feats, ev_logits = _eval_run(net, x, samp)
    ref_feats, ref_logits = RS.network(net, x, samp["levels"])
    torch.cuda.synchronize()
    assert logits.shape == (B, N, 50)
    assert [tuple(f.shape) for f in feats] == [(B, 1024, 64), (B, 256, 128), (B, 64, 256), (B, 36, 512), (B, 64, 512), (B, 256, 256),
                                               (B, 1024, 128), (B, N, 128)]
    for name, r in zip(RS.LEVELS, ref_feats):
        share = float((r != 0).double().mean())
        assert share > 0.2, f"{name}: a trivial level ({share:.2f} nonzero)"
    err = _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, "partseg")
    # the per-point argmax: agreement on at least the share of points whose fp64 top-2 margin exceeds the larger measured error; and
    # a point whose margin exceeds it twice over cannot change its class in either path (each logit moves by at most that error)
    top2 = ref_logits.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    same = logits.argmax(-1) == ev_logits.argmax(-1)
    share, agree = float((margin > err).double().mean()), float(same.double().mean())
    print(f"argmax: agrees with net.eval() on {agree:.5f} of the points; {share:.5f} have an fp64 margin above {err:.3e}")
    assert agree >= share
    assert bool(same[margin > 2 * err].all())


def test_frozen_partseg_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    net = copy.deepcopy(_net()).train()
    B, N = 2, 2048
    x = _clouds(dev, B, N, seed=3)
    start = _start_idx(dev, B)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = FrozenPointConvPartseg(net)
    out_inline = fnet(x, start_idx=start)
    out_handle = fnet(x, sampling=net.precompute_sampling(x, start))
    torch.cuda.synchronize()
    assert out_inline.shape == (B, N, 50)
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(out_inline, out_handle), "a precomputed sampling handle changes the output"
    assert torch.equal(fnet(x, cls_label=torch.zeros(B, 16, device=dev), start_idx=start), out_inline), "cls_label is unused"
    with torch.no_grad():
        net.in2.mlp.weights[1].mul_(1.5)
        net.fc3.bias.add_(0.25)
    stale = fnet(x, start_idx=start)
    fresh = fnet.refresh()(x, start_idx=start)
    torch.cuda.synchronize()
    assert torch.equal(stale, out_inline)
    assert not torch.equal(fresh, out_inline)
    assert torch.equal(fresh, FrozenPointConvPartseg(net)(x, start_idx=start))
    with pytest.raises(ValueError, match=r"\[B,N,3\]"):
        fnet(x.permute(0, 2, 1))


def test_default_forward_is_unchanged_by_the_sampling_argument(dev):
    """``forward(sampling=None)`` draws its FPS starts from the same generator in the same order as ``precompute_sampling``: with
    the generator reset, the plain forward and the forward on a handle drawn the same way give the same bits."""
    ev = copy.deepcopy(_net()).eval()
    x = _clouds(dev, 1, 2048, seed=8)
    with torch.no_grad():
        torch.manual_seed(21)
        plain = ev(x)
        torch.manual_seed(21)
        handled = ev(x, sampling=ev.precompute_sampling(x))
    assert torch.equal(plain, handled)


def test_frozen_partseg_falls_back_for_other_widths(dev):
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    from pointcloudlib_amd.misc.pointconv_utils import PointConvDensitySetInterpolation
    net = copy.deepcopy(_net())
    torch.manual_seed(5)
    net.in2 = PointConvDensitySetInterpolation(nsample=16, in_channel=256 + 3, mlp=[96, 96], bandwidth=0.2).to(dev)
    net.in3 = PointConvDensitySetInterpolation(nsample=16, in_channel=96 + 3, mlp=[128, 128, 128], bandwidth=0.1).to(dev)
    _alive(_perturb(net, 9))
    B, N = 2, 2048
    x = _clouds(dev, B, N, seed=4)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    fnet = FrozenPointConvPartseg(net)
    assert fnet.levels == STOCK[:6] + ["module", "fused"]
    feats, logits = fnet.run(x, sampling=samp)
    ev_feats, ev_logits = _eval_run(net, x, samp)
    ref_feats, ref_logits = RS.network(net, x, samp["levels"])
    torch.cuda.synchronize()
    assert feats[6].shape == (B, 1024, 96)
    _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, "fallback")
    with torch.no_grad():
        net.in2.mlp.weights[1].mul_(1.5)
    assert torch.equal(fnet(x, sampling=samp), logits)
    fresh = fnet.refresh()(x, sampling=samp)
    assert not torch.equal(fresh, logits)
    assert torch.equal(fresh, FrozenPointConvPartseg(net)(x, sampling=samp))


def test_frozen_partseg_forward_memory(dev):
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    net = _net()
    B, N = 4, 2048
    x = _clouds(dev, B, N, seed=6)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    fnet = FrozenPointConvPartseg(net)
    ev = copy.deepcopy(net).eval()

    def peak(fn):
        fn()                                       # warm-up: one-time allocations (constants, plans)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        assert out.shape == (B, N, 50)
        del out
        return torch.cuda.max_memory_allocated() - base

    with torch.no_grad():
        p_frozen, p_eval = peak(lambda: fnet(x, sampling=samp)), peak(lambda: ev(x, sampling=samp))
    # what a frozen forward may hold at once, in floats: the widest moment is in3 -- its contraction output [B*N, 16 * 128] (the only
    # large intermediate), its Uf [B*N, 128] and the interpolated features [B*N, 128] -- and the inputs; plus 25 % (the level
    # outputs kept for run(), the Linear's [B*N, 128] rows)
    contraction = B * N * 16 * 128
    uf = interpolated = B * N * 128
    inputs = B * N * 3
    bound = 1.25 * 4 * (contraction + uf + interpolated + inputs)
    grouped = 4 * B * N * 16 * 128                 # one [B, N, 16, 128] activation of in3 under net.eval()
    print(f"peak of a forward: frozen +{p_frozen / 2**20:.1f} MiB, net.eval() +{p_eval / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB, "
          f"one grouped in3 tensor {grouped / 2**20:.1f} MiB")
    assert p_frozen < p_eval
    assert p_frozen <= bound, f"frozen forward peak +{p_frozen / 2**20:.1f} MiB > bound {bound / 2**20:.1f} MiB"
