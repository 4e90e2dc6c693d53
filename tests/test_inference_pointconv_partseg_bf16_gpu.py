"""bf16 frozen PointConv part segmentation on the GPU (``FrozenPointConvPartseg(net, precision="bf16")``,
pcl_pointconv_seg_level_infer_bf16_f32: csrc/infer_pointconv_seg_bf16.hip): the five new kernels through the C ABI -- bit for bit
against the fp64 restatement and against the fp32 entry on the exactly representable data of
tests/test_inference_pointconv_partseg_gpu.py (tests/test_inference_pointconv_partseg_bf16_cpu.py holds that every rounded
activation and weight of those data is a bf16 number), within the derived bound of tests/pointconv_bf16_bound.py on random data,
group by group, many tiles per workgroup -- then the network, the contract of the evaluator and the memory of a forward.

Shapes, seeds, modules and the network are those of tests/test_inference_pointconv_partseg_gpu.py (imported, so the cached cases
are shared)."""
import copy
import functools

import pytest
import torch

import pointconv_bf16_bound as PB
import pointconv_infer_ref as R
from pointconv_partseg_bf16_cases import BF16, CLS_BF16, FP32, LARGE, NEW, case_args
from pointconv_partseg_infer_ref import EXACT_SEED, SHAPES
from test_inference_pointconv_gpu import _frozen_stacks
from test_inference_pointconv_partseg_gpu import STOCK, _clouds, _module_case, _net, _start_idx

pytestmark = pytest.mark.gpu


_level_call = functools.partial(R.level_call, entry=BF16)


# ------------------------------------------------------------------------------------------------- 1. exactly representable data
@pytest.mark.parametrize("name", NEW)
def test_bf16_level_kernel_exact_data_bit_for_bit(dev, name):
    c = R.exact_case(*SHAPES[name], EXACT_SEED)
    nets = R.pack_nets(c["wn"], c["dn"], 400)
    want = R.level(c["feat"], c["wn"], c["dn"], *case_args(c))
    got = _level_call(dev, c["feat"], nets, *case_args(c))
    assert got.shape == (SHAPES[name][3], SHAPES[name][5], 16 * SHAPES[name][1][-1])
    assert torch.equal(got.cpu(), want.float()), f"{int((got.cpu() != want.float()).sum())} of {want.numel()} outputs differ from fp64"
    assert torch.equal(got, _level_call(dev, c["feat"], nets, *case_args(c), entry=FP32)), "differs from the fp32 entry"


# ------------------------------------------------------------------------------------------------- 2. random data within the bound
@pytest.mark.parametrize("name", NEW)
def test_bf16_level_kernel_within_the_bound(dev, name):
    """MI355X, bf16 entry (fp32 entry) x bound: sa0 0.0748 (0.000092), sa2 0.0180 (0.000031), in1 0.1023 (0.000587), in2 0.1912
    (0.000216), in3 0.0241 (0.000103)."""
    mods, c = _module_case(name)
    feat, nets = _frozen_stacks(mods)
    got = _level_call(dev, feat, nets, *case_args(c))
    assert torch.equal(got, _level_call(dev, feat, nets, *case_args(c))), "two calls differ"
    assert bool(torch.isfinite(got).all())
    ref, bound = PB.level_ref_and_bound(feat, nets, *case_args(c))
    assert float((ref != 0).double().mean()) > 0.3, "a trivial level"
    assert bool(torch.isfinite(bound).all()) and bool((bound[ref != 0] > 0).all())
    ratio = PB.worst_ratio(got, ref, bound)
    ratio32 = PB.worst_ratio(_level_call(dev, feat, nets, *case_args(c), entry=FP32), ref, bound)
    print(f"{name}: bf16 entry {ratio:.4f} x bound, fp32 entry {ratio32:.6f} x bound (largest |value| {float(ref.abs().max()):.3e}, "
          f"largest bf16 error {float((got.double() - ref).abs().max()):.3e})")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------- 3. group independence
@pytest.mark.parametrize("name", ["in2", "sa2"])
def test_bf16_level_kernel_groups_are_independent(dev, name):
    """ns = 16 (in2: four groups per tile) and ns = 32 (sa2: two), both with a Uf table the groups share."""
    mods, c = _module_case(name)
    feat, nets = _frozen_stacks(mods)
    full = _level_call(dev, feat, nets, *case_args(c))
    one = _level_call(dev, feat, nets, c["xyz"][1:2], c["new_xyz"][1:2], c["points"][1:2], c["idx"][1:2], c["density"][1:2])
    assert torch.equal(full[1:2], one), "cloud 1 alone differs from cloud 1 in the batch"
    perm = [2, 1, 0]                                                       # clouds 0 and 2 swapped: every group moves
    swapped = _level_call(dev, feat, nets, c["xyz"][perm], c["new_xyz"][perm], c["points"][perm], c["idx"][perm], c["density"][perm])
    assert torch.equal(swapped, full[perm])
    gp = [0, 3, 2, 1, 4]                                                   # two groups of one cloud swapped (centres and lists together)
    moved = _level_call(dev, feat, nets, c["xyz"], c["new_xyz"][:, gp], c["points"], c["idx"][:, gp], c["density"])
    assert torch.equal(moved, full[:, gp])
    # a partly filled last tile: the first m = 5, 6, 7 groups of ONE cloud against the same groups in a launch of eight (full tiles)
    g = torch.Generator().manual_seed(5)
    ns, N = SHAPES[name][0], SHAPES[name][4]
    more_xyz = torch.rand(1, 8, 3, generator=g).to(dev)
    more_idx = R.knn_lists(1, N, 8, ns, g).to(dev)
    eight = _level_call(dev, feat, nets, c["xyz"][:1], more_xyz, c["points"][:1], more_idx, c["density"][:1])
    assert eight[0].unique(dim=0).shape[0] == 8, "the eight groups are to differ"
    for m in (5, 6, 7):
        part = _level_call(dev, feat, nets, c["xyz"][:1], more_xyz[:, :m], c["points"][:1], more_idx[:, :m], c["density"][:1])
        assert torch.equal(part, eight[:, :m]), f"m = {m}: {m % (64 // ns)} live group(s) in the last tile"


# ------------------------------------------------------------------------------------------------- 4. several tiles per workgroup
@pytest.mark.parametrize("name", sorted(LARGE))
def test_bf16_level_kernel_many_tiles_per_workgroup(dev, name):
    """As tests/test_inference_pointconv_partseg_gpu.py::test_level_kernel_many_tiles_per_workgroup, on the bf16 entry: 8195 groups
    in one launch on the exactly representable data; every cloud bit for bit its B = 1 launch, whose workgroups own fewer tiles,
    and the first and last 100 groups bit for bit the fp64 restatement.  The configuration (many tiles per workgroup, two workgroups
    per compute unit) in which layer 1's packed chain lost steps in the 128/128/256 kernel of ns = 64."""
    from pointcloudlib_amd import _lib
    ns, widths, D, B, N, m = LARGE[name]
    gpt = 64 // ns
    gt_all, gt_one = (_lib.lib().pcl_pointconv_seg_level_infer_group_tile(ns, G) for G in (B * m, m))
    assert gt_all >= 2 * gpt and gt_all > gt_one >= gpt, f"workgroups own {gt_all} groups in the large launch, {gt_one} in the B = 1 launch"
    assert (B * m) % gpt != 0, "the last tile is to be partly filled"
    c = R.exact_case(ns, widths, D, B, N, m, EXACT_SEED)
    nets = R.pack_nets(c["wn"], c["dn"], 400)
    pts = lambda b: None if c["points"] is None else c["points"][b]
    full = _level_call(dev, c["feat"], nets, *case_args(c))
    assert bool(torch.isfinite(full).all())
    for b in range(B):
        bs = slice(b, b + 1)
        one = _level_call(dev, c["feat"], nets, c["xyz"][bs], c["new_xyz"][bs], pts(bs), c["idx"][bs], c["density"][bs])
        differ = (full[bs] != one).any(dim=-1).sum()
        assert torch.equal(full[bs], one), f"cloud {b} alone differs from cloud {b} in the batch in {int(differ)} of {m} groups"
    for b, sl in ((0, slice(0, 100)), (B - 1, slice(m - 100, m))):
        bs = slice(b, b + 1)
        audit = []
        want = R.level(c["feat"], c["wn"], c["dn"], c["xyz"][bs], c["new_xyz"][bs, sl], pts(bs), c["idx"][bs, sl], c["density"][bs], audit=audit)
        assert max(audit) < 2.0 ** 24 and float((want != 0).double().mean()) > 0.3       # exact in any order, and no trivial result
        assert torch.equal(full[bs, sl].cpu(), want.float()), f"cloud {b}, groups {sl}: differs from fp64"


# ------------------------------------------------------------------------------------------------- 5. the two shared shapes
@pytest.mark.parametrize("ns", [32, 64])
def test_shared_shapes_give_the_bits_of_the_cls_bf16_entry_point(dev, ns):
    from test_inference_pointconv_gpu import _module_case as cls_case
    mods, c = cls_case(ns)
    feat, nets = _frozen_stacks(mods)
    want = _level_call(dev, feat, nets, *case_args(c), entry=CLS_BF16)
    got = _level_call(dev, feat, nets, *case_args(c))
    assert torch.equal(got, want)
    assert not torch.equal(got, _level_call(dev, feat, nets, *case_args(c), entry=FP32)), "the bf16 entry ran the fp32 kernel"


# ------------------------------------------------------------------------------------------------- 6. the network
def test_bf16_frozen_partseg_network(dev):
    """MI355X: contractions sa0 0.0780, sa1 0.0302, sa2 0.0265, in1 0.1474, in2 0.1961, in3 0.0350 x bound; logits max |bf16 - fp32|
    9.8e-6 at a largest |logit| of 0.19, per-point top-1 agreement 1.0 (printed, not asserted: near-tied points of a perturbed,
    untrained net make it no threshold)."""
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    from pointcloudlib_amd.misc.ops import three_interpolate
    net = copy.deepcopy(_net()).train()
    B, N = 2, 2048
    x = _clouds(dev, B, N)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    levels = samp["levels"]
    before = {k: v.clone() for k, v in net.state_dict().items()}
    f32, f16 = FrozenPointConvPartseg(net), FrozenPointConvPartseg(net, precision="bf16")
    assert f16.levels == f32.levels == STOCK
    assert all(type(a[1]) is type(b[1]) for a, b in zip(f16.plans, f32.plans))
    assert all(type(a[1].linear) is type(b[1].linear) for a, b in zip(f16.plans, f32.plans) if a[0] == "fused")
    assert type(f16.fc1) is type(f32.fc1) and f16.W3.dtype == torch.float32
    feats, logits = f16.run(x, sampling=samp)
    feats_again, logits_again = f16.run(x, sampling=samp)
    torch.cuda.synchronize()
    assert logits.shape == (B, N, 50) and logits.dtype == torch.float32 and bool(torch.isfinite(logits).all())
    assert torch.equal(logits, logits_again) and all(torch.equal(a, b) for a, b in zip(feats, feats_again)), "two runs differ"
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    # each fused launch on the bf16 run's own inputs, against the restatement of the constants it was given
    pts = [x.contiguous()] + [levels[i][0].contiguous() for i in range(4)]
    n_fused = 0
    for i, (kind, plan) in enumerate(f16.plans):
        if kind != "fused":
            continue
        if i < 4:
            new_xyz, ((idx, density),) = levels[i]
            xyz1, points = pts[i], None if i == 0 else feats[i - 1]
        else:                                                              # an interpolation level, on its own three_interpolate output
            lv = levels[i]
            new_xyz, idx, density = lv["new_xyz"], lv["idx"], lv["density"]
            xyz1, points = pts[7 - i], three_interpolate(feats[i - 1].contiguous(), lv["idx3"], lv["w3"])
        new_xyz, idx, density = new_xyz.contiguous(), idx.contiguous(), density.contiguous()
        S = idx.shape[1]
        got = plan.contract(xyz1, new_xyz, points, idx, density).view(B, S, -1)
        feat = [(plan.W0, plan.scales[0], plan.shifts[0])] + [(plan.Ws[l], plan.scales[l], plan.shifts[l]) for l in range(1, plan.L)]
        ref, bound = PB.level_ref_and_bound(feat, plan.nets, xyz1, new_xyz, points, idx, density, plan.slope)
        # no trivial level.  A contraction column c*16 + m is zero wherever channel c or WeightNet output m is dead under the
        # perturbed constants (the fp32 file's 0.2 is for the outputs behind the Linear, which mixes the columns)
        share = float((ref != 0).double().mean())
        assert share > 0.05 and float(ref.abs().max()) > 0.1, f"level {i}: a trivial level ({share:.3f} nonzero)"
        ratio = PB.worst_ratio(got, ref, bound)
        print(f"level {i} (ns {idx.shape[2]}, L {plan.L}) contraction: {ratio:.4f} x bound ({share:.3f} nonzero, largest |value| {float(ref.abs().max()):.3e}, "
              f"largest error {float((got.double() - ref).abs().max()):.3e})")
        assert ratio <= 1.0
        assert torch.equal(plan.linear.run(got.view(B * S, -1)).view(B, S, -1), feats[i]), f"level {i}: not the output of the run"
        del ref, bound
        n_fused += 1
    assert n_fused == 6
    f32_feats, l32 = f32.run(x, sampling=samp)
    same = float((logits.argmax(-1) == l32.argmax(-1)).float().mean())
    print(f"logits: max |bf16 - fp32| {float((logits - l32).abs().max()):.3e} (largest |logit| {float(l32.abs().max()):.3e}), "
          f"per-point top-1 agreement {same:.5f}")
    # the two module levels run the same code under either precision (the plans' types, above); their inputs differ by bf16 roundings
    for i in (3, 4):
        print(f"level {i} (module): max |bf16 run - fp32 run| {float((feats[i] - f32_feats[i]).abs().max()):.3e}")
        assert feats[i].shape == f32_feats[i].shape and feats[i].dtype == torch.float32
    with torch.no_grad():
        net.in2.mlp.weights[1].mul_(1.5)
    assert torch.equal(f16(x, sampling=samp), logits)                      # a snapshot: stale until refresh()
    fresh = f16.refresh()(x, sampling=samp)
    assert f16.precision == "bf16" and not torch.equal(fresh, logits)
    assert torch.equal(fresh, FrozenPointConvPartseg(net, precision="bf16")(x, sampling=samp))


# ------------------------------------------------------------------------------------------------- 7. the contract
def test_bf16_frozen_partseg_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    net = _net()
    fnet = FrozenPointConvPartseg(net, precision="bf16")
    assert fnet.precision == "bf16" and FrozenPointConvPartseg(net).precision == "fp32"
    B = 2
    x = _clouds(dev, B, 2048, seed=3)
    for bad in (x.cpu(), x.double()):
        with pytest.raises(TypeError, match="float32 tensor on the GPU"):
            fnet(bad)
    # a bf16 weight 8 bytes behind a 16-byte boundary: the wrapper holds the entry point's precondition
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    plan = fnet.plans[0][1]
    new_xyz, ((idx, density),) = samp["levels"][0]
    args = (x.contiguous(), new_xyz.contiguous(), None, idx.contiguous(), density.contiguous())
    good = plan.contract(*args)
    w = plan.Ws_bf16[2]
    base = torch.empty(w.numel() + 8, dtype=torch.bfloat16, device=dev)
    off = base[4:4 + w.numel()].view_as(w)
    off.copy_(w)
    assert off.data_ptr() % 16 == 8
    plan.Ws_bf16[2] = off
    with pytest.raises(ValueError, match="pcl_pointconv_seg_level_infer_bf16_f32.*16-byte aligned"):
        plan.contract(*args)
    plan.Ws_bf16[2] = w
    assert torch.equal(plan.contract(*args), good)


def test_bf16_frozen_partseg_falls_back_for_other_widths(dev):
    """``levels`` does not depend on the precision: a level without a kernel is ``"module"`` under bf16 too, and the forward runs."""
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    from pointcloudlib_amd.misc.pointconv_utils import PointConvDensitySetInterpolation
    from test_inference_pointconv_gpu import _alive
    from test_inference_gpu import _perturb
    net = copy.deepcopy(_net())
    torch.manual_seed(5)
    net.in2 = PointConvDensitySetInterpolation(nsample=16, in_channel=256 + 3, mlp=[96, 96], bandwidth=0.2).to(dev)
    net.in3 = PointConvDensitySetInterpolation(nsample=16, in_channel=96 + 3, mlp=[128, 128, 128], bandwidth=0.1).to(dev)
    _alive(_perturb(net, 9))
    B, N = 2, 2048
    x = _clouds(dev, B, N, seed=4)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    f32, f16 = FrozenPointConvPartseg(net), FrozenPointConvPartseg(net, precision="bf16")
    assert f16.levels == f32.levels == STOCK[:6] + ["module", "fused"]
    assert type(f16.plans[6][1]) is type(f32.plans[6][1]) and f16.plans[7][1].entry == BF16
    feats, logits = f16.run(x, sampling=samp)
    assert feats[6].shape == (B, 1024, 96) and logits.shape == (B, N, 50) and bool(torch.isfinite(logits).all())


# ------------------------------------------------------------------------------------------------- 8. memory
def test_bf16_frozen_partseg_forward_memory(dev):
    """A bf16 forward holds what the fp32 frozen forward holds; the bf16 copies of the ten weights live in the snapshot.  Allowed
    on top of the fp32 peak: their bytes, each rounded up to the allocator's 512-byte block."""
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    net = _net()
    B, N = 4, 2048
    x = _clouds(dev, B, N, seed=6)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    f32, f16 = FrozenPointConvPartseg(net), FrozenPointConvPartseg(net, precision="bf16")

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

    p32, p16 = peak(lambda: f32(x, sampling=samp)), peak(lambda: f16(x, sampling=samp))
    ws = [w for kind, plan in f16.plans if kind == "fused" for w in plan.Ws_bf16[1:]]
    copies = sum(w.numel() * w.element_size() for w in ws)
    blocks = sum(-(-w.numel() * w.element_size() // 512) * 512 for w in ws)
    print(f"peak of a forward: bf16 +{p16 / 2**20:.2f} MiB, fp32 +{p32 / 2**20:.2f} MiB, bf16 weight copies {copies / 2**10:.0f} KiB "
          f"in {len(ws)} tensors ({blocks / 2**10:.0f} KiB of allocator blocks)")
    assert len(ws) == 10
    assert copies == 2 * (32 * 32 + 64 * 32 + 64 * 64 + 128 * 64 + 128 * 128 + 256 * 128 + 256 * 256 + 128 * 128 + 128 * 128 + 128 * 128)
    assert p16 <= p32 + blocks
