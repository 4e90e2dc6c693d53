"""bf16 frozen PointConv on the GPU (``FrozenPointConv(net, precision="bf16")``, pcl_pointconv_level_infer_bf16_f32 of
csrc/infer_pointconv.hip): the fused level kernel through the C ABI -- bit for bit against the fp64 restatement and against the
fp32 entry on the exactly representable data of tests/test_inference_pointconv_gpu.py (tests/test_inference_pointconv_bf16_cpu.py
holds that every z1, z2 and weight of those data is a bf16 number), within the derived bound of tests/pointconv_bf16_bound.py on
random data, group by group -- then the network, and the contract of the evaluator.

Shapes, seeds and modules are those of tests/test_inference_pointconv_gpu.py (imported, so the cached cases are shared)."""
import copy
import functools

import pytest
import torch

import pointconv_bf16_bound as PB
import pointconv_infer_ref as R
from test_inference_pointconv_gpu import (EXACT_SEED, MANY, SHAPES, _clouds, _frozen_stacks, _module_case, _net, _sampling_from, _start_idx)

pytestmark = pytest.mark.gpu

BF16 = "pcl_pointconv_level_infer_bf16_f32"
FP32 = "pcl_pointconv_level_infer_f32"


_level_call = functools.partial(R.level_call, entry=BF16)


# ------------------------------------------------------------------------------------------------- 1. exactly representable data
@pytest.mark.parametrize("ns", [32, 64])
def test_bf16_level_kernel_exact_data_bit_for_bit(dev, ns):
    _, widths, D, B, N, m = SHAPES[ns]
    c = R.exact_case(ns, widths, D, B, N, m, EXACT_SEED)
    nets = R.pack_nets(c["wn"], c["dn"], 400)
    args = (c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    want = R.level(c["feat"], c["wn"], c["dn"], *args)
    got = _level_call(dev, c["feat"], nets, *args)
    assert torch.equal(got.cpu(), want.float()), f"{int((got.cpu() != want.float()).sum())} of {want.numel()} outputs differ from fp64"
    assert torch.equal(got, _level_call(dev, c["feat"], nets, *args, entry=FP32)), "differs from the fp32 entry"


# ------------------------------------------------------------------------------------------------- 2. several tiles per workgroup
@pytest.mark.parametrize("ns", [32, 64])
def test_bf16_level_kernel_many_tiles_per_workgroup(dev, ns):
    """As tests/test_inference_pointconv_gpu.py::test_level_kernel_many_tiles_per_workgroup, on the bf16 entry: Z now lies over a
    smaller X1 | X2, and the tile loop reuses both.

    This is the test that found the packed-instruction defect of layer 1: with layer 1 left to the
    compiler's packed fp32 instructions, 2 to 9 of the 4101 groups of the ns = 64 launch differed from fp64 in every launch, other
    groups each time, while every B = 1 launch (2 tiles per workgroup) was exact.  With single-lane steps 18 launches were exact."""
    from pointcloudlib_amd import _lib
    _, widths, D, B, N, m = MANY[ns]
    gpt = 64 // ns
    gt_all, gt_one = (_lib.lib().pcl_pointconv_level_infer_group_tile(ns, G) for G in (B * m, m))
    assert gt_all >= 2 * gpt and gt_all > gt_one >= gpt, f"workgroups own {gt_all} groups in the large launch, {gt_one} in the B = 1 launch"
    c = R.exact_case(ns, widths, D, B, N, m, EXACT_SEED)
    nets = R.pack_nets(c["wn"], c["dn"], 400)
    pts = lambda b: None if c["points"] is None else c["points"][b]
    full = _level_call(dev, c["feat"], nets, c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    assert bool(torch.isfinite(full).all())
    for b in range(B):
        one = _level_call(dev, c["feat"], nets, c["xyz"][b:b + 1], c["new_xyz"][b:b + 1], pts(slice(b, b + 1)), c["idx"][b:b + 1],
                          c["density"][b:b + 1])
        assert torch.equal(full[b:b + 1], one), f"cloud {b} alone differs from cloud {b} in the batch"
    for b, sl in ((0, slice(0, 100)), (B - 1, slice(m - 100, m))):
        bs = slice(b, b + 1)
        want = R.level(c["feat"], c["wn"], c["dn"], c["xyz"][bs], c["new_xyz"][bs, sl], pts(bs), c["idx"][bs, sl], c["density"][bs])
        assert float((want != 0).double().mean()) > 0.3
        assert torch.equal(full[bs, sl].cpu(), want.float()), f"cloud {b}, groups {sl}: differs from fp64"


# ------------------------------------------------------------------------------------------------- 3. random data within the bound
@pytest.mark.parametrize("ns", [32, 64])
def test_bf16_level_kernel_within_the_bound(dev, ns):
    """MI355X: ns = 32 bf16 0.0324 x bound (fp32 entry 0.000044 x), ns = 64 bf16 0.0119 x bound (fp32 entry 0.000003 x)."""
    mods, c = _module_case(ns)
    feat, nets = _frozen_stacks(mods)
    args = (c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    got = _level_call(dev, feat, nets, *args)
    assert torch.equal(got, _level_call(dev, feat, nets, *args)), "two calls differ"
    assert bool(torch.isfinite(got).all())
    ref, bound = PB.level_ref_and_bound(feat, nets, *args)
    assert float((ref != 0).double().mean()) > 0.3, "a trivial level"
    assert bool(torch.isfinite(bound).all()) and bool((bound[ref != 0] > 0).all())
    ratio = PB.worst_ratio(got, ref, bound)
    ratio32 = PB.worst_ratio(_level_call(dev, feat, nets, *args, entry=FP32), ref, bound)
    print(f"ns={ns}: bf16 entry {ratio:.4f} x bound, fp32 entry {ratio32:.6f} x bound (largest |value| {float(ref.abs().max()):.3e}, "
          f"largest bf16 error {float((got.double() - ref).abs().max()):.3e})")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------- 4. group independence
def test_bf16_level_kernel_groups_are_independent(dev):
    mods, c = _module_case(32)
    feat, nets = _frozen_stacks(mods)
    assert c["points"] is None                                             # (ns = 32 carries no features: no Uf table to share)
    full = _level_call(dev, feat, nets, c["xyz"], c["new_xyz"], None, c["idx"], c["density"])
    one = _level_call(dev, feat, nets, c["xyz"][1:2], c["new_xyz"][1:2], None, c["idx"][1:2], c["density"][1:2])
    assert torch.equal(full[1:2], one), "cloud 1 alone differs from cloud 1 in the batch"
    perm = [2, 1, 0]                                                       # clouds 0 and 2 swapped: every group moves
    swapped = _level_call(dev, feat, nets, c["xyz"][perm], c["new_xyz"][perm], None, c["idx"][perm], c["density"][perm])
    assert torch.equal(swapped, full[perm])
    gp = [0, 3, 2, 1, 4]                                                   # two groups of one cloud swapped
    moved = _level_call(dev, feat, nets, c["xyz"], c["new_xyz"][:, gp], None, c["idx"][:, gp], c["density"])
    assert torch.equal(moved, full[:, gp])


def test_bf16_level_kernel_groups_share_one_uf_table(dev):
    """ns = 64, D = 128: two groups of a cloud swapped read the same Uf rows from their new places."""
    mods, c = _module_case(64)
    feat, nets = _frozen_stacks(mods)
    full = _level_call(dev, feat, nets, c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    gp = [2, 1, 0]
    moved = _level_call(dev, feat, nets, c["xyz"], c["new_xyz"][:, gp], c["points"], c["idx"][:, gp], c["density"])
    assert torch.equal(moved, full[:, gp])
    one = _level_call(dev, feat, nets, c["xyz"][1:2], c["new_xyz"][1:2], c["points"][1:2], c["idx"][1:2], c["density"][1:2])
    assert torch.equal(full[1:2], one)


# ------------------------------------------------------------------------------------------------- 5. the network
def test_bf16_frozen_pointconv_network(dev):
    """MI355X: sa1 contraction 0.0407 x bound, sa2 contraction 0.0148 x bound; logits max |bf16 - fp32| 1.5e-5, top-1 equal."""
    from pointcloudlib_amd.inference import FrozenPointConv
    net = copy.deepcopy(_net()).train()
    B, N = 4, 1024
    x = _clouds(dev, B, N, seed=2)
    samp = net.precompute_sampling(x)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    f32, f16 = FrozenPointConv(net), FrozenPointConv(net, precision="bf16")
    assert f16.levels == f32.levels == ["fused", "fused", "all"]
    assert type(f16.plans[2][1]) is type(f32.plans[2][1])
    assert all(type(a[1].linear) is type(b[1].linear) for a, b in zip(f16.plans[:2], f32.plans[:2]))
    assert [type(m) for m in f16.head] == [type(m) for m in f32.head]
    feats, logits = f16.run(x, sampling=samp)
    feats_again, logits_again = f16.run(x, sampling=samp)
    torch.cuda.synchronize()
    assert logits.shape == (B, 40) and logits.dtype == torch.float32 and bool(torch.isfinite(logits).all())
    assert torch.equal(logits, logits_again) and all(torch.equal(a, b) for a, b in zip(feats, feats_again)), "two runs differ"
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    # each fused launch on the bf16 run's own inputs, against the restatement of the constants it was given
    pts, points = x.permute(0, 2, 1).contiguous(), None
    for i in (0, 1):
        plan = f16.plans[i][1]
        new_xyz, ((idx, density),) = samp["levels"][i]
        new_xyz, idx, density = new_xyz.contiguous(), idx.contiguous(), density.contiguous()
        S = idx.shape[1]
        got = plan.contract(pts, new_xyz, points, idx, density).view(B, S, -1)
        feat = [(plan.W0, plan.scales[0], plan.shifts[0])] + [(plan.Ws[l], plan.scales[l], plan.shifts[l]) for l in (1, 2)]
        ref, bound = PB.level_ref_and_bound(feat, plan.nets, pts, new_xyz, points, idx, density, plan.slope)
        assert float((ref != 0).double().mean()) > 0.2, "a trivial level"
        ratio = PB.worst_ratio(got, ref, bound)
        print(f"sa{i + 1} contraction: {ratio:.4f} x bound (largest |value| {float(ref.abs().max()):.3e}, largest error "
              f"{float((got.double() - ref).abs().max()):.3e})")
        assert ratio <= 1.0
        assert torch.equal(plan.linear.run(got.view(B * S, -1)).view(B, S, -1), feats[i])
        pts, points = new_xyz, feats[i]
    l32 = f32(x, sampling=samp)
    print(f"logits: max |bf16 - fp32| {float((logits - l32).abs().max()):.3e} (largest |logit| {float(l32.abs().max()):.3e}), "
          f"top-1 agreement {float((logits.argmax(1) == l32.argmax(1)).float().mean()):.2f}")
    with torch.no_grad():
        net.sa2.mlp.weights[1].mul_(1.5)
    assert torch.equal(f16(x, sampling=samp), logits)                      # a snapshot: stale until refresh()
    fresh = f16.refresh()(x, sampling=samp)
    assert f16.precision == "bf16" and not torch.equal(fresh, logits)
    assert torch.equal(fresh, FrozenPointConv(net, precision="bf16")(x, sampling=samp))


# ------------------------------------------------------------------------------------------------- 6. the contract
def test_bf16_frozen_pointconv_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointConv
    net = _net()
    fnet = FrozenPointConv(net, precision="bf16")
    assert fnet.precision == "bf16" and FrozenPointConv(net).precision == "fp32"
    x = _clouds(dev, 2, 1024, seed=3)
    for bad in (x.cpu(), x.double()):
        with pytest.raises(TypeError, match="float32 tensor on the GPU"):
            fnet(bad)
    # a bf16 weight 8 bytes behind a 16-byte boundary: the wrapper holds the entry point's precondition
    samp = _sampling_from(net, x, _start_idx(dev, 2, 1024))
    plan = fnet.plans[0][1]
    new_xyz, ((idx, density),) = samp["levels"][0]
    pts = x.permute(0, 2, 1).contiguous()
    args = (pts, new_xyz.contiguous(), None, idx.contiguous(), density.contiguous())
    good = plan.contract(*args)
    w = plan.Ws_bf16[2]
    base = torch.empty(w.numel() + 8, dtype=torch.bfloat16, device=dev)
    off = base[4:4 + w.numel()].view_as(w)
    off.copy_(w)
    assert off.data_ptr() % 16 == 8
    plan.Ws_bf16[2] = off
    with pytest.raises(ValueError, match="pcl_pointconv_level_infer_bf16_f32.*16-byte aligned"):
        plan.contract(*args)
    plan.Ws_bf16[2] = w
    assert torch.equal(plan.contract(*args), good)


def test_bf16_frozen_pointconv_forward_memory(dev):
    """A bf16 forward holds what the fp32 frozen forward holds, plus the bf16 copies of the four weights."""
    from pointcloudlib_amd.inference import FrozenPointConv
    net = _net()
    B, N = 8, 1024
    x = _clouds(dev, B, N, seed=6)
    samp = _sampling_from(net, x, _start_idx(dev, B, N))
    f32, f16 = FrozenPointConv(net), FrozenPointConv(net, precision="bf16")

    def peak(fn):
        fn()                                       # warm-up: one-time allocations (constants, plans)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        assert out.shape == (B, 40)
        del out
        return torch.cuda.max_memory_allocated() - base

    p32, p16 = peak(lambda: f32(x, sampling=samp)), peak(lambda: f16(x, sampling=samp))
    copies = sum(w.numel() * w.element_size() for _, plan in f16.plans[:2] for w in plan.Ws_bf16[1:])
    print(f"peak of a forward: bf16 +{p16 / 2**20:.2f} MiB, fp32 +{p32 / 2**20:.2f} MiB, bf16 weight copies {copies / 2**10:.0f} KiB")
    assert copies == 2 * (64 * 64 + 128 * 64 + 128 * 128 + 256 * 128)
    assert p16 <= p32 + copies
