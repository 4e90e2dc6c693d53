"""The wide PointConv level kernel on the GPU (csrc/infer_pointconv_wide.hip through pcl_pointconv_wide_level_infer_f32: sa3 and in0
of the part-seg network, the last layer and the contraction a chunk of columns at a time) and ``FrozenPointConvPartseg(net,
wide_levels=True)``: the two shapes through the C ABI -- against the fp64 restatement of tests/pointconv_infer_ref.py, bit for bit
on exactly representable data (every output column: every chunk seam), group by group, several tiles per workgroup -- then the
whole network and the evaluator's contract.

Yardstick (tests/test_inference_gpu.py): the fused path may be no further from the fp64 restatement than the existing path on the
same inputs (max |difference|), x 1.25, plus 1e-6.  The existing path of the level kernel is the composite ``index_points`` +
eval-mode ``PointwiseMLP`` copies + ``pointconv_contract``; of the network, ``net.eval()`` under ``no_grad``."""
import copy
import functools

import pytest
import torch

import pointconv_infer_ref as R
import pointconv_partseg_infer_ref as RS
from pointconv_partseg_infer_ref import EXACT_SEED
from pointconv_wide_cases import ALL_FUSED, GROUP_TILE, MANY_B, MANY_M_END, MANY_N, MANY_SEED, SHAPES, STOCK, WIDE, case_args, many_m
from test_inference_gpu import _err, _perturb
from test_inference_pointconv_gpu import _alive, _composite, _frozen_stacks
from test_inference_pointconv_partseg_gpu import _clouds, _eval_run, _net, _start_idx

pytestmark = pytest.mark.gpu

NAMES = sorted(SHAPES)
_level_call = functools.partial(R.level_call, entry=WIDE)


@functools.lru_cache(maxsize=None)
def _module_case(name):
    """Perturbed eval-mode modules of one level and random inputs (on the device), shared by the tests that read them."""
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.misc.pointconv_utils import DensityNet, WeightNet
    dev = torch.device("cuda:0")
    ns, widths, D, B, N, m = SHAPES[name]
    seed = 500 + NAMES.index(name)
    torch.manual_seed(seed)
    mods = torch.nn.ModuleDict({"mlp": PointwiseMLP([3 + D] + widths, bias=True), "wn": WeightNet(3, 16), "dn": DensityNet()}).to(dev)
    _alive(_perturb(mods, seed + 7)).eval()
    g = torch.Generator().manual_seed(seed)
    case = {"xyz": torch.rand(B, N, 3, generator=g), "new_xyz": torch.rand(B, m, 3, generator=g),
            "points": torch.randn(B, N, D, generator=g), "density": 3 * torch.rand(B, N, generator=g).clamp(min=1e-3),
            "idx": R.knn_lists(B, N, m, ns, g)}
    return mods, {k: v.to(dev) for k, v in case.items()}


# ------------------------------------------------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("name", NAMES)
def test_level_kernel_against_fp64(dev, name):
    mods, c = _module_case(name)
    feat, nets = _frozen_stacks(mods)
    got = _level_call(dev, feat, nets, *case_args(c))
    again = _level_call(dev, feat, nets, *case_args(c))
    assert torch.equal(got, again), "two calls differ"
    want_eval = _composite(mods, c)
    ref = R.level(R.stack_of(mods["mlp"]), R.stack_of(mods["wn"].mlp), R.stack_of(mods["dn"].mlp), *case_args(c))
    assert got.shape == ref.shape == (SHAPES[name][3], SHAPES[name][5], 16 * 512)
    assert float((ref != 0).double().mean()) > 0.3, "a trivial level"
    e_fused, e_eval = _err(got, ref), _err(want_eval, ref)
    print(f"{name}: fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64 (largest |value| {float(ref.abs().max()):.3e})")
    assert e_fused <= 1.25 * e_eval + 1e-6, f"fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64"


# ------------------------------------------------------------------------------------------------- 2. exactly representable data
@pytest.mark.parametrize("name", NAMES)
def test_level_kernel_exact_data_bit_for_bit(dev, name):
    c = R.exact_case(*SHAPES[name], EXACT_SEED)
    want = R.level(c["feat"], c["wn"], c["dn"], *case_args(c))
    got = _level_call(dev, c["feat"], R.pack_nets(c["wn"], c["dn"], 400), *case_args(c))
    diff = got.cpu() != want.float()
    assert not bool(diff.any()), f"{int(diff.sum())} of {want.numel()} outputs differ, in columns {diff.reshape(-1, 512, 16).any(-1).any(0).nonzero().flatten().tolist()[:16]}"


# ------------------------------------------------------------------------------------------------- 3. group independence
@pytest.mark.parametrize("name", NAMES)
def test_level_kernel_groups_are_independent(dev, name):
    mods, c = _module_case(name)
    ns, N = SHAPES[name][0], SHAPES[name][4]
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
    # a partly filled last tile: the first groups of ONE cloud against the same groups in a launch of whole tiles -- ns = 16: 5, 6, 7
    # groups (1, 2, 3 live groups of 4 in the last tile) against eight; ns = 32: 3 groups (1 of 2) against four
    whole, parts = (8, (5, 6, 7)) if ns == 16 else (4, (3,))
    g = torch.Generator().manual_seed(5)
    more_xyz = torch.rand(1, whole, 3, generator=g).to(dev)
    more_idx = R.knn_lists(1, N, whole, ns, g).to(dev)
    ref = _level_call(dev, feat, nets, c["xyz"][:1], more_xyz, c["points"][:1], more_idx, c["density"][:1])
    assert ref[0].unique(dim=0).shape[0] == whole, "the groups are to differ"
    for m in parts:
        part = _level_call(dev, feat, nets, c["xyz"][:1], more_xyz[:, :m], c["points"][:1], more_idx[:, :m], c["density"][:1])
        assert torch.equal(part, ref[:, :m]), f"m = {m} of {whole}"


# ------------------------------------------------------------------------------------------------- 4. several tiles per workgroup
@pytest.mark.parametrize("name", NAMES)
def test_level_kernel_many_tiles_per_workgroup(dev, name):
    """A launch whose workgroups walk several tiles on the exactly representable data: every cloud bit for bit a B = 1 launch of that
    cloud, and the first and last 100 groups bit for bit the fp64 restatement."""
    from pointcloudlib_amd import _lib
    ns, widths, D = SHAPES[name][:3]
    B, N, gpt = MANY_B, MANY_N, 64 // ns
    group_tile = getattr(_lib.lib(), GROUP_TILE)
    m = many_m(group_tile, ns, B)
    assert m is not None, f"no m below {MANY_M_END} gives a workgroup two tiles at B = {B}"
    gt_all = group_tile(ns, B * m)
    print(f"{name}: m = {m}, {B * m} groups, {gt_all} groups ({gt_all // gpt} tiles) per workgroup; B = 1: {group_tile(ns, m)}")
    assert gt_all >= 2 * gpt, f"workgroups own {gt_all} groups"
    assert (B * m) % gpt != 0, "the last tile is to be partly filled"
    c = R.exact_case(ns, widths, D, B, N, m, MANY_SEED)
    nets = R.pack_nets(c["wn"], c["dn"], 400)
    full = _level_call(dev, c["feat"], nets, *case_args(c))
    assert bool(torch.isfinite(full).all())
    for b in range(B):
        bs = slice(b, b + 1)
        one = _level_call(dev, c["feat"], nets, c["xyz"][bs], c["new_xyz"][bs], c["points"][bs], c["idx"][bs], c["density"][bs])
        assert torch.equal(full[bs], one), f"cloud {b} alone differs from cloud {b} in the batch"
    for b, sl in ((0, slice(0, 100)), (B - 1, slice(m - 100, m))):
        bs = slice(b, b + 1)
        audit = []
        want = R.level(c["feat"], c["wn"], c["dn"], c["xyz"][bs], c["new_xyz"][bs, sl], c["points"][bs], c["idx"][bs, sl], c["density"][bs],
                       audit=audit)
        assert max(audit) < 2.0 ** 24 and float((want != 0).double().mean()) > 0.3       # exact in any order, and no trivial result
        assert torch.equal(full[bs, sl].cpu(), want.float()), f"cloud {b}, groups {sl}: differs from fp64"


# ------------------------------------------------------------------------------------------------- 5. the network
def test_frozen_partseg_wide_against_fp64(dev):
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    net = _net()
    B, N = 2, 2048
    x = _clouds(dev, B, N)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    wide, default = FrozenPointConvPartseg(net, wide_levels=True), FrozenPointConvPartseg(net)
    assert wide.levels == ALL_FUSED and default.levels == STOCK
    feats, logits = wide.run(x, sampling=samp)
    d_feats, d_logits = default.run(x, sampling=samp)
    ev_feats, ev_logits = _eval_run(net, x, samp)
    ref_feats, ref_logits = RS.network(net, x, samp["levels"])
    torch.cuda.synchronize()
    assert logits.shape == (B, N, 50)
    for name, f, d in zip(RS.LEVELS[:3], feats, d_feats):
        assert torch.equal(f, d), f"{name}: the level in front of the wide ones changed its bits"
    assert not torch.equal(feats[3], d_feats[3]) or not torch.equal(feats[4], d_feats[4]), "the wide levels did not run another path"
    for name, f, e, r in zip(RS.LEVELS + ("logits",), feats + [logits], ev_feats + [ev_logits], ref_feats + [ref_logits]):
        assert f.shape == e.shape == r.shape, (name, f.shape, e.shape, r.shape)
        ef, ee = _err(f, r), _err(e, r)
        print(f"wide {name}: frozen {ef:.3e} vs eval {ee:.3e} from fp64 (largest |value| {float(r.detach().abs().max()):.3e})")
        assert ef <= 1.25 * ee + 1e-6, f"wide {name}: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    # the same forward with bf16 operands in the six other levels: the wide levels run the fp32 wide kernel
    bf16 = FrozenPointConvPartseg(net, precision="bf16", wide_levels=True)
    assert bf16.levels == ALL_FUSED and [p.entry for _, p in bf16.plans[3:5]] == [WIDE, WIDE]
    b_logits = bf16(x, sampling=samp)
    torch.cuda.synchronize()
    assert b_logits.shape == logits.shape and bool(torch.isfinite(b_logits).all())
    print(f"bf16 + wide logits: {_err(b_logits, ref_logits):.3e} from fp64")


# ------------------------------------------------------------------------------------------------- 6. the contract
def test_frozen_partseg_wide_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    net = copy.deepcopy(_net()).train()
    B, N = 2, 2048
    x = _clouds(dev, B, N, seed=3)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    before = {k: v.clone() for k, v in net.state_dict().items()}
    wide = FrozenPointConvPartseg(net, wide_levels=True)
    out = wide(x, sampling=samp)
    explicit, plain = FrozenPointConvPartseg(net, wide_levels=False)(x, sampling=samp), FrozenPointConvPartseg(net)(x, sampling=samp)
    torch.cuda.synchronize()
    assert torch.equal(explicit, plain), "wide_levels=False is not the form without the keyword"
    assert torch.equal(wide(x, sampling=samp), out), "two forwards differ"
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    with torch.no_grad():
        net.sa3.mlp.running_mean_2.add_(0.25)
        net.sa3.mlp.running_var_1.mul_(1.5)
    stale = wide(x, sampling=samp)
    fresh = wide.refresh()(x, sampling=samp)
    torch.cuda.synchronize()
    assert wide.levels == ALL_FUSED
    assert torch.equal(stale, out)
    assert not torch.equal(fresh, out)
    assert torch.equal(fresh, FrozenPointConvPartseg(net, wide_levels=True)(x, sampling=samp))


def test_frozen_partseg_wide_forward_memory(dev):
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    net = _net()
    B, N = 4, 2048
    x = _clouds(dev, B, N, seed=6)
    samp = net.precompute_sampling(x, _start_idx(dev, B))
    wide, default = FrozenPointConvPartseg(net, wide_levels=True), FrozenPointConvPartseg(net)

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

    p_wide, p_default = peak(lambda: wide(x, sampling=samp)), peak(lambda: default(x, sampling=samp))
    print(f"peak of a forward at B = {B}: wide +{p_wide / 2**20:.2f} MiB, default +{p_default / 2**20:.2f} MiB")
    assert p_wide <= p_default
