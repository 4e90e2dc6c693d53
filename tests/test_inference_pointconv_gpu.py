"""Frozen inference for PointConv classification on the GPU (pointcloudlib_amd/inference.py: FrozenPointConv,
csrc/infer_pointconv.hip): the fused level kernel through the C ABI -- against the fp64 restatement of
tests/pointconv_infer_ref.py, bit for bit on exactly representable data, group by group -- then whole networks, the contract of the
evaluator, the fallback for a level without a kernel and the memory a forward needs.

Yardstick (tests/test_inference_gpu.py): the fused path may be no further from the fp64 restatement than the existing path on the
same inputs (max |difference|), x 1.25, plus 1e-6.  The existing path of the level kernel is the composite ``index_points`` +
eval-mode ``PointwiseMLP`` copies + ``pointconv_contract``; of a network, ``net.eval()`` under ``no_grad``.

``_perturb`` makes a fifth of the BatchNorm gammas negative; a DensityNet's single output channel behind a negative gamma is zero
for every point and erases its level, so ``_alive`` gives that one channel a positive gamma and beta after the perturbation."""
import copy
import functools

import pytest
import torch

import pointconv_infer_ref as R
from test_inference_gpu import _err, _perturb

pytestmark = pytest.mark.gpu

# (ns, widths, point features D, B, N, m): 15 groups at ns = 32 (the last tile half filled, tiles straddle clouds, N % 4 != 0);
# Uf from 128 point features at ns = 64
SHAPES = {32: (32, [64, 64, 128], 0, 3, 40, 5), 64: (64, [128, 128, 256], 128, 2, 70, 3)}
EXACT_SEED = 0                                   # tests/test_inference_pointconv_cpu.py::test_exact_cases_are_exact holds it


def _alive(root):
    from pointcloudlib_amd.misc.pointconv_utils import DensityNet
    with torch.no_grad():
        for mod in root.modules():
            if isinstance(mod, DensityNet):
                mod.mlp.gammas[-1].abs_()
                mod.mlp.betas[-1].fill_(0.5)
    return root


_level_call = functools.partial(R.level_call, entry="pcl_pointconv_level_infer_f32")


# ------------------------------------------------------------------------------------------------- 1. against fp64
@functools.lru_cache(maxsize=None)
def _module_case(ns):
    """Perturbed eval-mode modules of one level and random inputs (on the device), shared by the tests that read them."""
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.misc.pointconv_utils import DensityNet, WeightNet
    dev = torch.device("cuda:0")
    _, widths, D, B, N, m = SHAPES[ns]
    torch.manual_seed(100 + ns)
    mods = torch.nn.ModuleDict({"mlp": PointwiseMLP([3 + D] + widths, bias=True), "wn": WeightNet(3, 16), "dn": DensityNet()}).to(dev)
    _alive(_perturb(mods, 7 + ns)).eval()
    g = torch.Generator().manual_seed(ns)
    case = {"xyz": torch.rand(B, N, 3, generator=g), "new_xyz": torch.rand(B, m, 3, generator=g),
            "points": None if D == 0 else torch.randn(B, N, D, generator=g), "density": 3 * torch.rand(B, N, generator=g).clamp(min=1e-3),
            "idx": R.knn_lists(B, N, m, ns, g)}
    return mods, {k: None if v is None else v.to(dev) for k, v in case.items()}


def _composite(mods, c):
    """The existing path: index_points, the eval-mode PointwiseMLP copies, pointconv_contract."""
    from pointcloudlib_amd.misc.ops import index_points
    from pointcloudlib_amd.misc.pointconv_utils import pointconv_contract
    B, m, _ = c["idx"].shape
    with torch.no_grad():
        d = (index_points(c["xyz"], c["idx"]) - c["new_xyz"].view(B, m, 1, 3)).contiguous()
        x = d if c["points"] is None else torch.cat([d, index_points(c["points"], c["idx"])], dim=-1).contiguous()
        rho = index_points(mods["dn"](c["density"]), c["idx"])
        return pointconv_contract(mods["mlp"](x), rho, mods["wn"](d))


def _frozen_stacks(mods):
    from pointcloudlib_amd.inference import _eval_consts, pack_small_nets
    mlp = mods["mlp"]
    feat = [(mlp.weights[l].detach(), *_eval_consts(mlp, l)) for l in range(mlp.n_layers)]
    return feat, pack_small_nets(mods["wn"], mods["dn"])


@pytest.mark.parametrize("ns", [32, 64])
def test_level_kernel_against_fp64(dev, ns):
    mods, c = _module_case(ns)
    feat, nets = _frozen_stacks(mods)
    args = (c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    got = _level_call(dev, feat, nets, *args)
    again = _level_call(dev, feat, nets, *args)
    assert torch.equal(got, again), "two calls differ"
    want_eval = _composite(mods, c)
    ref = R.level(R.stack_of(mods["mlp"]), R.stack_of(mods["wn"].mlp), R.stack_of(mods["dn"].mlp), *args)
    assert float((ref != 0).double().mean()) > 0.3, "a trivial level"
    e_fused, e_eval = _err(got, ref), _err(want_eval, ref)
    print(f"ns={ns}: fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64 (largest |value| {float(ref.abs().max()):.3e})")
    assert e_fused <= 1.25 * e_eval + 1e-6, f"fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64"


def test_packed_small_nets_against_the_modules(dev):
    """The folded constants (evaluated in fp64 at the header's offsets) against the modules' own eval outputs."""
    from test_inference_pointconv_cpu import _small_nets_torch
    mods, c = _module_case(32)
    _, nets = _frozen_stacks(mods)
    d = (torch.rand(300, 3, device=dev) - 0.5).contiguous()
    dens = (3 * torch.rand(1, 300, device=dev)).clamp(min=1e-3)
    with torch.no_grad():
        w_mod, rho_mod = mods["wn"](d.view(1, 1, 300, 3)).view(300, 16), mods["dn"](dens).view(300, 1)
    w, rho = _small_nets_torch(nets, d.double(), dens.double().view(300, 1))
    assert float(w_mod.abs().max()) > 0.1 and float(rho_mod.abs().max()) > 0.1
    assert _err(w_mod, w) <= 1e-5 * float(w.abs().max()) and _err(rho_mod, rho) <= 1e-5 * float(rho.abs().max())


# ------------------------------------------------------------------------------------------------- 2. exactly representable data
@pytest.mark.parametrize("ns", [32, 64])
def test_level_kernel_exact_data_bit_for_bit(dev, ns):
    _, widths, D, B, N, m = SHAPES[ns]
    c = R.exact_case(ns, widths, D, B, N, m, EXACT_SEED)
    want = R.level(c["feat"], c["wn"], c["dn"], c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    got = _level_call(dev, c["feat"], R.pack_nets(c["wn"], c["dn"], 400), c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    assert torch.equal(got.cpu(), want.float()), f"{int((got.cpu() != want.float()).sum())} of {want.numel()} outputs differ"


# ------------------------------------------------------------------------------------------------- 3. group independence
def test_level_kernel_groups_are_independent(dev):
    mods, c = _module_case(32)
    feat, nets = _frozen_stacks(mods)
    full = _level_call(dev, feat, nets, c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    one = _level_call(dev, feat, nets, c["xyz"][1:2], c["new_xyz"][1:2], None, c["idx"][1:2], c["density"][1:2])
    assert torch.equal(full[1:2], one), "cloud 1 alone differs from cloud 1 in the batch"
    perm = [2, 1, 0]                                                       # clouds 0 and 2 swapped: every group moves
    swapped = _level_call(dev, feat, nets, c["xyz"][perm], c["new_xyz"][perm], None, c["idx"][perm], c["density"][perm])
    assert torch.equal(swapped, full[perm])
    # two groups of one cloud swapped (centres and lists move together, the cloud stays)
    gp = [0, 3, 2, 1, 4]
    moved = _level_call(dev, feat, nets, c["xyz"], c["new_xyz"][:, gp], None, c["idx"][:, gp], c["density"])
    assert torch.equal(moved, full[:, gp])


# ------------------------------------------------------------------------------------------------- 3b. several tiles per workgroup
# (ns, widths, D, B, N, m): enough groups that a workgroup owns 8 tiles on an MI355X (at least two workgroups per compute unit
# remain), as a B = 32 forward does; G = 8195 is odd, so at ns = 32 the last workgroup's last tile is half filled behind full ones
MANY = {32: (32, [64, 64, 128], 0, 5, 40, 1639), 64: (64, [128, 128, 256], 128, 3, 70, 1367)}


@pytest.mark.parametrize("ns", [32, 64])
def test_level_kernel_many_tiles_per_workgroup(dev, ns):
    """A launch whose workgroups walk several tiles (the tile loop's closing barrier, the reuse of the row records, RW and Z, the
    group index at t0 > 0) on the exactly representable data: every cloud bit for bit a B = 1 launch of that cloud, whose workgroups
    own fewer tiles, and the first and last 100 groups bit for bit the fp64 restatement."""
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
        audit = []
        want = R.level(c["feat"], c["wn"], c["dn"], c["xyz"][bs], c["new_xyz"][bs, sl], pts(bs), c["idx"][bs, sl], c["density"][bs], audit=audit)
        assert max(audit) < 2.0 ** 24 and float((want != 0).double().mean()) > 0.3       # exact in any order, and no trivial result
        assert torch.equal(full[bs, sl].cpu(), want.float()), f"cloud {b}, groups {sl}: differs from fp64"


# ------------------------------------------------------------------------------------------------- 4.-7. networks
@functools.lru_cache(maxsize=None)
def _net(seed=0):
    from pointcloudlib_amd.networks.cls.pointconv import PointConvDensityClsSsg
    torch.manual_seed(seed)
    return _alive(_perturb(PointConvDensityClsSsg().to("cuda:0"), seed + 1))


def _clouds(dev, B, N=1024, seed=0):
    from pointcloudlib_amd import synth
    return torch.from_numpy(synth.gauss_ball(B, N, seed)).to(dev).permute(0, 2, 1).contiguous()             # [B,3,N]


def _eval_run(net, x, sampling):
    """The existing evaluation path (net.eval() + no_grad) on a copy, level by level -> (channel-last features, logits)."""
    ev = copy.deepcopy(net).eval()
    with torch.no_grad():
        lv = sampling["levels"]
        x1, p1 = ev.sa1(x, None, sampling=lv[0])
        x2, p2 = ev.sa2(x1, p1, sampling=lv[1])
        _, p3 = ev.sa3(x2, p2, sampling=lv[2])
        feats = [p.permute(0, 2, 1) for p in (p1, p2, p3)]
        return feats, ev(x, sampling=sampling)


def _start_idx(dev, B, N):
    g = torch.Generator().manual_seed(11)
    return (torch.randint(0, N, (B,), generator=g, dtype=torch.int32).to(dev), torch.randint(0, 512, (B,), generator=g, dtype=torch.int32).to(dev))


def _sampling_from(net, x, start):
    """A sampling handle with explicit FPS starts (what forward(start_idx=) would draw inline)."""
    pts = x.permute(0, 2, 1).contiguous()
    levels = []
    for sa, s in zip((net.sa1, net.sa2, net.sa3), (start[0], start[1], None)):
        lv = sa.sample(pts, s)
        levels.append(lv)
        pts = lv[0] if lv[0] is not None else pts
    return {"levels": levels, "event": None}


def _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, what):
    for i, (f, e, r) in enumerate(zip(feats, ev_feats, ref_feats)):
        assert f.shape == e.shape == r.shape, (i, f.shape, e.shape, r.shape)
        ef, ee = _err(f, r), _err(e, r)
        print(f"{what} level {i}: frozen {ef:.3e} vs eval {ee:.3e} from fp64 (largest |value| {float(r.abs().max()):.3e})")
        assert ef <= 1.25 * ee + 1e-6, f"{what} level {i}: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    ef, ee = _err(logits, ref_logits), _err(ev_logits, ref_logits)
    print(f"{what} logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64")
    assert ef <= 1.25 * ee + 1e-6, f"{what} logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64"


def test_frozen_pointconv_against_fp64(dev):
    from pointcloudlib_amd.inference import FrozenPointConv
    net = _net()
    B, N = 3, 1024
    x = _clouds(dev, B, N)
    start = _start_idx(dev, B, N)
    samp = _sampling_from(net, x, start)
    fnet = FrozenPointConv(net)
    assert fnet.levels == ["fused", "fused", "all"]
    feats, logits = fnet.run(x, start_idx=start)
    ev_feats, ev_logits = _eval_run(net, x, samp)
    ref_feats, ref_logits = R.network(net, x.permute(0, 2, 1), samp["levels"])
    torch.cuda.synchronize()
    assert all(float((r != 0).double().mean()) > 0.2 for r in ref_feats), "a trivial level"
    _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, "cls")
    assert torch.equal(logits.argmax(1), ev_logits.argmax(1)), "top-1 differs from net.eval()"


def test_frozen_pointconv_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointConv
    net = copy.deepcopy(_net()).train()
    B, N = 2, 1024
    x = _clouds(dev, B, N, seed=3)
    start = _start_idx(dev, B, N)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = FrozenPointConv(net)
    out_inline = fnet(x, start_idx=start)
    out_handle = fnet(x, sampling=_sampling_from(net, x, start))
    torch.cuda.synchronize()
    assert out_inline.shape == (B, 40)
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(out_inline, out_handle), "a precomputed sampling handle changes the output"
    lists = tuple(lv[1][0][0] for lv in _sampling_from(net, x, start)["levels"][:2])       # the same groups, handed in as knn_lists
    assert torch.equal(fnet(x, start_idx=start, knn_lists=lists), out_inline)
    with torch.no_grad():
        net.sa2.mlp.weights[1].mul_(1.5)
    stale = fnet(x, start_idx=start)
    fresh = fnet.refresh()(x, start_idx=start)
    torch.cuda.synchronize()
    assert torch.equal(stale, out_inline)
    assert not torch.equal(fresh, out_inline)
    assert torch.equal(fresh, FrozenPointConv(net)(x, start_idx=start))


def test_frozen_pointconv_falls_back_for_other_widths(dev):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.inference import FrozenPointConv
    from pointcloudlib_amd.misc.pointconv_utils import PointConvDensitySetAbstraction
    assert not _lib.lib().pcl_pointconv_level_infer_supported(32, 3, 32, 32, 64, 16)
    net = copy.deepcopy(_net())
    torch.manual_seed(5)
    net.sa1 = PointConvDensitySetAbstraction(npoint=512, nsample=32, in_channel=3, mlp=[32, 32, 64], bandwidth=0.1, group_all=False).to(dev)
    net.sa2 = PointConvDensitySetAbstraction(npoint=128, nsample=64, in_channel=64 + 3, mlp=[128, 128, 256], bandwidth=0.2, group_all=False).to(dev)
    _alive(_perturb(net, 9))
    B, N = 2, 1024
    x = _clouds(dev, B, N, seed=4)
    start = _start_idx(dev, B, N)
    samp = _sampling_from(net, x, start)
    fnet = FrozenPointConv(net)
    assert fnet.levels == ["module", "fused", "all"]
    feats, logits = fnet.run(x, sampling=samp)
    ev_feats, ev_logits = _eval_run(net, x, samp)
    ref_feats, ref_logits = R.network(net, x.permute(0, 2, 1), samp["levels"])
    torch.cuda.synchronize()
    assert feats[0].shape == (B, 512, 64)
    _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, "fallback")
    with torch.no_grad():
        net.sa1.mlp.weights[2].mul_(1.5)
    assert torch.equal(fnet(x, sampling=samp), logits)
    fresh = fnet.refresh()(x, sampling=samp)
    assert not torch.equal(fresh, logits)
    assert torch.equal(fresh, FrozenPointConv(net)(x, sampling=samp))


def test_frozen_pointconv_forward_memory(dev):
    from pointcloudlib_amd.inference import FrozenPointConv
    net = _net()
    B, N = 8, 1024
    x = _clouds(dev, B, N, seed=6)
    samp = _sampling_from(net, x, _start_idx(dev, B, N))
    fnet = FrozenPointConv(net)
    ev = copy.deepcopy(net).eval()

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

    with torch.no_grad():
        p_frozen, p_eval = peak(lambda: fnet(x, sampling=samp)), peak(lambda: ev(x, sampling=samp))
    # what a frozen forward may hold at once, in floats: the inputs, the two contraction outputs [B*S, 16 C] (the only large
    # intermediates of the k-NN levels) and sa2's Uf, plus 25 % (the group_all level's B*128 rows, the level outputs)
    contraction = B * 512 * 16 * 128 + B * 128 * 16 * 256
    uf = B * 512 * 128
    inputs = B * N * 3
    bound = 1.25 * 4 * (contraction + uf + inputs)
    grouped = 4 * B * 512 * 32 * 64                # one [B, S, ns, C1] tensor of sa1
    print(f"peak of a forward: frozen +{p_frozen / 2**20:.1f} MiB, net.eval() +{p_eval / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB, "
          f"one grouped sa1 tensor {grouped / 2**20:.1f} MiB")
    assert p_frozen < p_eval
    # sa1's fused launch of this forward (4 tiles per workgroup on an MI355X) against the launch of each cloud alone (1 tile)
    from pointcloudlib_amd import _lib
    assert _lib.lib().pcl_pointconv_level_infer_group_tile(32, B * 512) > _lib.lib().pcl_pointconv_level_infer_group_tile(32, 512)
    pts = x.permute(0, 2, 1).contiguous()
    new_xyz, ((idx, density),) = samp["levels"][0]
    plan = fnet.plans[0][1]
    with torch.no_grad():
        full = plan.contract(pts, new_xyz.contiguous(), None, idx.contiguous(), density.contiguous()).view(B, 512, -1)
        for b in range(B):
            one = plan.contract(pts[b:b + 1], new_xyz[b:b + 1].contiguous(), None, idx[b:b + 1].contiguous(), density[b:b + 1].contiguous())
            assert torch.equal(full[b], one), f"sa1 contraction of cloud {b}: the B = {B} launch differs from the cloud alone"
    assert p_frozen <= bound, f"frozen forward peak +{p_frozen / 2**20:.1f} MiB > bound {bound / 2**20:.1f} MiB"
