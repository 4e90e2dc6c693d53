"""Frozen inference for PointCNN classification on the GPU (pointcloudlib_amd/inference.py: FrozenPointCNN, csrc/infer_xconv.hip):
the fused stage kernel through the C ABI -- against the fp64 restatement of tests/pointcnn_infer_ref.py, bit for bit on exactly
representable data, region by region -- then whole networks, the contract of the evaluator, the fallback for a stage without a
kernel and the memory a forward needs.

Yardstick (tests/test_inference_gpu.py): the fused path may be no further from the fp64 restatement than the existing path on the
same inputs (max |difference|), x 1.25, plus 1e-6.  The existing path of the stage kernel is the composite of the eval-mode
modules on the same lists (``group_points``, ``index_points``, the lift, the three X-transform layers, ``xconv_core``); of a
network, ``net.eval()`` under ``no_grad``.

``_perturb`` (tests/test_inference_gpu.py) moves the BatchNorms of the PointwiseMLPs; ``_perturb_all`` moves the ones behind
``Conv`` and ``SepConv`` too."""
import copy
import functools

import pytest
import torch

import pointcnn_infer_ref as R
from test_inference_gpu import _err, _perturb
from test_inference_pointcnn_cpu import _perturb_all

pytestmark = pytest.mark.gpu

# RandPointCNN(C_in, C_out, 3, K, D, P) of the four stages; the level tests run them on B = 3, N = 40, P = 5: 15 regions, the one
# tile partly filled and straddling the clouds
STAGE_ARGS = {1: (3, 48, 8, 1, -1), 2: (48, 96, 12, 2, 384), 3: (96, 192, 16, 2, 128), 4: (192, 384, 16, 3, 128)}
B0, N0, P0 = 3, 40, 5
EXACT_SEED = 0                                   # tests/test_inference_pointcnn_cpu.py::test_exact_cases_are_exact holds it


@functools.lru_cache(maxsize=None)
def _module_case(s):
    """A perturbed eval-mode stage, its plan and random inputs (on the device), shared by the tests that read them."""
    from pointcloudlib_amd.inference import _FusedXConv, _xconv_fusable
    from pointcloudlib_amd.misc.pointcnn import RandPointCNN
    dev = torch.device("cuda:0")
    C_in, C_out, K, D, P = STAGE_ARGS[s]
    torch.manual_seed(100 + s)
    st = RandPointCNN(C_in, C_out, 3, K, D, P).to(dev)
    _perturb_all(_perturb(st, 7 + s), 70 + s).eval()
    assert _xconv_fusable(st)
    g = torch.Generator().manual_seed(s)
    case = {"pts": torch.rand(B0, N0, 3, generator=g), "rep": torch.rand(B0, P0, 3, generator=g),
            "fts": torch.randn(B0, N0, C_in, generator=g), "knn": R.knn_lists(B0, K * D, P0, N0, g)}
    return st, _FusedXConv(st, None), {k: v.to(dev) for k, v in case.items()}


def _rows(plan, fts):
    from pointcloudlib_amd.inference import _rows_gemm
    B, N, C = fts.shape
    return _rows_gemm(fts.reshape(B * N, C).contiguous(), plan.Wd, plan.bd, tag="pt").view(B, N, -1)


def _composite(st, c):
    """The existing path on the same lists, up to the depthwise taps."""
    from pointcloudlib_amd.misc.ops import group_points, index_points
    from pointcloudlib_amd.misc.pointcnn import xconv_core
    pc, xc = st.pointcnn, st.pointcnn.x_conv
    idx = R.dilated(c["knn"], pc.D)
    B, P, K = idx.shape
    with torch.no_grad():
        fts = pc.dense(c["fts"])
        local = group_points(c["pts"].contiguous(), c["rep"].contiguous(), None, idx, use_xyz=True).contiguous()
        regional = index_points(fts, idx)
        X = xc.x_trans_2(xc.x_trans_1(xc.x_trans_0(local))).reshape(B, P, K, K)
        return xconv_core(X, xc.dense(local), regional, xc.end_conv.depthwise, xc.end_conv.depthwise_bias)


# ------------------------------------------------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_level_kernel_against_fp64(dev, s):
    st, plan, c = _module_case(s)
    k = R.plan_consts(plan)
    rows = _rows(plan, c["fts"])
    got = R.level_call(dev, k, c["pts"], c["rep"], rows, c["knn"], plan.D)
    again = R.level_call(dev, k, c["pts"], c["rep"], rows, c["knn"], plan.D)
    assert torch.equal(got, again), "two calls differ"
    want_eval = _composite(st, c)
    sc = R.stage_consts(st)
    W, b, _, _ = sc["dense"]
    ref = R.level(sc, c["pts"], c["rep"], c["fts"].double() @ W.t() + b, R.dilated(c["knn"], plan.D))
    assert got.shape == want_eval.shape == ref.shape
    assert float((ref != 0).double().mean()) > 0.3, "a trivial stage"
    e_fused, e_eval = _err(got, ref), _err(want_eval, ref)
    print(f"stage {s}: fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64 (largest |value| {float(ref.abs().max()):.3e})")
    assert e_fused <= 1.25 * e_eval + 1e-6, f"fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64"


# ------------------------------------------------------------------------------------------------- 2. exactly representable data
def _exact_call(dev, c, d, sl=slice(None)):
    return R.level_call(dev, R.kernel_consts(c), d["pts"][sl], d["rep"][sl], d["rows"][sl], d["knn"][sl], c["D"])


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_level_kernel_exact_data_bit_for_bit(dev, s):
    c, d = R.exact_case(s, B0, N0, P0, EXACT_SEED)
    want = R.level(c, d["pts"], d["rep"], d["rows"], R.dilated(d["knn"], c["D"]))
    got = _exact_call(dev, c, d)
    assert torch.equal(got.cpu(), want.float()), f"{int((got.cpu() != want.float()).sum())} of {want.numel()} outputs differ"


# ------------------------------------------------------------------------------------------------- 3. dilation
@pytest.mark.parametrize("s", [2, 4])
def test_level_kernel_dilation_is_the_row_stride(dev, s):
    _, plan, c = _module_case(s)
    k = R.plan_consts(plan)
    rows = _rows(plan, c["fts"])
    assert plan.D > 1
    strided = R.level_call(dev, k, c["pts"], c["rep"], rows, c["knn"], plan.D)
    sliced = R.level_call(dev, k, c["pts"], c["rep"], rows, c["knn"][:, 0::plan.D, :].contiguous(), 1)
    assert torch.equal(strided, sliced)


# ------------------------------------------------------------------------------------------------- 4. region independence
@pytest.mark.parametrize("s", [1, 3])
def test_level_kernel_regions_are_independent(dev, s):
    _, plan, c = _module_case(s)
    k = R.plan_consts(plan)
    rows = _rows(plan, c["fts"])
    call = lambda pts, rep, rw, knn: R.level_call(dev, k, pts, rep, rw, knn, plan.D)
    full = call(c["pts"], c["rep"], rows, c["knn"])
    one = call(c["pts"][1:2], c["rep"][1:2], rows[1:2], c["knn"][1:2])
    assert torch.equal(full[1:2], one), "cloud 1 alone differs from cloud 1 in the batch"
    perm = [2, 1, 0]                                                       # clouds 0 and 2 swapped: every region moves
    assert torch.equal(call(c["pts"][perm], c["rep"][perm], rows[perm], c["knn"][perm]), full[perm])
    gp = [0, 3, 2, 1, 4]                                                   # two regions of every cloud swapped
    assert torch.equal(call(c["pts"], c["rep"][:, gp], rows, c["knn"][:, :, gp]), full[:, gp])


# ------------------------------------------------------------------------------------------------- 4b. several tiles per workgroup
# stage -> (B, P) at N = 40: enough regions that a workgroup of the large launch owns more tiles than one of a B = 1 launch on an
# MI355X (K = 16: one workgroup per compute unit wanted, K = 8: two); B * P is odd, so the last tile is partly filled
MANY = {1: (5, 3279), 4: (5, 1639)}


@pytest.mark.parametrize("s", [1, 4])
def test_level_kernel_many_tiles_per_workgroup(dev, s):
    """A launch whose workgroups walk several tiles (the tile loop's closing barrier, the reuse of PT, H, TA and TB, the region index
    at t0 > g0) on the exactly representable data: every cloud bit for bit a B = 1 launch of that cloud, whose workgroups own fewer
    tiles, and the first and last 100 regions bit for bit the fp64 restatement."""
    from pointcloudlib_amd import _lib
    B, P = MANY[s]
    K = R.STAGES[s][0]
    rt_all, rt_one = (_lib.lib().pcl_xconv_level_infer_region_tile(K, n) for n in (B * P, P))
    assert rt_all > rt_one >= 16, f"workgroups own {rt_all} regions in the large launch, {rt_one} in the B = 1 launch"
    c, d = R.exact_case(s, B, N0, P, EXACT_SEED)
    full = _exact_call(dev, c, d)
    assert bool(torch.isfinite(full).all())
    for b in range(B):
        assert torch.equal(full[b:b + 1], _exact_call(dev, c, d, slice(b, b + 1))), f"cloud {b} alone differs from cloud {b} in the batch"
    for b, sl in ((0, slice(0, 100)), (B - 1, slice(P - 100, P))):
        audit = []
        want = R.level(c, d["pts"][b:b + 1], d["rep"][b:b + 1, sl], d["rows"][b:b + 1], R.dilated(d["knn"][b:b + 1, :, sl], c["D"]), audit=audit)
        assert max(audit) < 2.0 ** 24 and float((want != 0).double().mean()) > 0.3       # exact in any order, and no trivial result
        assert torch.equal(full[b:b + 1, sl].cpu(), want.float()), f"cloud {b}, regions {sl}: differs from fp64"


# ------------------------------------------------------------------------------------------------- 5.-8. networks
@functools.lru_cache(maxsize=None)
def _net(seed=0):
    from pointcloudlib_amd.networks.cls.pointcnn import PointCNNcls
    torch.manual_seed(seed)
    net = PointCNNcls().to("cuda:0")
    return _perturb_all(_perturb(net, seed + 1), seed + 2)


def _clouds(dev, B, N, seed=0):
    from pointcloudlib_amd import synth
    return (torch.from_numpy(synth.gauss_ball(B, N, seed)).to(dev).contiguous(), torch.from_numpy(synth.unit_normals(B, N, seed + 1)).to(dev).contiguous())


def _stages(net):
    return [net.pcnn1] + list(net.pcnn2)


def _eval_run(net, x, normal):
    """The existing evaluation path (net.eval() + no_grad) on a copy, stage by stage -> (features, logits, the GPU's own
    representatives and k-NN lists of every stage)."""
    ev = copy.deepcopy(net).eval()
    feats, reps, knns = [], [], []
    with torch.no_grad():
        pts, fts = x, (x if normal is None else normal)
        for st in _stages(ev):
            rep, fts = st((pts, fts))
            knns.append(st.pointcnn.knn(rep.transpose(1, 2).contiguous(), pts.transpose(1, 2).contiguous()))
            feats.append(fts)
            reps.append(rep)
            pts = rep
        return feats, ev(x, normal), reps, knns


def _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, what):
    for i, (f, e, r) in enumerate(zip(feats, ev_feats, ref_feats)):
        assert f.shape == e.shape == r.shape, (i, f.shape, e.shape, r.shape)
        ef, ee = _err(f, r), _err(e, r)
        print(f"{what} stage {i + 1}: frozen {ef:.3e} vs eval {ee:.3e} from fp64 (largest |value| {float(r.abs().max()):.3e})")
        assert ef <= 1.25 * ee + 1e-6, f"{what} stage {i + 1}: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    ef, ee = _err(logits, ref_logits), _err(ev_logits, ref_logits)
    print(f"{what} logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64")
    assert ef <= 1.25 * ee + 1e-6, f"{what} logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64"


@pytest.mark.parametrize("with_normal", [False, True])
def test_frozen_pointcnn_against_fp64(dev, with_normal):
    from pointcloudlib_amd.inference import FrozenPointCNN
    net = _net()
    x, nrm = _clouds(dev, 2, 512)
    normal = nrm if with_normal else None
    fnet = FrozenPointCNN(net)
    assert fnet.levels == ["fused"] * 4
    feats, logits = fnet.run(x, normal)
    assert torch.equal(fnet(x, normal), logits)
    ev_feats, ev_logits, reps, knns = _eval_run(net, x, normal)
    ref_feats, ref_logits = R.network(net, x, normal, reps, knns)
    torch.cuda.synchronize()
    assert logits.shape == (2, 40) and [f.shape[1:] for f in feats] == [(512, 48), (384, 96), (128, 192), (128, 384)]
    assert all(float((r != 0).double().mean()) > 0.2 for r in ref_feats), "a trivial stage"
    _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, "normal" if with_normal else "xyz")
    assert torch.equal(logits.argmax(1), ev_logits.argmax(1)), "top-1 differs from net.eval()"


def test_frozen_pointcnn_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointCNN
    net = copy.deepcopy(_net()).train()
    x, _ = _clouds(dev, 2, 512, seed=3)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = FrozenPointCNN(net)
    out = fnet(x)
    torch.cuda.synchronize()
    assert out.shape == (2, 40)
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    with torch.no_grad():
        net.pcnn2[0].pointcnn.x_conv.x_trans_1.mlp.weights[0].mul_(1.5)
        net.pcnn2[1].pointcnn.x_conv.end_conv.bn.running_mean.add_(0.25)
    stale = fnet(x)
    fresh = fnet.refresh()(x)
    torch.cuda.synchronize()
    assert torch.equal(stale, out)
    assert not torch.equal(fresh, out)
    assert torch.equal(fresh, FrozenPointCNN(net)(x))
    with pytest.raises(ValueError, match="fp32 only"):
        FrozenPointCNN(net, precision="bf16")


def test_frozen_pointcnn_falls_back_for_other_shapes(dev):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.inference import FrozenPointCNN
    from pointcloudlib_amd.networks.cls.pointcnn import AbbPointCNN
    assert not _lib.lib().pcl_xconv_level_infer_supported(8, 16, 32, 22)
    net = copy.deepcopy(_net())
    torch.manual_seed(5)
    net.pcnn1 = AbbPointCNN(3, 64, 8, 1, -1).to(dev)                     # C_out = 64: C_mid 16, dense 32, dm 22 -- no kernel
    net.pcnn2[0] = AbbPointCNN(64, 96, 12, 2, 384).to(dev)              # (12, 24, 48, 2): the kernel of stage 2
    _perturb_all(_perturb(net, 9), 10)
    x, _ = _clouds(dev, 2, 512, seed=4)
    fnet = FrozenPointCNN(net)
    assert fnet.levels == ["module", "fused", "fused", "fused"]
    feats, logits = fnet.run(x)
    ev_feats, ev_logits, reps, knns = _eval_run(net, x, None)
    ref_feats, ref_logits = R.network(net, x, None, reps, knns)
    torch.cuda.synchronize()
    assert feats[0].shape == (2, 512, 64)
    _assert_yardstick(feats, logits, ev_feats, ev_logits, ref_feats, ref_logits, "fallback")
    with torch.no_grad():
        net.pcnn1.pointcnn.x_conv.dense.weights[1].mul_(1.5)
    assert torch.equal(fnet(x), logits)
    fresh = fnet.refresh()(x)
    assert not torch.equal(fresh, logits)
    assert torch.equal(fresh, FrozenPointCNN(net)(x))


def test_frozen_pointcnn_forward_memory(dev):
    from pointcloudlib_amd.inference import FrozenPointCNN
    net = _net()
    B, N = 8, 1024
    x, _ = _clouds(dev, B, N, seed=6)
    fnet = FrozenPointCNN(net)
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
        p_frozen, p_eval = peak(lambda: fnet(x)), peak(lambda: ev(x))
    # what a frozen forward may hold at once, in floats: the inputs, stage 1's D [B*N, 576] and dense output [B*N, 24], and the
    # largest D of a later stage (stage 4's [B*128, 576]), plus 25 % (lists, the pointwise outputs)
    bound = 1.25 * 4 * (B * N * 3 + B * N * 576 + B * N * 24 + B * 128 * 576)
    print(f"peak of a forward: frozen +{p_frozen / 2**20:.1f} MiB, net.eval() +{p_eval / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB")
    assert p_frozen < p_eval
    assert p_frozen <= bound, f"frozen forward peak +{p_frozen / 2**20:.1f} MiB > bound {bound / 2**20:.1f} MiB"
