"""Frozen inference for PointCNN part segmentation on the GPU (pointcloudlib_amd/inference.py: FrozenPointCNNPartseg,
csrc/infer_xconv.h, csrc/infer_xconv_seg.hip): the FX form and the new tap shapes of the level kernel through the C ABI -- against
the fp64 restatement of tests/pointcnn_partseg_infer_ref.py, bit for bit on exactly representable data, region by region -- then
the whole network, the contract of the evaluator, its plans and the memory a forward needs.

Yardstick (tests/test_inference_gpu.py): the fused path may be no further from the fp64 restatement than the existing path on the
same inputs (max |difference|), x 1.25, plus 1e-6.  For a stage it is taken at ``raw``, the pointwise conv's output: the existing
path is the composite of the eval-mode modules on the same lists (for encoder_0: ``xconv_core``'s einsum form and the 16512-wide
pointwise GEMM); for the network, ``net.eval()`` under ``no_grad``."""
import copy
import functools

import pytest
import torch

import pointcnn_infer_ref as R
import pointcnn_partseg_infer_ref as S
from test_inference_gpu import _err, _perturb
from test_inference_pointcnn_cpu import _perturb_all

pytestmark = pytest.mark.gpu

NAMES = list(S.SHAPES)                           # every instantiation of csrc/infer_xconv_seg.hip
# constructor arguments of the stage modules (networks/seg/pointcnn_partseg.py)
STAGE_ARGS = {"encoder_0": (3, 256, 8, 1, -1), "encoder_1": (256, 256, 12, 1, 768), "decoder_3": (256, 50, 256, 8, 1, 2048)}
B0, P0 = 3, 5                                    # 15 regions: the one tile partly filled and straddling the clouds
EXACT_SEED = 0                                   # tests/test_inference_pointcnn_partseg_cpu.py::test_exact_cases_are_exact holds it


def _n0(name):
    K, D = S.SHAPES[name][:2]
    return K * D + 3


def _is_fx(name):
    return name in S.FX_SHAPES


def _ref_level(name):
    return S.level_fx if _is_fx(name) else R.level


@functools.lru_cache(maxsize=None)
def _exact(name, B, N, P):
    return S.exact_case(name, B, N, P, EXACT_SEED)


def _exact_call(dev, name, c, d, sl=slice(None), **kw):
    return S.level_call(dev, R.kernel_consts(c), d["pts"][sl], d["rep"][sl], d["rows"][sl], d["knn"][sl], c["D"], fx=_is_fx(name), **kw)


@functools.lru_cache(maxsize=None)
def _module_case(name):
    """A perturbed eval-mode stage, its plan and random inputs (on the device), shared by the tests that read them."""
    from pointcloudlib_amd.inference import _FusedXConvSeg, _xconv_seg_form
    from pointcloudlib_amd.misc.pointcnn import RandPointCNN, RandPointCNN_Decoder
    dev = torch.device("cuda:0")
    args = STAGE_ARGS[name]
    torch.manual_seed(200 + NAMES.index(name))
    st = (RandPointCNN(args[0], args[1], 3, *args[2:]) if len(args) == 5 else RandPointCNN_Decoder(args[0], args[1], args[2], 3, *args[3:])).to(dev)
    _perturb_all(_perturb(st, 17 + NAMES.index(name)), 170 + NAMES.index(name)).eval()
    form = _xconv_seg_form(st)
    assert form == ("fx" if _is_fx(name) else "taps")
    K = S.SHAPES[name][0]
    g = torch.Generator().manual_seed(NAMES.index(name))
    case = {"pts": torch.rand(B0, 40, 3, generator=g), "rep": torch.rand(B0, P0, 3, generator=g),
            "fts": torch.randn(B0, 40, args[0], generator=g), "knn": R.knn_lists(B0, K, P0, 40, g)}
    return st, _FusedXConvSeg(st, None, form), {k: v.to(dev) for k, v in case.items()}


def _rows(plan, fts):
    from pointcloudlib_amd.inference import _rows_gemm
    B, N, C = fts.shape
    return _rows_gemm(fts.reshape(B * N, C).contiguous(), plan.Wd, plan.bd, tag="pt").view(B, N, -1)


def _plan_consts(plan):
    return {k: getattr(plan, k) for k in ("fs", "ft", "Wa", "sa", "ta", "Wb", "sb", "tb", "W0", "W1", "sc1", "sh1", "W2", "b2", "wd", "bias")}


def _composite_raw(st, c):
    """The existing path on the same lists, up to the pointwise conv's output (its ReLU and BatchNorm aside)."""
    from pointcloudlib_amd.misc.ops import group_points, index_points
    from pointcloudlib_amd.misc.pointcnn import xconv_core
    pc, xc = st.pointcnn, st.pointcnn.x_conv
    idx = R.dilated(c["knn"], pc.D)
    B, P, K = idx.shape
    pw = copy.deepcopy(xc.end_conv.pointwise).eval()
    pw.last_act = False                                              # raw: the module's own GEMM without its ReLU
    with torch.no_grad():
        fts = pc.dense(c["fts"])
        local = group_points(c["pts"].contiguous(), c["rep"].contiguous(), None, idx, use_xyz=True).contiguous()
        regional = index_points(fts, idx)
        X = xc.x_trans_2(xc.x_trans_1(xc.x_trans_0(local))).reshape(B, P, K, K)
        return pw(xconv_core(X, xc.dense(local), regional, xc.end_conv.depthwise, xc.end_conv.depthwise_bias))


def _fused_raw(plan, c):
    """What ``_FusedXConvSeg.run`` does behind the neighbour search, on given lists."""
    B, N, _ = c["pts"].shape
    D = plan.contract(c["pts"], c["rep"], _rows(plan, c["fts"]).reshape(B * N, -1), c["knn"])
    return plan.pointwise(D).view(B, c["rep"].shape[1], -1)


# ------------------------------------------------------------------------------------------------- 1. exactly representable data
@pytest.mark.parametrize("name", NAMES)
def test_level_kernel_exact_data_bit_for_bit(dev, name):
    c, d = _exact(name, B0, _n0(name), P0)
    want = _ref_level(name)(c, d["pts"], d["rep"], d["rows"], R.dilated(d["knn"], c["D"]))
    got = _exact_call(dev, name, c, d)
    assert torch.equal(got.cpu(), want.float()), f"{int((got.cpu() != want.float()).sum())} of {want.numel()} outputs differ"
    assert torch.equal(_exact_call(dev, name, c, d), got), "two calls differ"


def test_fx_then_folded_gemm_exact_data_bit_for_bit(dev):
    """The FX launch and the GEMM with ``fold_taps``' weight against taps-then-pointwise in fp64 (nothing folded there)."""
    from pointcloudlib_amd.inference import _rows_gemm, fold_taps
    c, d = _exact("encoder_0", B0, _n0("encoder_0"), P0)
    want = R.level(c, d["pts"], d["rep"], d["rows"], R.dilated(d["knn"], 1)) @ c["Wp"].t()
    Wf, bf = fold_taps(c["wd"], c["bias"], c["Wp"])
    FX = _exact_call(dev, "encoder_0", c, d)
    got = _rows_gemm(FX.reshape(B0 * P0, -1).contiguous(), Wf.float().to(dev).contiguous(), bf.float().to(dev))
    assert float((want != 0).double().mean()) > 0.3
    assert torch.equal(got.cpu().view(want.shape), want.float())


# ------------------------------------------------------------------------------------------------- 2. the yardstick at raw
@pytest.mark.parametrize("name", NAMES)
def test_stage_against_fp64(dev, name):
    st, plan, c = _module_case(name)
    got = _fused_raw(plan, c)
    assert torch.equal(_fused_raw(plan, c), got), "two calls differ"
    want_eval = _composite_raw(st, c)
    ref, _ = R.stage(R.stage_consts(st), c["pts"], c["rep"], c["fts"], R.dilated(c["knn"], plan.D))
    assert got.shape == want_eval.shape == ref.shape
    assert float((ref != 0).double().mean()) > 0.3, "a trivial stage"
    e_fused, e_eval = _err(got, ref), _err(want_eval, ref)
    print(f"{name}: fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64 at raw (largest |value| {float(ref.abs().max()):.3e})")
    assert e_fused <= 1.25 * e_eval + 1e-6, f"fused {e_fused:.3e} vs composite {e_eval:.3e} from fp64"


# ------------------------------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("name", NAMES)
def test_level_kernel_regions_are_independent(dev, name):
    _, plan, c = _module_case(name)
    k = _plan_consts(plan)
    rows = _rows(plan, c["fts"])
    call = lambda pts, rep, rw, knn: S.level_call(dev, k, pts, rep, rw, knn, plan.D, fx=_is_fx(name))
    full = call(c["pts"], c["rep"], rows, c["knn"])
    one = call(c["pts"][1:2], c["rep"][1:2], rows[1:2], c["knn"][1:2])
    assert torch.equal(full[1:2], one), "cloud 1 alone differs from cloud 1 in the batch"
    perm = [2, 1, 0]                                                       # clouds 0 and 2 swapped: every region moves
    assert torch.equal(call(c["pts"][perm], c["rep"][perm], rows[perm], c["knn"][perm]), full[perm])
    gp = [0, 3, 2, 1, 4]                                                   # two regions of every cloud swapped
    assert torch.equal(call(c["pts"], c["rep"][:, gp], rows, c["knn"][:, :, gp]), full[:, gp])


# ------------------------------------------------------------------------------------------------- 4. several tiles per workgroup
# B * P = 16395 regions, just past 8 * 16 * 128: on an MI355X (two workgroups per compute unit wanted at K = 8 and 12) a workgroup
# of the large launch owns more tiles than one of a B = 1 launch; B * P is odd, so the last tile is partly filled
MANY = (5, 3279)


@pytest.mark.parametrize("name", NAMES)
def test_level_kernel_many_tiles_per_workgroup(dev, name):
    from pointcloudlib_amd import _lib
    B, P = MANY
    K = S.SHAPES[name][0]
    rt_all, rt_one = (_lib.lib().pcl_xconv_level_infer_region_tile(K, n) for n in (B * P, P))
    assert rt_all > rt_one >= 16, f"workgroups own {rt_all} regions in the large launch, {rt_one} in the B = 1 launch"
    c, d = _exact(name, B, _n0(name), P)
    full = _exact_call(dev, name, c, d)
    assert bool(torch.isfinite(full).all())
    for b in range(B):
        assert torch.equal(full[b:b + 1], _exact_call(dev, name, c, d, slice(b, b + 1))), f"cloud {b} alone differs from cloud {b} in the batch"
    for b, sl in ((0, slice(0, 100)), (B - 1, slice(P - 100, P))):
        audit = []
        want = _ref_level(name)(c, d["pts"][b:b + 1], d["rep"][b:b + 1, sl], d["rows"][b:b + 1], R.dilated(d["knn"][b:b + 1, :, sl], c["D"]), audit=audit)
        assert max(audit) < 2.0 ** 24 and float((want != 0).double().mean()) > 0.3
        assert torch.equal(full[b:b + 1, sl].cpu(), want.float()), f"cloud {b}, regions {sl}: differs from fp64"


# ------------------------------------------------------------------------------------------------- 5. guard columns
@pytest.mark.parametrize("name", NAMES)
def test_level_kernel_leaves_guard_columns(dev, name):
    """``level_call`` fills ``out`` with a marker and asserts that everything behind a row's columns kept it; here with no guard
    columns beyond the rounding to a multiple of 4 (decoder_3: ldo = 40), with 8 (ldo = 48) and with 36 -- the same bits."""
    c, d = _exact(name, B0, _n0(name), P0)
    outs = [_exact_call(dev, name, c, d, guard=g) for g in (0, 8, 36)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    if name == "decoder_3":
        assert outs[0].shape[-1] == 37


# ------------------------------------------------------------------------------------------------- 6. decoder geometry
@pytest.mark.parametrize("name", ["encoder_1", "decoder_3"])
def test_level_kernel_more_representatives_than_points(dev, name):
    """P > N, as a decoder has it (representatives: the finer level's points): exact data, 2 x 29 regions from 2 x 15 points."""
    c, d = _exact(name, 2, 15, 29)
    want = R.level(c, d["pts"], d["rep"], d["rows"], R.dilated(d["knn"], c["D"]))
    assert torch.equal(_exact_call(dev, name, c, d).cpu(), want.float())


def test_decoder_stage_through_the_evaluator_plan(dev):
    """``_FusedXConvSeg.run`` and ``_FuseConv`` on a decoder with 50 fine points over 24 coarse ones, with the GPU's own lists."""
    from pointcloudlib_amd.inference import _FuseConv, _FusedXConvSeg
    from pointcloudlib_amd.misc.ops import knn_indices
    st, _, _ = _module_case("decoder_3")
    g = torch.Generator().manual_seed(9)
    B, N, P = 2, 24, 50
    pts_l, pts_h = torch.rand(B, N, 3, generator=g).to(dev), torch.rand(B, P, 3, generator=g).to(dev)
    fts_l, raw_h = torch.randn(B, N, 256, generator=g).to(dev), torch.randn(B, P, 256, generator=g).to(dev)
    sk = (torch.rand(256, generator=g).double().to(dev) + 0.5, torch.randn(256, generator=g).double().to(dev) * 0.1)
    plan = _FusedXConvSeg(st, None, "taps")
    fuse = _FuseConv(st.conv_fuse, [plan.out_affine, sk])
    raw = plan.run(pts_l, pts_h, fts_l.reshape(B * N, -1))
    got = fuse.run(raw, raw_h.reshape(B * P, -1)).view(B, P, -1)
    fts_h = sk[0].float() * torch.relu(raw_h) + sk[1].float()
    with torch.no_grad():
        _, want_eval = st((pts_l, fts_l), (pts_h, fts_h))
    knn = knn_indices(pts_h.transpose(1, 2).contiguous(), pts_l.transpose(1, 2).contiguous(), 8)
    fts_h64 = sk[0] * raw_h.double().clamp(min=0) + sk[1]
    _, ref = S.decoder_stage(S.decoder_consts(st), pts_l, fts_l, pts_h, fts_h64, R.dilated(knn, 1))
    e_fused, e_eval = _err(got, ref), _err(want_eval, ref)
    print(f"decoder_3 with conv_fuse: fused {e_fused:.3e} vs module {e_eval:.3e} from fp64")
    assert got.shape == (B, P, 50) and float((ref != 0).double().mean()) > 0.2
    assert e_fused <= 1.25 * e_eval + 1e-6


# ------------------------------------------------------------------------------------------------- 7.-10. the network
@functools.lru_cache(maxsize=None)
def _net(seed=0):
    from pointcloudlib_amd.networks.seg.pointcnn_partseg import PointCNN_partseg
    torch.manual_seed(seed)
    net = PointCNN_partseg().to("cuda:0")
    return _perturb_all(_perturb(net, seed + 1), seed + 2)


def _clouds(dev, B, N, seed=0):
    from pointcloudlib_amd import synth
    return torch.from_numpy(synth.gauss_ball(B, N, seed)).to(dev).contiguous()


def _eval_run(net, x):
    """The existing evaluation path (net.eval() + no_grad) on a copy, stage by stage -> (features, logits, the GPU's own
    representatives of the encoders and the k-NN lists of every stage)."""
    ev = copy.deepcopy(net).eval()
    T = lambda t: t.transpose(1, 2).contiguous()
    feats, reps, knns, lv = [], [], [], []
    with torch.no_grad():
        cur = (x, x)
        for name in S.ENCODERS:
            st = getattr(ev, name)
            rep, f = st(cur)
            knns.append(st.pointcnn.knn(T(rep), T(cur[0])))
            cur = (rep, f)
            lv.append(cur)
            reps.append(rep)
            feats.append(f)
        low = lv[3]
        for j, name in enumerate(S.DECODERS):
            st = getattr(ev, name)
            ph, f = st(low, lv[3 - j])
            knns.append(st.pointcnn.knn(T(ph), T(low[0])))
            low = (ph, f)
            feats.append(f)
        return feats, ev(x), reps, knns


@functools.lru_cache(maxsize=None)
def _network_case():
    """One frozen run, one eval run and one fp64 evaluation at B = 2, N = 1024 (FPS runs at 768, 384 and 128), shared."""
    from pointcloudlib_amd.inference import FrozenPointCNNPartseg
    dev = torch.device("cuda:0")
    net = _net()
    x = _clouds(dev, 2, 1024)
    fnet = FrozenPointCNNPartseg(net)
    feats, logits = fnet.run(x)
    ev_feats, ev_logits, reps, knns = _eval_run(net, x)
    ref_feats, _, ref_logits = S.network(net, x, reps, knns)
    torch.cuda.synchronize()
    return fnet, x, (feats, logits), (ev_feats, ev_logits), (ref_feats, ref_logits)


def test_frozen_partseg_against_fp64(dev):
    fnet, x, (feats, logits), (ev_feats, ev_logits), (ref_feats, ref_logits) = _network_case()
    assert torch.equal(fnet(x), logits)
    assert logits.shape == (2, 50, 1024)
    assert [tuple(f.shape[1:]) for f in feats] == [(1024, 256), (768, 256), (384, 512), (128, 1024), (128, 1024), (384, 512), (768, 256), (1024, 50)]
    assert all(float((r != 0).double().mean()) > 0.2 for r in ref_feats), "a trivial stage"
    for i, (f, e, r) in enumerate(zip(feats + [logits], ev_feats + [ev_logits], ref_feats + [ref_logits])):
        what = (S.ENCODERS + S.DECODERS + ("logits",))[i]
        assert f.shape == e.shape == r.shape, (what, f.shape, e.shape, r.shape)
        ef, ee = _err(f, r), _err(e, r)
        print(f"{what}: frozen {ef:.3e} vs eval {ee:.3e} from fp64 (largest |value| {float(r.abs().max()):.3e})")
        assert ef <= 1.25 * ee + 1e-6, f"{what}: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    agree = float((logits.argmax(1) == ev_logits.argmax(1)).float().mean())
    print(f"per-point argmax agreement with net.eval(): {agree:.4f} of {logits.shape[0] * logits.shape[2]} points "
          f"(with fp64: frozen {float((logits.argmax(1) == ref_logits.argmax(1)).float().mean()):.4f}, "
          f"eval {float((ev_logits.argmax(1) == ref_logits.argmax(1)).float().mean()):.4f})")


def test_frozen_partseg_plans(dev):
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.inference import FrozenPointCNNPartseg
    from test_inference_pointcnn_partseg_cpu import NET_SHAPES
    fnet = _network_case()[0]
    lib = _lib.lib()
    assert [fnet.levels[i] for i in (0, 1, 6, 7)] == ["fused"] * 4
    for i in (2, 3, 4, 5):
        assert fnet.levels[i] == ("fused" if lib.pcl_xconv_level_infer_supported(*NET_SHAPES[i]) else "module"), i
    # a stage with a part that is not the stock one runs as its module: the lift of encoder_1 with a leaky ReLU
    net = copy.deepcopy(_net())
    net.encoder_1.pointcnn.x_conv.dense.slope = 0.25
    other = FrozenPointCNNPartseg(net)
    assert other.levels == ["fused", "module"] + fnet.levels[2:]
    x = _clouds(dev, 2, 256, seed=5)
    feats, logits = other.run(x)
    with torch.no_grad():
        _, want1 = copy.deepcopy(net.encoder_1).eval()((x, feats[0]))
    # the module plan is that module on the features the fused encoder_0 hands on: the same kernels on the same inputs
    assert _err(feats[1], want1.double()) <= 1e-5 * float(want1.abs().max())
    assert logits.shape == (2, 50, 256) and bool(torch.isfinite(logits).all())
    assert not torch.equal(feats[1], FrozenPointCNNPartseg(_net()).run(x)[0][1])


def test_frozen_partseg_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointCNNPartseg
    net = copy.deepcopy(_net()).train()
    x = _clouds(dev, 2, 256, seed=3)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = FrozenPointCNNPartseg(net)
    out = fnet(x)
    torch.cuda.synchronize()
    assert out.shape == (2, 50, 256)
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(fnet(x, x), out)                                   # ``normal`` is ignored, as by net.forward
    with torch.no_grad():
        net.encoder_0.pointcnn.x_conv.end_conv.depthwise.mul_(1.5)        # inside the folded taps
        net.decoder_3.conv_fuse.mlp.running_mean_0.add_(0.25)
    stale = fnet(x)
    fresh = fnet.refresh()(x)
    torch.cuda.synchronize()
    assert torch.equal(stale, out)
    assert not torch.equal(fresh, out)
    assert torch.equal(fresh, FrozenPointCNNPartseg(net)(x))
    with pytest.raises(ValueError, match="fp32 only"):
        FrozenPointCNNPartseg(net, precision="bf16")
    with pytest.raises(ValueError, match=r"\[B,N,3\]"):
        fnet(x.transpose(1, 2))


def test_frozen_partseg_forward_memory(dev):
    """Peak allocation during a frozen forward at B = 2, N = 1024, above the allocation before it, stays below the bytes of
    encoder_0's D alone, B * N * 16512 * 4 = 135 MB -- the tensor the fold removes."""
    fnet, x = _network_case()[:2]
    B, N = x.shape[:2]
    fnet(x)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fnet(x)
    torch.cuda.synchronize()
    assert out.shape == (B, 50, N)
    del out
    peak = torch.cuda.max_memory_allocated() - base
    bound = B * N * 16512 * 4
    print(f"peak of a frozen forward: +{peak / 2**20:.1f} MiB, encoder_0's D alone {bound / 2**20:.1f} MiB")
    assert peak < bound
