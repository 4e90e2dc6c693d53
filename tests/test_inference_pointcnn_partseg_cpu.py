"""Frozen inference for PointCNN part segmentation (pointcloudlib_amd/inference.py: FrozenPointCNNPartseg, csrc/infer_xconv.h,
csrc/infer_xconv_seg.hip): the parts that need no GPU -- the fold of the depthwise taps into the pointwise conv and of the two
trailing affines into ``conv_fuse`` against the unfolded fp64 restatement of tests/pointcnn_partseg_infer_ref.py, the data of the
GPU file's bit-for-bit tests, the ABI."""
import ctypes

import pytest
import torch

import pointcnn_infer_ref as R
import pointcnn_partseg_infer_ref as S
from test_inference_pointcnn_cpu import _perturb_all

SYMBOLS = ("pcl_xconv_level_infer_fx_f32", "pcl_xconv_level_infer_fx_supported")
# (shape, B, N = K*D + 3, P, seed): the cases of tests/test_inference_pointcnn_partseg_gpu.py, its decoder geometry (P > N) included
EXACT_CASES = [(name, 3, K * D + 3, 5, 0) for name, (K, D, _, _, _) in S.SHAPES.items()] + [("encoder_1", 2, 15, 29, 0), ("decoder_3", 2, 15, 29, 0)]
# (K, C_mid, C2, dm) of the eight stages of PointCNN_partseg(part_num=50), encoder_0 .. 3, decoder_0 .. 3
NET_SHAPES = [(8, 64, 128, 86), (12, 64, 128, 1), (16, 128, 256, 2), (16, 256, 512, 2), (16, 256, 512, 1), (16, 128, 256, 1), (12, 64, 128, 1), (8, 12, 25, 1)]
U64 = 2.0 ** -53


def test_symbols_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)


def test_the_network_has_the_shapes_of_the_table():
    from pointcloudlib_amd.networks.seg.pointcnn_partseg import PointCNN_partseg
    net = PointCNN_partseg()
    got = []
    for name in S.ENCODERS + S.DECODERS:
        pc = getattr(net, name).pointcnn
        got.append((pc.K, pc.x_conv.C_mid, pc.x_conv.C_in, pc.x_conv.end_conv.dm))
        assert pc.D == 1
    assert got == NET_SHAPES
    assert [NET_SHAPES[i] for i in (0, 1, 7)] == [(K, CM, C2, dm) for K, _, CM, C2, dm in S.SHAPES.values()]


def test_supported_queries():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert lib.pcl_xconv_level_infer_fx_supported(8, 64, 128) == 1
    assert [s for s in [(8, 64, 128), (12, 64, 128), (8, 12, 25), (8, 12, 24), (8, 64, 64), (16, 64, 128), (0, 0, 0)] if lib.pcl_xconv_level_infer_fx_supported(*s)] == [(8, 64, 128)]
    assert lib.pcl_xconv_level_infer_supported(12, 64, 128, 1) == 1 and lib.pcl_xconv_level_infer_supported(8, 12, 25, 1) == 1
    # the FX shape has no tap form (dm = 0 names no tap kernel either), dm is part of a tap shape, the cls shapes stay
    for q in [(8, 64, 128, 0), (8, 64, 128, 86), (8, 64, 128, 1), (12, 64, 128, 2), (8, 12, 25, 2), (8, 12, 24, 1), (12, 64, 128, 0)]:
        assert lib.pcl_xconv_level_infer_supported(*q) == 0, q
    assert lib.pcl_xconv_level_infer_supported(8, 12, 24, 16) == 1
    # a K = 16 stage of the network answers 0 or 1; the evaluator's plan follows the answer (the GPU file checks that)
    for q in NET_SHAPES[2:6]:
        assert lib.pcl_xconv_level_infer_supported(*q) in (0, 1)


def test_launchers_reject_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fx = lambda K, CM, C2, ldo: lib.pcl_xconv_level_infer_fx_f32(p, p, p, p, p, p, 1, 40, 5, K, 1, CM, C2, *([p] * 13), ldo, None)
    assert fx(8, 64, 120, 1536) == -1 and b"no kernel" in lib.pcl_last_error() and b"fx_supported" in lib.pcl_last_error()
    assert fx(12, 64, 128, 2304) == -1 and b"no kernel" in lib.pcl_last_error()
    assert fx(8, 64, 128, 1532) == -1 and b"ldo" in lib.pcl_last_error()             # fewer than K*C columns
    assert fx(8, 64, 128, 1538) == -1 and b"ldo" in lib.pcl_last_error()             # no multiple of 4
    taps = lambda K, CM, C2, dm, ldo: lib.pcl_xconv_level_infer_f32(p, p, p, p, p, p, 1, 40, 5, K, 1, CM, C2, dm, *([p] * 15), ldo, None)
    assert taps(8, 12, 25, 1, 37) == -1 and b"ldo" in lib.pcl_last_error()           # 37 columns need ldo >= 40
    assert taps(8, 64, 128, 0, 1536) == -1 and b"no kernel" in lib.pcl_last_error()  # dm = 0 is the FX entry's alone


def test_interface_without_a_gpu():
    import pointcloudlib_amd.inference as inference
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.networks.cls.pointcnn import PointCNNcls
    from pointcloudlib_amd.networks.seg.pointcnn_partseg import PointCNN_partseg
    assert "FrozenPointCNNPartseg" in inference.__all__ and "FrozenPointCNNPartseg" in inference.__doc__ and "fold_taps" in dir(inference)
    with pytest.raises(TypeError, match="PointCNN_partseg"):
        inference.FrozenPointCNNPartseg(PointCNNcls())
    with pytest.raises(ValueError, match="fp32 only"):
        inference.FrozenPointCNNPartseg(PointCNN_partseg(), precision="bf16")
    net = PointCNN_partseg()
    fnet = inference.FrozenPointCNNPartseg(net)
    lib = _lib.lib()
    want = ["fused" if lib.pcl_xconv_level_infer_supported(*s) else "module" for s in NET_SHAPES]
    want[0] = "fused"
    assert fnet.levels == want and [want[i] for i in (0, 1, 6, 7)] == ["fused"] * 4
    assert fnet.plans[0][1].form == "fx" and all(fnet.plans[i][1].form == "taps" for i in (1, 6, 7))
    assert net.training and all(m.training for m in net.modules())
    assert fnet.plans[0][1].Wf.shape == (256, 8 * 192) and fnet.plans[7][1].Wp.shape == (50, 40)
    assert [f is not None and f.folded for f in fnet.fuses] == [k == "fused" for k in want[4:]]


# ------------------------------------------------------------------------------------------------- the folds
def _two_steps(wd, bias_d, Wp, FX):
    """Taps, then the pointwise conv, in fp64: FX [R, K, C] -> raw [R, C_out]."""
    C, dm, K = wd.shape
    D = torch.einsum("rkc,cjk->rcj", FX, wd).reshape(FX.shape[0], C * dm) + bias_d
    return D @ Wp.t()


@pytest.mark.parametrize("C,dm,K,Cout", [(192, 86, 8, 256), (36, 16, 8, 48), (5, 3, 4, 7)])
def test_fold_taps_against_taps_then_pointwise(C, dm, K, Cout):
    """Both sides sum the same C*dm*(K+1) products per output in another association.  In fp64 (unit roundoff u = 2^-53) a sum of n
    terms in ANY order, products rounded, is within (n + 1) u * (sum of |terms|) of the exact value to first order.  The two-step
    side chains K + 1 terms (taps, bias) and then C*dm terms; the folded side dm terms (Wf), then K*C + 1 terms, and rounds bf's C*dm
    terms.  So |folded - two-step| <= 1.01 * u * [(K + 2 + C*dm + 1) + (dm + 1 + K*C + 2 + C*dm + 1)] * S with S[o] = sum_{c,j}
    |Wp| (|bias| + sum_k |wd| |FX|) -- the bound asserted, per output."""
    from pointcloudlib_amd.inference import fold_taps
    g = torch.Generator().manual_seed(C + dm)
    wd = torch.rand(C, dm, K, generator=g).double() - 0.5
    bias_d = torch.rand(C * dm, generator=g).double() - 0.5
    Wp = torch.randn(Cout, C * dm, generator=g).double() / (C * dm) ** 0.5
    FX = torch.randn(50, K, C, generator=g).double()
    Wf, bf = fold_taps(wd, bias_d, Wp)
    assert Wf.shape == (Cout, K * C) and bf.shape == (Cout,) and Wf.dtype == bf.dtype == torch.float64
    want = _two_steps(wd, bias_d, Wp, FX)
    got = FX.reshape(50, K * C) @ Wf.t() + bf
    S_ = _two_steps(wd.abs(), bias_d.abs(), Wp.abs(), FX.abs())
    n = (K + 2 + C * dm + 1) + (dm + 1 + K * C + 2 + C * dm + 1)
    assert float(want.abs().max()) > 0.1
    excess = (got - want).abs() - 1.01 * U64 * n * S_
    print(f"C={C} dm={dm} K={K}: |folded - two-step| max {float((got - want).abs().max()):.3e}, bound min {float((1.01 * U64 * n * S_).min()):.3e}")
    assert float(excess.max()) <= 0.0
    # the column order: k*C + c
    k, c, o = K - 1, C // 2, Cout - 1
    assert float(Wf[o, k * C + c] - (Wp[o, c * dm:(c + 1) * dm] * wd[c, :, k]).sum()) == pytest.approx(0.0, abs=1e-15)


def test_fold_taps_is_exact_on_exact_data():
    from pointcloudlib_amd.inference import fold_taps
    c, d = S.exact_case("encoder_0", 3, 40, 5, 0)
    Wf, bf = fold_taps(c["wd"], c["bias"], c["Wp"])
    assert torch.equal(Wf.float().double(), Wf) and torch.equal(bf.float().double(), bf)
    assert S.granule(Wf) >= 0.25 and float((Wf != 0).double().mean()) > 0.01
    FX = S.level_fx(c, d["pts"], d["rep"], d["rows"], R.dilated(d["knn"], 1))
    K, C = c["K"], c["wd"].shape[0]
    want = _two_steps(c["wd"], c["bias"], c["Wp"], FX.reshape(-1, K, C))
    assert torch.equal(FX.reshape(-1, K * C) @ Wf.t() + bf, want)


@pytest.mark.parametrize("name,B,N,P,seed", EXACT_CASES)
def test_exact_cases_are_exact(name, B, N, P, seed):
    """The data of the GPU file's bit-for-bit tests: every dot product's sum of |products| stays below 2^24 granules -- for the FX
    shape the contraction with the folded weight too --, the constants the kernel is given are fp32 numbers, fp32 and fp64
    evaluations of the restatement agree bit for bit, and the result is no trivial one."""
    from pointcloudlib_amd.inference import fold_taps
    c, d = S.exact_case(name, B, N, P, seed)
    args = (c, d["pts"], d["rep"], d["rows"], R.dilated(d["knn"], c["D"]))
    fx = name in S.FX_SHAPES
    fn = S.level_fx if fx else R.level
    audit = []
    want = fn(*args, audit=audit)
    if fx:
        Wf, bf = fold_taps(c["wd"], c["bias"], c["Wp"])
        big = want.abs() @ Wf.abs().t() + bf.abs()
        audit.append(float(big.max()) / min(S.granule(want) * S.granule(Wf), S.granule(bf)))
    assert max(audit) < 2.0 ** 24, audit
    assert torch.equal(fn(*args, dtype=torch.float32).double(), want)
    assert torch.equal(want.float().double(), want)
    assert float((want != 0).double().mean()) > 0.3 and want.unique().numel() > 100
    for n, t in R.kernel_consts(c).items():
        assert torch.equal(t.float().double(), t), n
    K = c["K"]
    assert d["knn"].shape == (B, K, P) and int(d["knn"].min()) == 0 and int(d["knn"].max()) == N - 1


@pytest.fixture(scope="module")
def net():
    from pointcloudlib_amd.networks.seg.pointcnn_partseg import PointCNN_partseg
    torch.manual_seed(0)
    return _perturb_all(PointCNN_partseg(), 1)


@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_conv_fuse_fold_against_the_unfolded_restatement(net, j):
    """``conv_fuse`` on ``cat(s_a relu(raw_a) + t_a, s_s relu(raw_s) + t_s)`` as the module writes it against the folded weight on
    ``relu(cat(raw_a, raw_s))`` (inference.fold_conv_fuse), both in fp64; and what ``_FuseConv`` keeps is that fold rounded once."""
    from pointcloudlib_amd.inference import _FuseConv, fold_conv_fuse
    dec, enc = getattr(net, S.DECODERS[j]), getattr(net, S.ENCODERS[3 - j])
    c = S.decoder_consts(dec)
    aff = [c["out"], R.stage_consts(enc)["out"]]
    g = torch.Generator().manual_seed(30 + j)
    raw_a, raw_s = (torch.randn(200, a[0].numel(), generator=g).double() for a in aff)
    feats = [s * r.clamp(min=0) + t for r, (s, t) in zip((raw_a, raw_s), aff)]
    want = R.dense_layer(torch.cat(feats, dim=1), c["fuse"])
    W, b = fold_conv_fuse(dec.conv_fuse, aff)
    _, _, sc, sh = c["fuse"]
    got = (sc * (torch.cat((raw_a, raw_s), dim=1).clamp(min=0) @ W.t() + b) + sh).clamp(min=0)
    assert W.shape == c["fuse"][0].shape and float(want.abs().max()) > 0.1
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    kept = _FuseConv(dec.conv_fuse, aff)
    assert kept.folded and torch.equal(kept.W, W.float()) and torch.equal(kept.b, b.float())
    plain = _FuseConv(dec.conv_fuse, [aff[0], None])
    assert not plain.folded and torch.equal(plain.W, dec.conv_fuse.mlp.weights[0].detach())


def test_refresh_keeps_the_folds_rounded_once(net):
    from pointcloudlib_amd.inference import FrozenPointCNNPartseg, fold_affine_into_linear, fold_taps
    fnet = FrozenPointCNNPartseg(net)
    ec = net.encoder_0.pointcnn.x_conv.end_conv
    Wf, bf = fold_taps(ec.depthwise, ec.depthwise_bias, ec.pointwise.weights[0])
    p0, p1 = fnet.plans[0][1], fnet.plans[1][1]
    assert torch.equal(p0.Wf, Wf.float()) and torch.equal(p0.bf, bf.float())
    d1 = net.encoder_1.pointcnn.dense.mlp
    Wd, bd = fold_affine_into_linear(d1.weights[0], d1.biases[0], *R.stage_consts(net.encoder_0)["out"])
    assert p1.folded and torch.equal(p1.Wd, Wd.float()) and torch.equal(p1.bd, bd.float())
    assert not fnet.plans[6][1].folded and not fnet.plans[7][1].folded              # a decoder's dense reads stored features
