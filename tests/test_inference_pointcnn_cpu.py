"""Frozen inference for PointCNN classification (pointcloudlib_amd/inference.py: FrozenPointCNN, csrc/infer_xconv.hip): the parts
that need no GPU -- the data of the GPU file's bit-for-bit tests, the folds of the evaluator against the unfolded fp64 restatement
of tests/pointcnn_infer_ref.py, the ABI."""
import ctypes

import pytest
import torch

import pointcnn_infer_ref as R

# (stage, B, N, P, seed): the shapes of tests/test_inference_pointcnn_gpu.py
EXACT_CASES = [(s, 3, 40, 5, 0) for s in (1, 2, 3, 4)]
SYMBOLS = ("pcl_xconv_level_infer_f32", "pcl_xconv_level_infer_supported", "pcl_xconv_level_infer_region_tile")


def _perturb_all(net, seed):
    """Every BatchNorm of a PointCNN (the PointwiseMLPs' and the ``_BatchNormLast`` behind ``Conv`` / ``SepConv``) away from its
    initial values, a fifth of the gammas negative."""
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.misc.pointcnn import _BatchNormLast
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in net.modules():
            pairs = []
            if isinstance(mod, PointwiseMLP) and mod.bn:
                pairs = [(mod.gammas[l], mod.betas[l], getattr(mod, f"running_mean_{l}"), getattr(mod, f"running_var_{l}")) for l in range(mod.n_layers)]
            elif isinstance(mod, _BatchNormLast):
                pairs = [(mod.weight, mod.bias, mod.running_mean, mod.running_var)]
            for gam, bet, rm, rv in pairs:
                c = gam.numel()
                gam.copy_(torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0) * (0.5 + torch.rand(c, generator=g)))
                bet.copy_(0.1 * torch.randn(c, generator=g))
                rm.copy_(0.1 * torch.randn(c, generator=g))
                rv.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return net


def test_xconv_infer_symbols_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.declared_symbols()
        assert hasattr(lib, name)


def test_xconv_infer_supported_is_the_four_stages():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    stages = {(K, CM, C2, dm) for K, _, CM, C2, dm in R.STAGES.values()}
    assert stages == {(8, 12, 24, 16), (12, 24, 48, 2), (16, 48, 96, 2), (16, 96, 192, 2)}
    values = {"K": (0, 4, 8, 12, 16, 32), "CM": (0, 12, 16, 24, 48, 96, 192), "C2": (0, 24, 32, 48, 96, 192, 384), "dm": (1, 2, 4, 16)}
    hits = set()
    for K in values["K"]:
        for CM in values["CM"]:
            for C2 in values["C2"]:
                for dm in values["dm"]:
                    if lib.pcl_xconv_level_infer_supported(K, CM, C2, dm):
                        hits.add((K, CM, C2, dm))
    assert hits == stages


def test_xconv_infer_region_tile():
    """Whole 16-region tiles, at most 8 of them, never fewer than one; 0 for a K without a kernel."""
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for K in (8, 12, 16):
        assert lib.pcl_xconv_level_infer_region_tile(K, 1) == 16
        assert lib.pcl_xconv_level_infer_region_tile(K, 1 << 22) == 128
        for Rg in (15, 1639, 8195, 32768):
            rt = lib.pcl_xconv_level_infer_region_tile(K, Rg)
            assert rt % 16 == 0 and 16 <= rt <= 128
    assert lib.pcl_xconv_level_infer_region_tile(10, 100) == 0 and lib.pcl_xconv_level_infer_region_tile(16, 0) == 0


def test_xconv_infer_launcher_rejects_other_shapes_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.pcl_xconv_level_infer_f32(p, p, p, p, p, p, 1, 40, 5, 8, 1, 16, 24, 16, *([p] * 15), 576, None)
    assert rc == -1 and b"no kernel" in lib.pcl_last_error()


def test_frozen_pointcnn_interface_without_a_gpu():
    import pointcloudlib_amd.inference as inference
    from pointcloudlib_amd.networks.cls.pointcnn import PointCNNcls
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    assert "FrozenPointCNN" in inference.__all__ and "FrozenPointCNN" in inference.__doc__
    with pytest.raises(TypeError, match="PointCNNcls"):
        inference.FrozenPointCNN(PointNet())
    with pytest.raises(ValueError, match="fp32 only"):
        inference.FrozenPointCNN(PointCNNcls(), precision="bf16")
    net = PointCNNcls()
    fnet = inference.FrozenPointCNN(net)
    assert fnet.levels == ["fused"] * 4 and net.training


@pytest.mark.parametrize("s,B,N,P,seed", EXACT_CASES)
def test_exact_cases_are_exact(s, B, N, P, seed):
    """The data of the GPU file's bit-for-bit tests: every dot product's sum of |products| stays below 2^24 granules (so every
    partial sum, in any order, is an fp32 number), the folded constants the kernel is given are fp32 numbers, the fp32 and fp64
    evaluations of the restatement agree bit for bit, and the result is no trivial one."""
    c, d = R.exact_case(s, B, N, P, seed)
    K, D = c["K"], c["D"]
    args = (c, d["pts"], d["rep"], d["rows"], R.dilated(d["knn"], D))
    audit = []
    want = R.level(*args, audit=audit)
    assert max(audit) < 2.0 ** 24, audit
    assert torch.equal(R.level(*args, dtype=torch.float32).double(), want)
    assert torch.equal(want.float().double(), want)
    assert float((want != 0).double().mean()) > 0.3 and want.unique().numel() > 100
    for name, t in R.kernel_consts(c).items():
        assert torch.equal(t.float().double(), t), name
    assert d["knn"].shape == (B, K * D, P) and int(d["knn"].min()) == 0 and int(d["knn"].max()) == N - 1


@pytest.fixture(scope="module")
def net():
    from pointcloudlib_amd.networks.cls.pointcnn import PointCNNcls
    torch.manual_seed(0)
    return _perturb_all(PointCNNcls(), 1)


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_xtrans_fold_against_the_unfolded_restatement(net, i):
    """``x_trans_0``'s BatchNorm folded into ``x_trans_1`` (inference.fold_xtrans), evaluated in fp64, against the three layers as
    the module writes them."""
    from pointcloudlib_amd.inference import fold_xtrans
    st = ([net.pcnn1] + list(net.pcnn2))[i]
    c = R.stage_consts(st)
    K = c["K"]
    g = torch.Generator().manual_seed(10 + i)
    p = (torch.rand(200, 3 * K, generator=g).double() - 0.5)
    want = R.dense_layer(R.dense_layer(R.conv_layer(p, c["x0"]), c["x1"]), c["x2"], act=False)
    W0, W1, sc1, sh1, W2, b2 = fold_xtrans(st.pointcnn.x_conv)
    got = (sc1 * ((p @ W0.t()).clamp(min=0) @ W1.t()) + sh1).clamp(min=0) @ W2.t() + b2
    assert float(want.abs().max()) > 0.1
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    k = R.kernel_consts(c)                                   # the helper's own fold is the same map
    assert all(float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()) for a, b in ((k["W1"], W1), (k["sh1"], sh1)))


def test_output_affine_folds_against_the_unfolded_restatement(net):
    """A stage's trailing affine ``s * relu(raw) + t`` folded into the next stage's ``dense`` and into the head's first layer
    (inference.fold_affine_into_linear, as FrozenPointCNN.refresh() applies it), evaluated in fp64."""
    from pointcloudlib_amd.inference import FrozenPointCNN, fold_affine_into_linear
    stages = [net.pcnn1] + list(net.pcnn2)
    g = torch.Generator().manual_seed(20)
    readers = [st.pointcnn.dense.mlp for st in stages[1:]] + [net.fcn[0].mlp]
    for st, reader in zip(stages, readers):
        c = R.stage_consts(st)
        s, t = c["out"]
        raw = torch.randn(300, s.numel(), generator=g).double()
        W, b, _, _ = R.mlp_layer(reader, 0)
        want = (s * raw.clamp(min=0) + t) @ W.t() + b
        Wf, bf = fold_affine_into_linear(reader.weights[0], reader.biases[0], s, t)
        got = raw.clamp(min=0) @ Wf.t() + bf
        assert float(want.abs().max()) > 0.1
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # what refresh() keeps is that fold rounded once to fp32
    fnet = FrozenPointCNN(net)
    for i, (st, reader) in enumerate(zip(stages, readers)):
        Wf, bf = fold_affine_into_linear(reader.weights[0], reader.biases[0], *R.stage_consts(st)["out"])
        kept = (fnet.plans[i + 1][1].Wd, fnet.plans[i + 1][1].bd) if i < 3 else (fnet.hW[0], fnet.hb[0])
        assert torch.equal(kept[0], Wf.float()) and torch.equal(kept[1], bf.float())
