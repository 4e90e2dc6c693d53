"""Frozen inference for PointConv classification (pointcloudlib_amd/inference.py: FrozenPointConv, csrc/infer_pointconv.hip): the
parts that need no GPU.  (The modules' own forward has no CPU path, so the comparison of the folded WeightNet / DensityNet
constants with the modules' eval outputs is in tests/test_inference_pointconv_gpu.py; here they are held to the fp64 restatement.)"""
import ctypes

import pytest
import torch

import pointconv_infer_ref as R

# (ns, widths, point features, B, N, m, seed): the two shapes of tests/test_inference_pointconv_gpu.py
EXACT_CASES = [(32, [64, 64, 128], 0, 3, 40, 5, 0), (64, [128, 128, 256], 128, 2, 70, 3, 0)]


def test_pointconv_infer_symbols_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for name in ("pcl_pointconv_level_infer_f32", "pcl_pointconv_level_infer_supported", "pcl_pointconv_level_infer_group_tile"):
        assert name in _lib.declared_symbols()
        assert name in _lib._SIGS
        assert hasattr(lib, name)
    assert _lib.define("PCL_POINTCONV_NETS_FLOATS") == 400


def test_pointconv_infer_supported_shapes():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert lib.pcl_pointconv_level_infer_supported(32, 3, 64, 64, 128, 16) == 1
    assert lib.pcl_pointconv_level_infer_supported(64, 3, 128, 128, 256, 16) == 1
    assert lib.pcl_pointconv_level_infer_supported(64, 3, 128, 128, 288, 16) == 0
    assert lib.pcl_pointconv_level_infer_supported(64, 2, 128, 128, 256, 16) == 0
    assert lib.pcl_pointconv_level_infer_supported(64, 3, 128, 128, 256, 8) == 0
    assert lib.pcl_pointconv_level_infer_supported(0, 3, 64, 64, 128, 16) == 0
    assert lib.pcl_pointconv_level_infer_supported(32, 3, 128, 128, 256, 16) == 0        # a kernel is one (ns, widths) pair


def test_pointconv_infer_group_tile():
    """Whole tiles, at most 8 of them, never more than the launch has; 0 for an ns without a kernel."""
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for ns in (32, 64):
        gpt = 64 // ns
        assert lib.pcl_pointconv_level_infer_group_tile(ns, 1) == gpt
        big = lib.pcl_pointconv_level_infer_group_tile(ns, 1 << 20)
        assert big == 8 * gpt
        for G in (15, 1639, 8195, 16384):
            gt = lib.pcl_pointconv_level_infer_group_tile(ns, G)
            assert gt % gpt == 0 and gpt <= gt <= big
    assert lib.pcl_pointconv_level_infer_group_tile(16, 100) == 0 and lib.pcl_pointconv_level_infer_group_tile(32, 0) == 0


@pytest.mark.parametrize("ns,L,widths,M", [(64, 3, (128, 128, 288), 16), (64, 2, (128, 128, 256), 16), (64, 3, (128, 128, 256), 8),
                                           (0, 3, (64, 64, 128), 16)])
def test_pointconv_infer_launcher_rejects_other_shapes_on_the_host(ns, L, widths, M):
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    c_widths = (ctypes.c_int32 * 3)(*widths)
    rc = lib.pcl_pointconv_level_infer_f32(p, p, p, p, 3, p, p, 1, 8, 4, ns, L, c_widths, ptrs, ptrs, ptrs, 0.0, p, M, p, 16 * widths[2], None)
    assert rc == -1
    assert b"no kernel" in lib.pcl_last_error()


def test_frozen_pointconv_rejects_other_networks():
    from pointcloudlib_amd.inference import FrozenPointConv
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    with pytest.raises(TypeError, match="PointConvDensityClsSsg"):
        FrozenPointConv(PointNet())


def test_frozen_keeps_its_dispatch():
    import pointcloudlib_amd.inference as inference
    from pointcloudlib_amd.networks.cls.pointconv import PointConvDensityClsSsg
    assert "FrozenPointConv" in inference.__all__
    with pytest.raises(TypeError, match="PointNet2_cls or PointNetMSG"):
        inference.frozen(PointConvDensityClsSsg())


def _small_nets_torch(packed, d, dens):
    """The packed buffer evaluated at the header's offsets, in fp64: (w [., 16], rho [., 1])."""
    p = packed.double()

    def layer(x, w0, cout, cin, s0, t0):
        W = p[w0:w0 + cout * cin].view(cout, cin)
        return (p[s0:s0 + cout] * (x @ W.t()) + p[t0:t0 + cout]).clamp(min=0)

    w = layer(layer(layer(d, 0, 8, 3, 24, 32), 40, 8, 8, 104, 112), 120, 16, 8, 248, 264)
    rho = layer(layer(layer(dens, 280, 8, 1, 288, 296), 304, 8, 8, 368, 376), 384, 1, 8, 392, 393)
    return w, rho


def test_packed_small_nets_reproduce_the_eval_restatement():
    """``pack_small_nets`` (the folded eval constants at the header's offsets) against the fp64 restatement read from the modules'
    parameters and running statistics: the only difference is the fp32 rounding of the folded constants."""
    from pointcloudlib_amd.inference import pack_small_nets
    from pointcloudlib_amd.misc.pointconv_utils import DensityNet, WeightNet
    torch.manual_seed(3)
    wn, dn = WeightNet(3, 16).eval(), DensityNet().eval()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for mlp in (wn.mlp, dn.mlp):
            for l in range(mlp.n_layers):
                c = mlp.gammas[l].numel()
                mlp.gammas[l].copy_(torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0) * (0.5 + torch.rand(c, generator=g)))
                mlp.betas[l].copy_(0.1 * torch.randn(c, generator=g))
                getattr(mlp, f"running_mean_{l}").copy_(0.1 * torch.randn(c, generator=g))
                getattr(mlp, f"running_var_{l}").copy_(0.5 + 1.5 * torch.rand(c, generator=g))
        dn.mlp.gammas[2].abs_()                  # the DensityNet's one output stays alive (relu of a negative gamma erases it)
        dn.mlp.betas[2].fill_(0.5)
    packed = pack_small_nets(wn, dn)
    assert packed.shape == (400,) and packed.dtype == torch.float32 and bool((packed[394:] == 0).all())
    d = torch.rand(200, 3, generator=g).double() - 0.5
    dens = 3 * torch.rand(200, 1, generator=g).double() + 1e-3
    w, rho = _small_nets_torch(packed, d, dens)
    w_ref = R.run_stack(R.stack_of(wn.mlp), d, 0.0, torch.float64)
    rho_ref = R.run_stack(R.stack_of(dn.mlp), dens, 0.0, torch.float64)
    assert float(w_ref.abs().max()) > 0.1 and float(rho_ref.abs().max()) > 0.1
    assert float((w - w_ref).abs().max()) <= 1e-5 * float(w_ref.abs().max())
    assert float((rho - rho_ref).abs().max()) <= 1e-5 * float(rho_ref.abs().max())


@pytest.mark.parametrize("ns,widths,D,B,N,m,seed", EXACT_CASES)
def test_exact_cases_are_exact(ns, widths, D, B, N, m, seed):
    """The data of the GPU file's bit-for-bit test: every dot product's sum of |products| stays below 2^24 granules (so every
    partial sum, in any order, is an fp32 number), the fp32 and fp64 evaluations of the restatement agree bit for bit, and the
    result is no trivial one."""
    c = R.exact_case(ns, widths, D, B, N, m, seed)
    args = (c["feat"], c["wn"], c["dn"], c["xyz"], c["new_xyz"], c["points"], c["idx"], c["density"])
    audit = []
    want = R.level(*args, audit=audit)
    assert max(audit) < 2.0 ** 23
    assert torch.equal(R.level(*args, dtype=torch.float32).double(), want)
    assert torch.equal(want.float().double(), want)
    assert float((want != 0).double().mean()) > 0.3 and want.unique().numel() > 1000
    assert int(c["idx"].min()) == 0 and int(c["idx"].max()) == N - 1
    assert float(c["density"].min()) > 0 and float(c["density"].max()) <= 3
