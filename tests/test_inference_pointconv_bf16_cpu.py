"""bf16 frozen PointConv (``FrozenPointConv(net, precision="bf16")``, pcl_pointconv_level_infer_bf16_f32): the parts that need no GPU
-- the new symbol and its host-side rejections, the Python contract, the exactness of the data the GPU file compares bit for bit,
the teeth of the yardstick (tests/pointconv_bf16_bound.py) and the bf16 snapshot."""
import ctypes

import pytest
import torch

import pointconv_bf16_bound as PB
import pointconv_infer_ref as R

ENTRY = "pcl_pointconv_level_infer_bf16_f32"
# (ns, widths, D, B, N, m): SHAPES and MANY of tests/test_inference_pointconv_gpu.py, which the bf16 GPU file reuses
SHAPES = {32: (32, [64, 64, 128], 0, 3, 40, 5), 64: (64, [128, 128, 256], 128, 2, 70, 3)}
MANY = {32: (32, [64, 64, 128], 0, 5, 40, 1639), 64: (64, [128, 128, 256], 128, 3, 70, 1367)}
EXACT_SEED = 0


def test_bf16_symbol_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert ENTRY in _lib.declared_symbols()
    assert ENTRY in _lib._SIGS
    assert hasattr(lib, ENTRY)
    assert _lib._SIGS[ENTRY] == _lib._SIGS["pcl_pointconv_level_infer_f32"]          # the same argument list


@pytest.mark.parametrize("ns,L,widths,M", [(64, 3, (128, 128, 288), 16), (64, 2, (128, 128, 256), 16), (64, 3, (128, 128, 256), 8),
                                           (0, 3, (64, 64, 128), 16)])
def test_bf16_launcher_rejects_other_shapes_on_the_host(ns, L, widths, M):
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    c_widths = (ctypes.c_int32 * 3)(*widths)
    rc = getattr(lib, ENTRY)(p, p, p, p, 3, p, p, 1, 8, 4, ns, L, c_widths, ptrs, ptrs, ptrs, 0.0, p, M, p, 16 * widths[2], None)
    err = lib.pcl_last_error()
    assert rc == -1
    assert b"no kernel" in err and ENTRY.encode() in err


def test_precision_argument():
    from pointcloudlib_amd.inference import PRECISIONS, FrozenPointConv
    from pointcloudlib_amd.networks.cls.pointconv import PointConvDensityClsSsg
    net = PointConvDensityClsSsg()
    with pytest.raises(ValueError, match="fp32.*bf16"):
        FrozenPointConv(net, precision="int8")
    assert "int8" not in PRECISIONS
    f32, f16 = FrozenPointConv(net), FrozenPointConv(net, precision="bf16")
    assert f32.precision == "fp32" and FrozenPointConv(net, precision="fp32").precision == "fp32" and f16.precision == "bf16"
    assert f32.levels == f16.levels == ["fused", "fused", "all"]
    for (k, p32), (_, p16) in zip(f32.plans, f16.plans):
        assert type(p32) is type(p16)
        if k == "fused":
            assert p32.entry == "pcl_pointconv_level_infer_f32" and not hasattr(p32, "Ws_bf16")
            assert p16.entry == ENTRY
            assert type(p32.linear) is type(p16.linear) and p16.linear.W.dtype == torch.float32
            assert p16.nets.dtype == torch.float32 and p16.W0.dtype == torch.float32
    assert [type(m) for m in f32.head] == [type(m) for m in f16.head]
    assert all(p.dtype == torch.float32 for m in f16.head for p in m.parameters())


def test_frozen_keeps_its_dispatch_under_either_precision():
    import pointcloudlib_amd.inference as inference
    from pointcloudlib_amd.networks.cls.pointconv import PointConvDensityClsSsg
    for kw in ({}, {"precision": "bf16"}):
        with pytest.raises(TypeError, match="PointNet2_cls or PointNetMSG"):
            inference.frozen(PointConvDensityClsSsg(), **kw)


def test_bf16_snapshot_and_refresh():
    """The weights of layers 2 and 3 of a perturbed feature MLP, rounded once; layer 1 has no entry; ``refresh()`` rounds again."""
    from pointcloudlib_amd.inference import FrozenPointConv
    from pointcloudlib_amd.networks.cls.pointconv import PointConvDensityClsSsg
    from test_inference_gpu import _perturb
    torch.manual_seed(0)
    net = _perturb(PointConvDensityClsSsg(), 1)
    with torch.no_grad():
        for sa in (net.sa1, net.sa2):
            for w in sa.mlp.weights:
                w.mul_(1.0 + 0.37 * torch.rand_like(w))
    fnet = FrozenPointConv(net, precision="bf16")

    def check():
        n = 0
        for sa, (kind, plan) in zip((net.sa1, net.sa2), fnet.plans):
            assert kind == "fused"
            mlp = sa.mlp
            assert plan.Ws_bf16[0] is None and plan.Ws[0] is None and not plan.c_W[0] and len(plan.Ws_bf16) == mlp.n_layers == 3
            for l in (1, 2):
                w = plan.Ws_bf16[l]
                assert w.dtype == torch.bfloat16 and w.is_contiguous() and w.data_ptr() % 16 == 0
                assert torch.equal(w, plan.Ws[l].to(torch.bfloat16)) and torch.equal(w, mlp.weights[l].detach().to(torch.bfloat16))
                assert not torch.equal(w.float(), plan.Ws[l])                              # a rounding that does something
                assert plan.c_W[l] == w.data_ptr()
                assert torch.equal(plan.Ws[l], mlp.weights[l].detach())                    # the fp32 snapshot stays
                n += 1
        return n

    assert check() == 4
    old = fnet.plans[1][1].Ws_bf16[1].clone()
    with torch.no_grad():
        net.sa2.mlp.weights[1].mul_(1.5)
    assert torch.equal(fnet.plans[1][1].Ws_bf16[1], old)      # a snapshot: stale until refresh()
    fnet.refresh()
    assert not torch.equal(fnet.plans[1][1].Ws_bf16[1], old)
    assert check() == 4


# ----------------------------------------------------------------------------------------------- the exact data stay exact in bf16
@pytest.mark.parametrize("shape", [SHAPES[32], SHAPES[64], MANY[32], MANY[64]], ids=["ns32", "ns64", "many32", "many64"])
def test_exact_cases_are_exact_in_bf16(shape):
    """On the data of the bit-for-bit GPU tests every z1 and z2 of the fp64 restatement and every weight of layers 2 and 3 is a bf16
    number, and every partial sum an fp32 number: the bf16 contract then gives the fp64 result bit for bit."""
    ns, widths, D, B, N, m = shape
    c = R.exact_case(ns, widths, D, B, N, m, EXACT_SEED)
    for W, _, _ in c["feat"][1:]:
        assert R.is_bf16(W)
    worst, inexact, total, audit = 0.0, 0, 0, []
    for b in range(B):                                        # a cloud at a time: the rows of the large cases are many
        bs = slice(b, b + 1)
        pts = None if c["points"] is None else c["points"][bs]
        _, x, _ = PB.rows(c["xyz"][bs], c["new_xyz"][bs], pts, c["idx"][bs])
        z1, z2, _ = PB.activations(c["feat"], x)
        for z in (z1, z2):
            inexact += int((z.float().to(torch.bfloat16).double() != z).sum())
            total += z.numel()
        worst = max(worst, float(z2.abs().max()))
        R.level(c["feat"], c["wn"], c["dn"], c["xyz"][bs], c["new_xyz"][bs], pts, c["idx"][bs], c["density"][bs], audit=audit)
    print(f"ns={ns} B={B} m={m}: {inexact} of {total} z1 / z2 inexact in bf16, largest |z2| {worst}, audit {max(audit):.3e}")
    assert inexact == 0
    assert max(audit) < 2.0 ** 24


# ----------------------------------------------------------------------------------------------- the yardstick has teeth
TEETH_GROUPS = (4, 70, 48)                                    # B, N, m of the yardstick's own case: 192 groups


def _random_level(ns):
    """The perturbed level of the GPU file's random-data test (``_module_case`` of tests/test_inference_pointconv_gpu.py: same
    seeds, so the same modules -- on the CPU they are only read, never run) with inputs drawn the same way for 192 groups."""
    from pointcloudlib_amd.inference import _eval_consts, pack_small_nets
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.misc.pointconv_utils import DensityNet, WeightNet
    from test_inference_gpu import _perturb
    _, widths, D, _, _, _ = SHAPES[ns]
    B, N, m = TEETH_GROUPS
    torch.manual_seed(100 + ns)
    mods = torch.nn.ModuleDict({"mlp": PointwiseMLP([3 + D] + widths, bias=True), "wn": WeightNet(3, 16), "dn": DensityNet()})
    _perturb(mods, 7 + ns)
    with torch.no_grad():
        mods["dn"].mlp.gammas[-1].abs_()                      # the DensityNet's one output stays alive
        mods["dn"].mlp.betas[-1].fill_(0.5)
    mlp = mods["mlp"]
    feat = [(mlp.weights[l].detach(), *_eval_consts(mlp, l)) for l in range(mlp.n_layers)]
    g = torch.Generator().manual_seed(ns)
    args = (torch.rand(B, N, 3, generator=g), torch.rand(B, m, 3, generator=g), None if D == 0 else torch.randn(B, N, D, generator=g),
            R.knn_lists(B, N, m, ns, g), 3 * torch.rand(B, N, generator=g).clamp(min=1e-3))
    return feat, pack_small_nets(mods["wn"], mods["dn"]), args


@pytest.mark.parametrize("ns", [32, 64])
def test_yardstick_has_teeth(ns):
    """The faithful emulation of the contract is within the bound; one whose layer 3 drops its last 8 k is not; the bound is finite
    and positive wherever the reference is nonzero.

    The bound carries absolute sums through two bf16 layers and the contraction, and 8 dropped k are a sixteenth of layer 3's
    fan-in at 128/128/256: there a single group need not show the defect (the 6 groups of the GPU file's case: 0.90 x bound), so
    the case has 192 groups of the same network (about 1.2 x; 48 groups 1.16 x, 384 groups 1.85 x).  At 64/64/128 the defect is 2.6 .. 2.8
    x bound at any of these sizes.  A defect that moves every output by less than the bound is not seen by this yardstick."""
    feat, nets, args = _random_level(ns)
    ref, bound = PB.level_ref_and_bound(feat, nets, *args)
    assert float((ref != 0).double().mean()) > 0.3, "a trivial level"
    assert bool(torch.isfinite(bound).all()) and bool((bound[ref != 0] > 0).all())
    faithful = PB.worst_ratio(PB.emulate(feat, nets, *args), ref, bound)
    dropped = PB.worst_ratio(PB.emulate(feat, nets, *args, drop_last_k=8), ref, bound)
    rel = float((bound / ref.abs().clamp(min=1e-30))[ref != 0].median())
    print(f"ns={ns}: faithful {faithful:.3f} x bound, last 8 k of layer 3 dropped {dropped:.2f} x bound; median bound / |ref| {rel:.3e}")
    assert faithful <= 1.0
    assert dropped > 1.0
