"""bf16 frozen PointConv part segmentation (``FrozenPointConvPartseg(net, precision="bf16")``,
pcl_pointconv_seg_level_infer_bf16_f32): the parts that need no GPU -- the new symbol and its host-side rejections, the Python
contract, the bf16 snapshot, the exactness in bf16 of the data the GPU file compares bit for bit, and the teeth of the yardstick
(tests/pointconv_bf16_bound.py, unchanged: it is generic in the layer count) at the five new shapes."""
import ctypes

import pytest
import torch

import pointconv_bf16_bound as PB
import pointconv_infer_ref as R
from pointconv_partseg_bf16_cases import BF16, CLS_BF16, EXACT, FP32, NEW, TEETH_GROUPS, case_args, module_case
from pointconv_partseg_infer_ref import EXACT_SEED, SHAPES

STOCK = ["fused", "fused", "fused", "module", "module", "fused", "fused", "fused"]


def test_bf16_symbol_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert BF16 in _lib.declared_symbols()
    assert BF16 in _lib._SIGS
    assert hasattr(lib, BF16)
    assert _lib._SIGS[BF16] == _lib._SIGS[CLS_BF16]                    # the same argument list (W as const void* const*)


@pytest.mark.parametrize("ns,L,widths,M", [(32, 3, (256, 256, 512), 16), (16, 2, (512, 512, 512), 16), (16, 3, (128, 128, 256), 16),
                                           (16, 2, (128, 128, 128), 8), (8, 2, (128, 128, 128), 16)])
def test_bf16_launcher_rejects_other_shapes_on_the_host(ns, L, widths, M):
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    c_widths = (ctypes.c_int32 * 3)(*widths)
    rc = getattr(lib, BF16)(p, p, p, p, 3, p, p, 1, 8, 4, ns, L, c_widths, ptrs, ptrs, ptrs, 0.0, p, M, p, 16 * 512, None)
    err = lib.pcl_last_error()
    assert rc == -1
    assert b"no kernel" in err and BF16.encode() in err


def test_precision_argument():
    from pointcloudlib_amd.inference import PRECISIONS, FrozenPointConvPartseg, _LevelLinear
    from pointcloudlib_amd.networks.seg.pointconv_partseg import PointConvDensity_partseg
    net = PointConvDensity_partseg().train()
    with pytest.raises(ValueError, match="fp32.*bf16"):
        FrozenPointConvPartseg(net, precision="int8")
    assert "int8" not in PRECISIONS
    f32, f16 = FrozenPointConvPartseg(net), FrozenPointConvPartseg(net, precision="bf16")
    assert f32.precision == "fp32" and FrozenPointConvPartseg(net, precision="fp32").precision == "fp32" and f16.precision == "bf16"
    assert f32.levels == f16.levels == STOCK
    assert net.training and all(m.training for m in net.modules())
    for (k, p32), (_, p16) in zip(f32.plans, f16.plans):
        assert type(p32) is type(p16)
        if k == "fused":
            assert p32.entry == FP32 and p32.precision == "fp32" and not hasattr(p32, "Ws_bf16")
            assert p16.entry == BF16 and p16.precision == "bf16" and p16.L == p32.L
            assert type(p32.linear) is type(p16.linear) is _LevelLinear and p16.linear.W.dtype == torch.float32
            assert p16.nets.dtype == torch.float32 and p16.W0.dtype == torch.float32
            assert p16.Wf is None or p16.Wf.dtype == torch.float32
        else:                                                          # an eval-mode copy of the level's own module, all fp32
            assert not p16.training and all(t.dtype == torch.float32 for t in p16.state_dict().values() if t.is_floating_point())
    assert type(f16.fc1) is type(f32.fc1)
    assert all(w.dtype == torch.float32 for w in f16.fc1.Ws) and f16.W3.dtype == torch.float32 and f16.b3.dtype == torch.float32


def test_frozen_keeps_its_dispatch_under_either_precision():
    import pointcloudlib_amd.inference as inference
    from pointcloudlib_amd.networks.seg.pointconv_partseg import PointConvDensity_partseg
    for kw in ({}, {"precision": "bf16"}):
        with pytest.raises(TypeError, match="PointNet2_cls or PointNetMSG"):
            inference.frozen(PointConvDensity_partseg(), **kw)


def test_bf16_snapshot_and_refresh():
    """The weights behind the first layer of every fused level of a perturbed net, rounded once: L - 1 of a level of L layers,
    2 + 2 + 2 + 1 + 1 + 2 = 10 in the stock network (its fused levels have 3, 3, 3, 2, 2, 3 layers).  Layer 1 has no entry;
    ``refresh()`` rounds again."""
    from pointcloudlib_amd.inference import FrozenPointConvPartseg
    from pointcloudlib_amd.networks.seg.pointconv_partseg import PointConvDensity_partseg
    from test_inference_gpu import _perturb
    torch.manual_seed(0)
    net = _perturb(PointConvDensity_partseg(), 1)
    with torch.no_grad():
        for name in net.LEVELS:
            for w in getattr(net, name).mlp.weights:
                w.mul_(1.0 + 0.37 * torch.rand_like(w))
    fnet = FrozenPointConvPartseg(net, precision="bf16")

    def check():
        n = 0
        for name, (kind, plan) in zip(net.LEVELS, fnet.plans):
            if kind != "fused":
                assert not hasattr(plan, "Ws_bf16")
                continue
            mlp = getattr(net, name).mlp
            assert plan.Ws_bf16[0] is None and plan.Ws[0] is None and not plan.c_W[0]
            assert len(plan.Ws_bf16) == mlp.n_layers == plan.L and plan.operands is plan.Ws_bf16
            for l in range(1, plan.L):
                w = plan.Ws_bf16[l]
                assert w.dtype == torch.bfloat16 and w.is_contiguous() and w.data_ptr() % 16 == 0
                assert torch.equal(w, plan.Ws[l].to(torch.bfloat16)) and torch.equal(w, mlp.weights[l].detach().to(torch.bfloat16))
                assert not torch.equal(w.float(), plan.Ws[l])                              # a rounding that does something
                assert plan.c_W[l] == w.data_ptr()
                assert torch.equal(plan.Ws[l], mlp.weights[l].detach())                    # the fp32 snapshot stays
                n += 1
        return n

    assert fnet.levels == STOCK and [p.L for k, p in fnet.plans if k == "fused"] == [3, 3, 3, 2, 2, 3]
    assert check() == 10
    plan = lambda: fnet.plans[6][1]                                    # in2: two layers, one bf16 weight
    old = plan().Ws_bf16[1].clone()
    with torch.no_grad():
        net.in2.mlp.weights[1].mul_(1.5)
    assert torch.equal(plan().Ws_bf16[1], old)                         # a snapshot: stale until refresh()
    fnet.refresh()
    assert fnet.precision == "bf16" and not torch.equal(plan().Ws_bf16[1], old)
    assert check() == 10


# ----------------------------------------------------------------------------------------------- the exact data stay exact in bf16
@pytest.mark.parametrize("name,ns,widths,D,B,N,m", EXACT, ids=[e[0] for e in EXACT])
def test_exact_cases_are_exact_in_bf16(name, ns, widths, D, B, N, m):
    """On the data of the bit-for-bit GPU tests every activation that the contract rounds (z1; at three layers z2 too) and every
    weight behind layer 1 is a bf16 number, and every partial sum an fp32 number: the bf16 contract then gives the fp64 result
    bit for bit."""
    c = R.exact_case(ns, widths, D, B, N, m, EXACT_SEED)
    for W, _, _ in c["feat"][1:]:
        assert R.is_bf16(W)
    worst, inexact, total, audit = 0.0, 0, 0, []
    for b in range(B):                                        # a cloud at a time: the rows of the large cases are many
        bs = slice(b, b + 1)
        pts = None if c["points"] is None else c["points"][bs]
        _, x, _ = PB.rows(c["xyz"][bs], c["new_xyz"][bs], pts, c["idx"][bs])
        rounded = PB.activations(c["feat"], x)[:-1]           # the last activation is never rounded
        assert len(rounded) == len(widths) - 1
        for z in rounded:
            inexact += int((z.float().to(torch.bfloat16).double() != z).sum())
            total += z.numel()
            worst = max(worst, float(z.abs().max()))
        R.level(c["feat"], c["wn"], c["dn"], c["xyz"][bs], c["new_xyz"][bs], pts, c["idx"][bs], c["density"][bs], audit=audit)
    print(f"{name} ns={ns} B={B} m={m}: {inexact} of {total} rounded activations inexact in bf16, largest {worst}, audit {max(audit):.3e}")
    assert inexact == 0
    assert max(audit) < 2.0 ** 24


# ----------------------------------------------------------------------------------------------- the yardstick has teeth
@pytest.mark.parametrize("name", NEW)
def test_yardstick_has_teeth(name):
    """The faithful emulation of the contract is within the bound; one whose last layer drops its last 8 k is not; the bound is
    finite and positive wherever the reference is nonzero.  192 groups of the level's perturbed modules:

        sa0 faithful 0.081, dropped 7.51 x     sa2 faithful 0.019, dropped 1.55 x     in1 faithful 0.143, dropped 10.30 x
        in2 faithful 0.214, dropped 20.52 x    in3 faithful 0.025, dropped 2.74 x

    At two layers the dropped k are of the one bf16 layer."""
    from test_inference_pointconv_gpu import _frozen_stacks
    B, N, m = TEETH_GROUPS[name]
    assert B * m >= 192
    mods, c = module_case(name, (B, N, m))
    feat, nets = _frozen_stacks(mods)
    assert len(feat) == len(SHAPES[name][1])
    ref, bound = PB.level_ref_and_bound(feat, nets, *case_args(c))
    assert float((ref != 0).double().mean()) > 0.3, "a trivial level"
    assert bool(torch.isfinite(bound).all()) and bool((bound[ref != 0] > 0).all())
    faithful = PB.worst_ratio(PB.emulate(feat, nets, *case_args(c)), ref, bound)
    dropped = PB.worst_ratio(PB.emulate(feat, nets, *case_args(c), drop_last_k=8), ref, bound)
    rel = float((bound / ref.abs().clamp(min=1e-30))[ref != 0].median())
    print(f"{name}: faithful {faithful:.3f} x bound, last 8 k of the last layer dropped {dropped:.2f} x bound; median bound / |ref| {rel:.3e}")
    assert faithful <= 1.0
    assert dropped > 1.0
