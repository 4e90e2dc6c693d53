"""Frozen inference with bf16 matrix operands (``frozen(net, precision="bf16")``, pcl_sa_level_infer_bf16_f32): the parts that need
no GPU -- the C ABI's host-side checks, the Python contract, and the teeth of the yardstick (tests/bf16_bound.py)."""
import ctypes

import pytest
import torch

TRIPLES = [(32, 32, 64), (64, 64, 128), (64, 96, 128), (128, 128, 256)]


def test_bf16_symbol_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    name = "pcl_sa_level_infer_bf16_f32"
    assert name in _lib.declared_symbols()
    assert name in _lib._SIGS
    assert hasattr(lib, name)
    assert _lib._SIGS[name] == _lib._SIGS["pcl_sa_level_infer_f32"]          # the same argument list


def _host_call(lib, widths, W=None, idx="buf"):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 16 == 0
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    c_W = ptrs if W is None else (ctypes.c_void_p * 3)(p, W(p), p)
    c_widths = (ctypes.c_int32 * 3)(*widths)
    rc = lib.pcl_sa_level_infer_bf16_f32(p, p, p, p, None, None, 0, 3, p if idx == "buf" else None, p, 1, 8, 4, 8, 3, c_widths, c_W,
                                         ptrs, ptrs, 0.0, p, widths[2], 0, None)
    return rc, lib.pcl_last_error()


def test_bf16_launcher_rejects_on_the_host():
    """Every check runs before any HIP call: none of these needs a GPU."""
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    rc, err = _host_call(lib, (128, 128, 288))
    assert rc == -1 and b"no kernel" in err and b"pcl_sa_level_infer_bf16_f32" in err
    rc, err = _host_call(lib, (64, 64, 128), idx=None)
    assert rc == -1 and b"null pointer" in err
    rc, err = _host_call(lib, (64, 64, 128), W=lambda p: None)
    assert rc == -1 and b"null pointer" in err
    rc, err = _host_call(lib, (64, 64, 128), W=lambda p: ctypes.c_void_p(p.value + 8))
    assert rc == -1 and b"16-byte aligned" in err
    for c1, c2, c3 in TRIPLES:                               # one query for both precisions
        assert lib.pcl_sa_level_infer_supported(64, 3, c1, c2, c3, 0) == 1


def test_frozen_precision_argument():
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls, PointNetMSG
    from pointcloudlib_amd.networks.seg import pointnet2_partseg as seg
    net = PointNet2_cls()
    with pytest.raises(ValueError, match="fp32.*bf16"):
        frozen(net, precision="fp16")
    assert frozen(net).precision == "fp32"
    assert frozen(net, precision="fp32").precision == "fp32"
    for cls in (PointNet2_cls, PointNetMSG, seg.PointNet2_partseg, seg.PointNetMSG):
        f32, f16 = frozen(cls()), frozen(cls(), precision="bf16")
        assert f16.precision == "bf16"
        kinds = [[k for k, _ in lv] for lv in f16.levels]
        assert kinds == [[k for k, _ in lv] for lv in f32.levels]
        assert all(k == "fused" for lv in kinds[:2] for k in lv) and kinds[2] == ["all"]
        for lv32, lv16 in zip(f32.levels, f16.levels):
            for (k, p32), (_, p16) in zip(lv32, lv16):
                assert type(p32) is type(p16)
                if k == "fused":
                    assert p32.entry == "pcl_sa_level_infer_f32" and not hasattr(p32, "Ws_bf16")
                    assert p16.entry == "pcl_sa_level_infer_bf16_f32"


def test_frozen_rejects_other_networks_under_either_precision():
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    with pytest.raises(TypeError, match="PointNet2_cls or PointNetMSG"):
        frozen(PointNet(), precision="bf16")


def test_direct_construction_checks_the_type_then_the_precision():
    """The six evaluators share one constructor: a direct ``FrozenPointNet2(net, "bf17")`` raises what ``frozen()`` raises, and a
    call wrong in both respects names the network."""
    from pointcloudlib_amd import inference as I
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls
    for cls in (I.FrozenPointNet2, I.FrozenPointNet2Partseg, I.FrozenPointNet, I.FrozenPointNetPartseg, I.FrozenPointConv, I.FrozenPointConvPartseg):
        other = PointNet2_cls() if cls.NET is PointNet else PointNet()
        with pytest.raises(TypeError, match=f"{cls.__name__} takes networks.*{cls.NET.__name__}, got {type(other).__name__}"):
            cls(other, "bf17")
    with pytest.raises(ValueError, match="FrozenPointNet2: precision must be one of .*fp32.*bf16.*got 'bf17'"):
        I.FrozenPointNet2(PointNet2_cls(), "bf17")


def test_bf16_snapshot_and_refresh():
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls
    torch.manual_seed(0)
    net = PointNet2_cls()
    fnet = frozen(net, precision="bf16")

    def check():
        n = 0
        for module, plans in zip(net.pointnet_modules, fnet.levels):
            for mlp, (kind, plan) in zip(module.mlps, plans):
                if kind != "fused":
                    continue
                assert plan.Ws_bf16[0] is None and len(plan.Ws_bf16) == mlp.n_layers
                for l in range(1, mlp.n_layers):
                    w = plan.Ws_bf16[l]
                    assert w.dtype == torch.bfloat16 and w.is_contiguous() and w.data_ptr() % 16 == 0
                    assert torch.equal(w, mlp.weights[l].detach().to(torch.bfloat16))
                    assert plan.c_W[l] == w.data_ptr()
                    assert torch.equal(plan.Ws[l], mlp.weights[l].detach())            # the fp32 snapshot stays
                    n += 1
        return n

    assert check() == 4                                       # SSG: two fused levels, layers 2 and 3 of each
    old = fnet.levels[1][0][1].Ws_bf16[1].clone()
    with torch.no_grad():
        net.pointnet_modules[1].mlps[0].weights[1].mul_(1.5)
    assert torch.equal(fnet.levels[1][0][1].Ws_bf16[1], old)  # a snapshot: stale until refresh()
    fnet.refresh()
    assert not torch.equal(fnet.levels[1][0][1].Ws_bf16[1], old)
    check()


# ----------------------------------------------------------------------------------------------- the yardstick has teeth
def _rows_case(triple, slope, seed):
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.inference import _eval_consts
    torch.manual_seed(seed)
    mlp = PointwiseMLP([6] + list(triple), bias=False, bn=True, slope=slope)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                     # eval constants away from scale 1 / shift 0 (some gamma < 0)
        for l in range(mlp.n_layers):
            c = mlp.gammas[l].numel()
            sign = torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
            mlp.gammas[l].copy_(sign * (0.5 + torch.rand(c, generator=g)))
            mlp.betas[l].copy_(0.1 * torch.randn(c, generator=g))
            getattr(mlp, f"running_mean_{l}").copy_(0.1 * torch.randn(c, generator=g))
            getattr(mlp, f"running_var_{l}").copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    Ws = [w.detach() for w in mlp.weights]
    consts = [_eval_consts(mlp, l) for l in range(mlp.n_layers)]
    x = torch.cat([torch.rand(64, 24, 3, generator=g) - torch.rand(64, 1, 3, generator=g), torch.randn(64, 24, 3, generator=g)], dim=-1)
    return x, Ws, [c[0] for c in consts], [c[1] for c in consts]


@pytest.mark.parametrize("triple", TRIPLES)
@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_yardstick_has_teeth(triple, slope):
    """The faithful emulation of the contract is within the bound; one that drops the last 8 k of the last layer is not."""
    from bf16_bound import emulate, rows_ref_and_bound, worst_ratio
    x, Ws, sc, sh = _rows_case(triple, slope, seed=sum(triple) + int(10 * slope))
    ref, bound = rows_ref_and_bound(x.double(), Ws, sc, sh, slope)
    ref, bound = ref.max(dim=1)[0], bound.max(dim=1)[0]       # 64 groups of 24 rows
    faithful = worst_ratio(emulate(x, Ws, sc, sh, slope).max(dim=1)[0], ref, bound)
    dropped = worst_ratio(emulate(x, Ws, sc, sh, slope, drop_last_k=8).max(dim=1)[0], ref, bound)
    print(f"{triple} slope {slope}: faithful {faithful:.3f} x bound, last 8 k dropped {dropped:.2f} x bound")
    assert faithful <= 1.0
    assert dropped > 1.0
