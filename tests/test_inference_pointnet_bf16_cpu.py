"""Frozen PointNet inference with bf16 matrix operands (``FrozenPointNet(net, precision="bf16")``,
pcl_pointnet_stack_infer_bf16_f32): the parts that need no GPU -- the C ABI's host-side checks, the Python contract, and the teeth
of the yardstick (tests/pointnet_bf16_yardstick.py)."""
import ctypes

import pytest
import torch

NAME = "pcl_pointnet_stack_infer_bf16_f32"
_WIDTHS = (64, 64, 64, 128, 1024)


def _w(*widths):
    return (ctypes.c_int32 * len(widths))(*widths)


def test_bf16_symbol_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert NAME in _lib.declared_symbols()
    assert NAME in _lib._SIGS
    assert hasattr(lib, NAME)
    assert _lib._SIGS[NAME] == _lib._SIGS["pcl_pointnet_stack_infer_f32"]          # the same argument list


def _launch(lib, widths=_WIDTHS, C0=3, W=None, ws_bytes=None, slope=0.0, B=2, N=100):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 16 == 0
    L = len(widths)
    ptrs = (ctypes.c_void_p * L)(*[p] * L)
    c_W = ptrs if W is None else (ctypes.c_void_p * L)(*[W(p) if l == 2 else p for l in range(L)])
    if ws_bytes is None:
        ws_bytes = lib.pcl_pointnet_stack_infer_workspace_bytes(B, N, widths[-1])
    rc = getattr(lib, NAME)(p, 3 * N, 1, N, None, B, N, C0, p, 3, L, _w(*widths), c_W, ptrs, ptrs, slope, p, ws_bytes, p, 1024, None)
    return rc, lib.pcl_last_error()


def test_bf16_launcher_rejects_on_the_host():
    """Every check runs before any HIP call: none of these needs a GPU."""
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for widths, c0 in [((64, 64, 96, 128, 1024), 3), ((64, 64, 128, 1024), 3), (_WIDTHS, 4)]:
        rc, err = _launch(lib, widths, C0=c0)
        assert rc == -1 and b"no kernel" in err and NAME.encode() in err
    rc, err = _launch(lib, W=lambda p: None)
    assert rc == -1 and b"null pointer" in err
    rc, err = _launch(lib, W=lambda p: ctypes.c_void_p(p.value + 8))
    assert rc == -1 and b"16-byte aligned" in err
    need = lib.pcl_pointnet_stack_infer_workspace_bytes(2, 100, 1024)
    rc, err = _launch(lib, ws_bytes=need - 4)
    assert rc == _lib.define("PCL_EWS") and b"workspace" in err
    for slope in (-0.1, 1.5):                                # the last epilogue runs on a tile's extreme accumulators
        rc, err = _launch(lib, slope=slope)
        assert rc == -1 and b"slope" in err
    assert lib.pcl_pointnet_stack_infer_supported(3, 5, _w(*_WIDTHS)) == 1           # one query for both precisions


def test_frozen_pointnet_precision_argument():
    from pointcloudlib_amd.inference import FrozenPointNet
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    net = PointNet()
    with pytest.raises(ValueError, match="fp32.*bf16"):
        FrozenPointNet(net, precision="fp16")
    f32, f32b, f16 = FrozenPointNet(net), FrozenPointNet(net, precision="fp32"), FrozenPointNet(net, precision="bf16")
    assert (f32.precision, f32b.precision, f16.precision) == ("fp32", "fp32", "bf16")
    assert f32.plan == f16.plan == "fused"
    assert f32.entry == f32b.entry == "pcl_pointnet_stack_infer_f32" and not hasattr(f32, "Ws_bf16")
    assert f16.entry == NAME
    assert all(p.dtype == torch.float32 for m in f16.head for p in m.parameters())                  # the head stays fp32
    # a stack of other widths: the module plan under either precision, an fp32 copy of the stack (the GPU tests run it)
    net.convs = PointwiseMLP([3, 64, 64, 96, 1024], bias=False)
    for precision in ("fp32", "bf16"):
        f = FrozenPointNet(net, precision=precision)
        assert f.plan == "module" and f.precision == precision and not hasattr(f, "Ws_bf16") and not hasattr(f, "entry")
        assert all(p.dtype == torch.float32 for p in f._convs.parameters())


def test_bf16_snapshot_and_refresh():
    from pointcloudlib_amd.inference import FrozenPointNet
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    torch.manual_seed(0)
    net = PointNet()
    fnet = FrozenPointNet(net, precision="bf16")

    def check():
        mlp = net.convs
        assert fnet.Ws_bf16[0] is None and len(fnet.Ws_bf16) == mlp.n_layers == 5
        assert fnet.c_W[0] is None
        for l in range(1, mlp.n_layers):
            w = fnet.Ws_bf16[l]
            assert w.dtype == torch.bfloat16 and w.is_contiguous() and w.data_ptr() % 16 == 0
            assert torch.equal(w, mlp.weights[l].detach().to(torch.bfloat16))
            assert fnet.c_W[l] == w.data_ptr()
            assert torch.equal(fnet.Ws[l], mlp.weights[l].detach())                # the fp32 snapshot stays
        assert torch.equal(fnet.Ws[0], mlp.weights[0].detach())

    check()
    old = fnet.Ws_bf16[4].clone()
    with torch.no_grad():
        net.convs.weights[4].mul_(1.5)
    assert torch.equal(fnet.Ws_bf16[4], old)                  # a snapshot: stale until refresh()
    fnet.refresh()
    assert not torch.equal(fnet.Ws_bf16[4], old)
    check()


# ----------------------------------------------------------------------------------------------- the yardstick has teeth
def test_round_bf16_is_round_to_nearest_even():
    from pointnet_bf16_yardstick import round_bf16
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, -257.0, 0.0, 3.0e-5], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -256.0, 0.0, float(torch.tensor(3.0e-5).to(torch.bfloat16))],
                        dtype=torch.float64)
    assert torch.equal(round_bf16(x), want)
    g = torch.Generator().manual_seed(0)
    r = torch.randn(4096, generator=g) * 10
    assert torch.equal(round_bf16(r.double()), r.to(torch.bfloat16).double())


DEFECTS = ["trunc", "drop_k4", "fp32_w5", "round_z5"]


@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_yardstick_has_teeth(slope):
    """On the GPU test's own generator and shape (B = 4, N = 129): the faithful emulation of the contract leaves at most 0.2 % of
    the outputs over T (a fifth of the cap) and none beyond the worst-case bound; each emulated defect fails the yardstick."""
    import bf16_bound
    import pointnet_bf16_yardstick as y
    B, N = 4, 129
    pts, Ws, sc, sh = y.case(100 + int(10 * slope), B, N)
    Wl = y.launch_weights(Ws)
    bounds = y.want_and_bounds(pts, [N] * B, Wl, sc, sh, slope)
    print(f"slope {slope}: median T {float(bounds[1].median()):.2e}")
    faithful = bf16_bound.emulate(pts, Ws, sc, sh, slope).max(dim=1)[0]
    ratio, share = y.check(faithful, *bounds, f"faithful emulation, slope {slope}", cap=y.CAP / 5)
    for defect in DEFECTS:
        got = y.emulate_defect(pts, Ws, sc, sh, slope, defect).max(dim=1)[0]
        r, s, outside = y.measure(got, *bounds)
        print(f"slope {slope} {defect}: worst ratio {r:.1f}, {100 * s:.1f} % over T, {outside} beyond the worst-case bound")
        with pytest.raises(AssertionError):
            y.check(got, *bounds, defect)
        assert s > 10 * y.CAP, f"{defect}: only {100 * s:.2f} % over T"
