"""bf16 frozen PointNet part segmentation (``FrozenPointNetPartseg(net, precision="bf16")``,
pcl_pointnet_seg_global_infer_bf16_f32 / pcl_pointnet_seg_head_infer_bf16_f32): the parts that need no GPU -- the yardstick of
tests/pointnet_partseg_bf16_yardstick.py against a faithful emulation and against one defect each, the one-rounding fold, the
snapshots ``refresh()`` makes, the new symbols' host-side rejections."""
import ctypes

import pytest
import torch

import pointnet_partseg_bf16_yardstick as ys

# what tests/test_inference_pointnet_partseg_bf16_gpu.py runs against the yardstick: (seed, slope) at B = 4, N = 129
GPU_CASES = [(0, 0.0), (1, 0.2)]
B, N, PART = 4, 129, 50
DEFECTS = ["trunc", "drop_k", "fp32_w", "round_out"]


def _global(seed, slope):
    out3, T128, Ws, sc, sh = ys.global_case(seed, B, N)
    n = [N] * B
    want = ys.global_want_and_bounds(out3, n, T128, ys.launch_weights(Ws), sc, sh, slope)[:4]
    return (lambda defect=None: ys.emulate_global(out3, n, T128, Ws, sc, sh, slope, defect)), want


def _head(seed, slope):
    F, bias, Ws, sc, sh, Wout, bout = ys.head_case(seed, B, N, PART)
    want = ys.head_want_and_bounds(F, bias, ys.launch_weights(Ws), sc, sh, Wout.to(torch.bfloat16), bout, slope)
    return (lambda defect=None: ys.emulate_head(F, bias, Ws, sc, sh, Wout, bout, slope, defect)), want


@pytest.mark.parametrize("seed,slope", GPU_CASES)
@pytest.mark.parametrize("make", [_global, _head], ids=["global", "head"])
def test_faithful_emulation_stays_under_half_the_cap(make, seed, slope):
    """The cap is twice what rounding flips alone cost on the seeds the GPU tests use; nothing leaves the worst-case bound."""
    emulate, want = make(seed, slope)
    ratio, share, outside = ys.measure(emulate(), *want)
    print(f"{make.__name__} seed {seed} slope {slope}: share over T {100 * share:.3f} %, worst ratio {ratio:.1f}")
    assert share <= ys.CAP / 2 and outside == 0
    ys.check(emulate(), *want, "emulation")


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("make", [_global, _head], ids=["global", "head"])
def test_yardstick_catches_a_defect(make, defect):
    """Truncation instead of rounding, one dropped k (conv4; the head's layer 3), an unrounded last weight, a rounded output."""
    emulate, want = make(*GPU_CASES[1])
    _, share, _ = ys.measure(emulate(defect), *want)
    print(f"{make.__name__} {defect}: share over T {100 * share:.1f} %")
    assert share > ys.CAP
    with pytest.raises(AssertionError):
        ys.check(emulate(defect), *want, defect)


def test_yardstick_catches_wrow_rounded_through_fp32():
    seed, slope = GPU_CASES[0]
    W64, once, twice = ys.double_rounding_wrow(seed)
    F, bias, Ws, sc, sh, Wout, bout = ys.head_case(seed, B, N, PART)
    want = ys.head_want_and_bounds(F, bias, [once] + ys.launch_weights(Ws[1:]), sc, sh, Wout.to(torch.bfloat16), bout, slope)
    good = ys.measure(ys.emulate_head(F, bias, Ws, sc, sh, Wout, bout, slope, W1_bf16=once), *want)
    bad = ys.measure(ys.emulate_head(F, bias, Ws, sc, sh, Wout, bout, slope, W1_bf16=twice), *want)
    print(f"rounded once: {100 * good[1]:.2f} % over T; through fp32: {100 * bad[1]:.1f} %")
    assert good[1] <= ys.CAP / 2 and bad[1] > ys.CAP


def test_head_fold_rounds_to_bf16_once():
    """``fold_partseg_head(..., dtype=torch.bfloat16)`` on a head whose folded ``Wrow`` is full of double-rounding cases: the
    result is the fp64 value's nearest bf16, not the fp32 fold's."""
    from pointcloudlib_amd.inference import fold_partseg_head
    W64, once, twice = ys.double_rounding_wrow(3)
    Wh = torch.zeros(256, 4944, dtype=torch.float64)
    Wh[:, 2064:2896] = W64                                     # out1 | out2 | out3 | out4; Wh_5 = 0: Wrow is these columns
    W5, s5, t5 = torch.randn(2048, 512), torch.rand(2048) + 0.5, torch.randn(2048)
    got = fold_partseg_head(Wh, W5, s5, t5, dtype=torch.bfloat16)[0]
    assert got.dtype == torch.bfloat16 and torch.equal(got, once)
    assert torch.equal(fold_partseg_head(Wh, W5, s5, t5)[0].to(torch.bfloat16), twice)


# ----------------------------------------------------------------------------------------------------------- the class
def test_precision_argument():
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
    net = PointNet_partseg()
    assert FrozenPointNetPartseg(net).precision == "fp32"
    fnet = FrozenPointNetPartseg(net, precision="bf16")         # TypeError without the feature
    assert fnet.precision == "bf16" and fnet.plan == "fused"
    for bad in ("fp16", "BF16", None):
        with pytest.raises(ValueError, match="precision"):
            FrozenPointNetPartseg(net, precision=bad)


def test_module_plan_ignores_the_precision():
    from pointcloudlib_amd.inference import FrozenPointNetPartseg
    from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
    net = PointNet_partseg(part_num=200)
    fnet = FrozenPointNetPartseg(net, precision="bf16")
    assert fnet.plan == "module" and fnet.precision == "bf16"
    assert not hasattr(fnet, "glob") and all(p.dtype == torch.float32 for p in fnet._module.parameters())
    assert not any(hasattr(fnet, name) for name in ("head", "Wout_bf16", "global_entry", "head_entry"))


def test_refresh_makes_the_bf16_snapshots():
    from pointcloudlib_amd.inference import FrozenPointNetPartseg, fold_partseg_head
    from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
    torch.manual_seed(0)
    net = PointNet_partseg(part_num=6)
    fnet = FrozenPointNetPartseg(net, precision="bf16")
    f32 = FrozenPointNetPartseg(net)
    assert not hasattr(f32.glob, "Ws_bf16") and not hasattr(f32.head, "Ws_bf16") and not hasattr(f32, "Wout_bf16")

    def check():
        s5, t5 = fnet.glob.scales[1], fnet.glob.shifts[1]
        Wrow16 = fold_partseg_head(net.convs.weights[0], net.conv5.weights[0], s5, t5, torch.bfloat16)[0]
        assert torch.equal(fnet.head.Ws_bf16[0], Wrow16)
        want = [net.conv4.weights[0], net.conv5.weights[0]]
        for got, w in zip(fnet.glob.Ws_bf16, want):
            assert got.dtype == torch.bfloat16 and got.is_contiguous() and torch.equal(got, w.detach().to(torch.bfloat16))
        for l in (1, 2):
            assert torch.equal(fnet.head.Ws_bf16[l], net.convs.weights[l].detach().to(torch.bfloat16))
        assert fnet.Wout_bf16.shape == (32, 128) and fnet.Wout_bf16.dtype == torch.bfloat16
        assert torch.equal(fnet.Wout_bf16[:6], net.convs4.weight.detach().to(torch.bfloat16)) and bool((fnet.Wout_bf16[6:] == 0).all())
        # the ctypes arrays point at the bf16 operands, 16-byte aligned; scale, shift and the fp32 snapshots are the fp32 form's
        operands = fnet.head.Ws_bf16 + [fnet.Wout_bf16]
        assert list(fnet.head_W) == [w.data_ptr() for w in operands] and all(w.data_ptr() % 16 == 0 for w in operands)
        assert list(fnet.glob.c_W) == [w.data_ptr() for w in fnet.glob.Ws_bf16]
        for a, b in zip(fnet.glob.scales + fnet.glob.shifts + fnet.head.Ws + [fnet.Wglob, fnet.c0],
                        f32.glob.scales + f32.glob.shifts + f32.head.Ws + [f32.Wglob, f32.c0]):
            assert torch.equal(a, b)

    check()
    with torch.no_grad():
        net.conv5.weights[0].mul_(1.5)
        net.convs.weights[0].add_(0.01)
    stale = fnet.head.Ws_bf16[0].clone()
    f32.refresh()
    fnet.refresh()
    assert not torch.equal(fnet.head.Ws_bf16[0], stale)
    check()


# ----------------------------------------------------------------------------------------------------------- the C ABI
_NAMES = ("pcl_pointnet_seg_global_infer_bf16_f32", "pcl_pointnet_seg_head_infer_bf16_f32")


def _w(*widths):
    return (ctypes.c_int32 * len(widths))(*widths)


def test_bf16_symbols_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for name in _NAMES:
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)


class _Launch:
    """The two bf16 launchers on a 256-byte host buffer (as in tests/test_inference_pointnet_partseg_cpu.py): every call here
    must be refused before anything is launched."""

    def __init__(self, lib):
        self.lib = lib
        self.buf = ctypes.create_string_buffer(256 + 16)
        base = ctypes.addressof(self.buf)
        self.p = ctypes.c_void_p(base + (-base) % 16)
        self.ptrs = (ctypes.c_void_p * 4)(*[self.p] * 4)
        self.B, self.N = 2, 100

    def part(self, C):
        return self.lib.pcl_pointnet_seg_part_workspace_bytes(self.B, self.N, C)

    def rows(self, ldf=832):
        return self.lib.pcl_pointnet_seg_rows_workspace_bytes(self.B, self.N, ldf)

    def glob(self, widths=(512, 2048), out=True, ws_bytes=None, ldf=832, f_bytes=None, W=None):
        p, q, B, N = self.p, self.ptrs, self.B, self.N
        ws_bytes = self.part(2048) if ws_bytes is None else ws_bytes
        f_bytes = self.rows(ldf) if f_bytes is None else f_bytes
        return self.lib.pcl_pointnet_seg_global_infer_bf16_f32(p, ldf, f_bytes, None, B, N, p, len(widths), _w(*widths), W or q, q, q, 0.0, p,
                                                               ws_bytes, p if out else None, 2048, None)

    def head(self, widths=(256, 256, 128, 50), out=True, ldf=832, f_bytes=None, w_out_rows=64, W=None):
        p, q, B, N = self.p, self.ptrs, self.B, self.N
        f_bytes = self.rows(ldf) if f_bytes is None else f_bytes
        return self.lib.pcl_pointnet_seg_head_infer_bf16_f32(p, ldf, f_bytes, None, B, N, p, 256, len(widths), _w(*widths), W or q, w_out_rows,
                                                             q, q, p, 0.0, p if out else None, widths[-1] * N, N, 1, None)


def test_bf16_launchers_reject_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    run = _Launch(lib)
    EWS = _lib.define("PCL_EWS")
    for call, bad in ((run.glob, (500, 2048)), (run.glob, (512, 2048, 2048)), (run.head, (256, 256, 96, 50)), (run.head, (256, 256, 128, 129))):
        assert call(widths=bad) == -1
        assert b"no kernel" in lib.pcl_last_error() and b"bf16" in lib.pcl_last_error()
    for call in (run.glob, run.head):
        assert call(out=False) == -1
        assert b"null pointer" in lib.pcl_last_error()
        assert call(f_bytes=run.rows() - 4) == EWS
        assert b"row workspace" in lib.pcl_last_error()
        assert call(ldf=834) == -1
        assert b"row stride" in lib.pcl_last_error()
        for l in range(2 if call == run.glob else 4):            # every layer's weight: null, then misaligned by one bf16
            q = (ctypes.c_void_p * 4)(*[run.p] * 4)
            q[l] = None
            assert call(W=q) == -1
            assert b"null pointer" in lib.pcl_last_error()
            q[l] = run.p.value + 2
            assert call(W=q) == -1
            assert b"16-byte aligned" in lib.pcl_last_error()
    assert run.glob(ws_bytes=run.part(2048) - 4) == EWS
    assert b"workspace" in lib.pcl_last_error()
    assert run.head(w_out_rows=50) == -1
    assert b"32-row blocks" in lib.pcl_last_error()
