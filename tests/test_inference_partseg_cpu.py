"""Frozen part-seg inference (pointcloudlib_amd/inference.py, csrc/infer_fp.hip): the parts that need no GPU."""
import ctypes

import pytest


def test_fp_infer_symbols_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for name in ("pcl_fp_level_infer_f32", "pcl_fp_level_infer_supported"):
        assert name in _lib.declared_symbols()
        assert name in _lib._SIGS
        assert hasattr(lib, name)


def test_fp_infer_supported_shapes():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for L, widths in [(2, (256, 256)), (2, (256, 128)), (3, (128, 128, 128)), (5, (128, 128, 128, 128, 50)),
                      (5, (128, 128, 128, 128, 64)), (5, (128, 128, 128, 128, 1)), (5, (128, 128, 128, 128, 32))]:
        assert lib.pcl_fp_level_infer_supported(L, *(widths + (0,) * (5 - L))) == 1, (L, widths)
    assert lib.pcl_fp_level_infer_supported(2, 200, 100, 0, 0, 0) == 0
    assert lib.pcl_fp_level_infer_supported(5, 128, 128, 128, 128, 65) == 0
    assert lib.pcl_fp_level_infer_supported(5, 128, 128, 128, 128, 0) == 0
    assert lib.pcl_fp_level_infer_supported(4, 128, 128, 128, 128, 0) == 0
    assert lib.pcl_fp_level_infer_supported(3, 256, 256, 128, 0, 0) == 0
    assert lib.pcl_fp_level_infer_supported(6, 128, 128, 128, 128, 50) == 0


def _call(lib, widths, Us, out, tap=None, tap_layer=-1, ldt=0):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p = (p + 15) // 16 * 16
    L = len(widths)
    ptrs = (ctypes.c_void_p * L)(*([p] * L))
    w = (ctypes.c_int32 * L)(*widths)
    return lib.pcl_fp_level_infer_f32(Us and p, None, None, 0, 0, None, None, None, 1, None, 2, 70, L, w, ptrs, ptrs, ptrs,
                                      (1 << L) - 1, 0.0, out and p, widths[-1], tap and p, tap_layer, ldt, None), buf


def test_fp_infer_launcher_rejects_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    rc, _ = _call(lib, [200, 100], True, True)
    assert rc == -1
    assert b"no kernel" in lib.pcl_last_error()
    rc, _ = _call(lib, [128, 128, 128, 128, 65], True, True)
    assert rc == -1
    assert b"no kernel" in lib.pcl_last_error()
    rc, _ = _call(lib, [256, 256], True, False)           # out NULL
    assert rc == -1
    assert b"null pointer" in lib.pcl_last_error()
    rc, _ = _call(lib, [256, 256], False, True)           # no layer-1 input at all
    assert rc == -1
    assert b"no input" in lib.pcl_last_error()
    rc, _ = _call(lib, [128, 128, 128], True, True, tap=True, tap_layer=2, ldt=128)     # the last layer is no tap
    assert rc == -1
    assert b"tap_layer" in lib.pcl_last_error()


def test_frozen_accepts_the_partseg_pointnets():
    from pointcloudlib_amd.inference import FrozenPointNet2Partseg, frozen
    from pointcloudlib_amd.networks.seg.pointnet2_partseg import PointNet2_partseg, PointNetMSG
    for cls in (PointNet2_partseg, PointNetMSG):
        fnet = frozen(cls())
        assert isinstance(fnet, FrozenPointNet2Partseg)
        assert [k for k, _ in fnet.fp.values()] == ["fused", "fused", "fused"]
        assert fnet.head_fused
        assert [[k for k, _ in lv] for lv in fnet.levels][2] == ["all"]


def test_frozen_partseg_plan_falls_back_for_other_widths():
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.misc.ops import PointNetFeaturePropagation
    from pointcloudlib_amd.networks.seg.pointnet2_partseg import PointNetMSG
    net = PointNetMSG(part_num=70)                          # part_num > 64: FP1 fused, the head on its own modules
    fnet = frozen(net)
    assert fnet.fp["fp1"][0] == "fused" and not fnet.head_fused
    net = PointNetMSG()
    net.fp2 = PointNetFeaturePropagation(576, [200, 100])
    net.fp1 = PointNetFeaturePropagation(100 + 22, [128, 128, 128])
    fnet = frozen(net)
    assert [fnet.fp[k][0] for k in ("fp3", "fp2", "fp1")] == ["fused", "module", "fused"]


def test_frozen_still_rejects_other_partseg_networks():
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.networks.seg.dgcnn_partseg import DGCNN_partseg
    from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
    for net in (DGCNN_partseg(part_num=50), PointNet_partseg(part_num=50)):
        with pytest.raises(TypeError, match="PointNet2_cls or PointNetMSG"):
            frozen(net)


def test_train_partseg_fast_eval_refuses_other_models():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "train_partseg.py"), "--model", "dgcnn", "--fast_eval"], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--fast_eval: --model pointnet2 or pointnet2_msg only" in r.stderr
