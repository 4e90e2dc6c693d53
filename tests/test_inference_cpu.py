"""Frozen inference (pointcloudlib_amd/inference.py, csrc/infer.hip): the parts that need no GPU."""
import ctypes

import pytest


def test_infer_symbols_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for name in ("pcl_sa_level_infer_f32", "pcl_sa_level_infer_supported"):
        assert name in _lib.declared_symbols()
        assert name in _lib._SIGS
        assert hasattr(lib, name)


def test_infer_supported_shapes():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    table = [(64, 64, 64, 128), (64, 128, 128, 256), (16, 32, 32, 64), (32, 64, 64, 128), (128, 64, 96, 128), (32, 64, 64, 128),
             (64, 128, 128, 256), (128, 128, 128, 256)]
    for ns, c1, c2, c3 in table:
        assert lib.pcl_sa_level_infer_supported(ns, 3, c1, c2, c3, 0) == 1, (ns, c1, c2, c3)
    assert lib.pcl_sa_level_infer_supported(64, 3, 128, 128, 288, 0) == 0
    assert lib.pcl_sa_level_infer_supported(64, 2, 64, 128, 0, 0) == 0
    assert lib.pcl_sa_level_infer_supported(0, 3, 64, 64, 128, 0) == 0


def test_infer_launcher_rejects_other_shapes_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    widths = (ctypes.c_int32 * 3)(128, 128, 288)
    rc = lib.pcl_sa_level_infer_f32(p, p, p, p, None, None, 0, 3, p, p, 1, 8, 4, 8, 3, widths, ptrs, ptrs, ptrs, 0.0, p, 288, 0, None)
    assert rc == -1
    assert b"no kernel" in lib.pcl_last_error()


def test_frozen_rejects_other_networks():
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.networks.cls.dgcnn import DGCNN
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    for net in (DGCNN(), PointNet()):
        with pytest.raises(TypeError, match="PointNet2_cls or PointNetMSG"):
            frozen(net)
