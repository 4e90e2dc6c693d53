"""Frozen PointNet inference (pointcloudlib_amd/inference.py: FrozenPointNet, csrc/infer_pointnet.hip): the parts that need no GPU."""
import ctypes

import pytest

_NAMES = ("pcl_pointnet_stack_infer_supported", "pcl_pointnet_stack_infer_workspace_bytes", "pcl_pointnet_stack_infer_f32",
          "pcl_pointnet_stack_infer_splits")
_WIDTHS = (64, 64, 64, 128, 1024)


def _w(*widths):
    return (ctypes.c_int32 * len(widths))(*widths)


def test_pointnet_infer_symbols_declared_and_exported():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    for name in _NAMES:
        assert name in _lib.declared_symbols()
        assert name in _lib._SIGS
        assert hasattr(lib, name)


def test_pointnet_infer_supported_shapes():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert lib.pcl_pointnet_stack_infer_supported(3, 5, _w(*_WIDTHS)) == 1
    assert lib.pcl_pointnet_stack_infer_supported(3, 4, _w(64, 64, 128, 1024)) == 0
    assert lib.pcl_pointnet_stack_infer_supported(3, 5, _w(64, 64, 96, 128, 1024)) == 0
    assert lib.pcl_pointnet_stack_infer_supported(4, 5, _w(*_WIDTHS)) == 0
    assert lib.pcl_pointnet_stack_infer_supported(3, 5, _w(64, 64, 64, 128, 1000)) == 0


def test_pointnet_infer_sizes_are_pure_functions():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert lib.pcl_pointnet_stack_infer_workspace_bytes(32, 1024, 1024) == 4 * 32 * 16 * 1024
    assert lib.pcl_pointnet_stack_infer_workspace_bytes(3, 65, 1024) == 4 * 3 * 2 * 1024
    # the column splits of the last layer: 4 up to 128 tiles, 2 up to 256, else 1
    assert [lib.pcl_pointnet_stack_infer_splits(b, n) for b, n in [(1, 64), (8, 1024), (2, 64 * 64 + 1), (16, 1024), (17, 1024), (32, 1024)]] \
        == [4, 4, 2, 2, 1, 1]


def _launch(lib, widths, C0=3, out=True, ws_bytes=None, B=2, N=100):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    L = len(widths)
    ptrs = (ctypes.c_void_p * L)(*[p] * L)
    if ws_bytes is None:
        ws_bytes = lib.pcl_pointnet_stack_infer_workspace_bytes(B, N, widths[-1])
    return lib.pcl_pointnet_stack_infer_f32(p, 3 * N, 1, N, None, B, N, C0, p, 3, L, _w(*widths), ptrs, ptrs, ptrs, 0.0, p, ws_bytes,
                                            p if out else None, 1024, None)


def test_pointnet_infer_launcher_rejects_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    assert _launch(lib, (64, 64, 96, 128, 1024)) == -1
    assert b"no kernel" in lib.pcl_last_error()
    assert _launch(lib, (64, 64, 128, 1024)) == -1
    assert b"no kernel" in lib.pcl_last_error()
    assert _launch(lib, _WIDTHS, C0=4) == -1
    assert b"no kernel" in lib.pcl_last_error()
    assert _launch(lib, _WIDTHS, out=False) == -1
    assert b"null pointer" in lib.pcl_last_error()
    need = lib.pcl_pointnet_stack_infer_workspace_bytes(2, 100, 1024)
    assert _launch(lib, _WIDTHS, ws_bytes=need - 4) == _lib.define("PCL_EWS")
    assert b"workspace" in lib.pcl_last_error()


def test_frozen_pointnet_plans():
    from pointcloudlib_amd.inference import FrozenPointNet
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    net = PointNet()
    assert FrozenPointNet(net).plan == "fused"
    net.convs = PointwiseMLP([3, 64, 64, 96, 1024], bias=False)
    assert FrozenPointNet(net).plan == "module"


def test_frozen_pointnet_rejects_other_networks():
    from pointcloudlib_amd.inference import FrozenPointNet, frozen
    from pointcloudlib_amd.networks.cls.dgcnn import DGCNN
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    with pytest.raises(TypeError, match="PointNet"):
        FrozenPointNet(DGCNN())
    with pytest.raises(TypeError, match="PointNet2_cls or PointNetMSG"):
        frozen(PointNet())


def test_train_cls_fast_eval_refuses_other_models():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "train_cls.py"), "--model", "dgcnn", "--fast_eval"], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--fast_eval: --model pointnet2 or pointnet only" in r.stderr
