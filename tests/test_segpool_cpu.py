"""Pooling over the clouds of packed rows (csrc/segpool.hip) without a GPU: the five entry points are
declared, typed and exported; every launcher rejects bad arguments on the host before any HIP call, naming itself; the ragged
PointNet validates host-side ``lengths`` like every other ragged operator, before anything touches the device."""
import ctypes
import re

import pytest
import torch

SEGPOOL = {"pcl_row_cloud_i32": 5, "pcl_bn_act_seg_max_f32": 11, "pcl_bn_act_seg_max_bwd_f32": 16, "pcl_seg_broadcast_rows_f32": 7,
           "pcl_seg_sum_rows_f32": 7}


def test_segpool_entry_points_are_declared_typed_and_exported():
    from pointcloudlib_amd import _lib
    L = ctypes.CDLL(_lib.so_path())
    txt = re.sub(r"/\*.*?\*/", "", open(_lib._HEADER).read(), flags=re.S)
    for name, arity in SEGPOOL.items():
        assert name in _lib.declared_symbols(), f"{name} not declared in include/pcl_hip.h"
        assert name in _lib._SIGS, f"{name} not typed in _lib._SIGS"
        assert hasattr(L, name), f"{name} not exported"
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == arity, name
        assert args[-1] is ctypes.c_void_p, f"{name}: the stream comes last"
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt).group(1)
        assert params.count(",") + 1 == arity, f"{name}: the header's arity differs from the table's"
        assert params.split(",")[-1].strip() == "void* stream", name


def _ptr():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _each_null(fn, args, pointer_slots, name, err):
    for k in pointer_slots:
        a = list(args)
        a[k] = None
        assert fn(*a) == -1 and (name + ": null pointer").encode() in err(), f"{name}: argument {k} = NULL"


def test_segpool_launchers_reject_bad_arguments_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    keep, p = _ptr()
    rows_out = ctypes.c_int(0)
    ro = ctypes.byref(rows_out)
    err = lib.pcl_last_error
    f = ctypes.c_float

    def sizes(fn, name, make):
        """make(B, C, n_rows) -> argument list"""
        for B, C, n_rows, what in ((0, 8, 10, b"B=0"), (65536, 8, 10, b"B=65536"), (2, 0, 10, b"C=0"), (2, 8, -1, b"n_rows=-1")):
            if C == 0 and name == "pcl_row_cloud_i32":
                continue
            assert fn(*make(B, C, n_rows)) == -1, (name, B, C, n_rows)
            msg = err()
            assert name.encode() in msg and what in msg, msg

    # (row_off, B, n_rows, row_cloud, stream)
    name, fn = "pcl_row_cloud_i32", lib.pcl_row_cloud_i32
    _each_null(fn, (p, 2, 10, p, None), (0, 3), name, err)
    sizes(fn, name, lambda B, C, n: (p, B, n, p, None))
    assert fn(p, 2, 0, p, None) == 0                                                   # no row: nothing to do, nothing launched
    # (Y, row_off, scale, shift, slope, B, C, n_rows, out, arg, stream)
    name, fn = "pcl_bn_act_seg_max_f32", lib.pcl_bn_act_seg_max_f32
    _each_null(fn, (p, p, p, p, f(0.2), 2, 8, 10, p, p, None), (0, 1, 2, 3, 8, 9), name, err)
    sizes(fn, name, lambda B, C, n: (p, p, p, p, f(0.2), B, C, n, p, p, None))
    # (gmax, ldg, arg, Y, scale, shift, slope, row_off, row_cloud, B, C, n_rows, du, stats_ws, stat_rows_out, stream)
    name, fn = "pcl_bn_act_seg_max_bwd_f32", lib.pcl_bn_act_seg_max_bwd_f32
    _each_null(fn, (p, 8, p, p, p, p, f(0.2), p, p, 2, 8, 10, p, p, ro, None), (0, 2, 3, 4, 5, 7, 8, 12, 13, 14), name, err)
    sizes(fn, name, lambda B, C, n: (p, max(C, 1), p, p, p, p, f(0.2), p, p, B, C, n, p, p, ro, None))
    assert fn(p, 7, p, p, p, p, f(0.2), p, p, 2, 8, 10, p, p, ro, None) == -1
    assert name.encode() in err() and b"ldg=7" in err()
    # (src, row_cloud, B, C, n_rows, dst, stream)
    name, fn = "pcl_seg_broadcast_rows_f32", lib.pcl_seg_broadcast_rows_f32
    _each_null(fn, (p, p, 2, 8, 10, p, None), (0, 1, 5), name, err)
    sizes(fn, name, lambda B, C, n: (p, p, B, C, n, p, None))
    assert fn(p, p, 2, 8, 0, p, None) == 0
    # (g, row_off, B, C, n_rows, gsrc, stream)
    name, fn = "pcl_seg_sum_rows_f32", lib.pcl_seg_sum_rows_f32
    _each_null(fn, (p, p, 2, 8, 10, p, None), (0, 1, 5), name, err)
    sizes(fn, name, lambda B, C, n: (p, p, B, C, n, p, None))
    del keep


def test_ragged_pointnet_rejects_what_lengths_rejects():
    from pointcloudlib_amd.misc import ops
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
    from pointcloudlib_amd.misc.stn import STN3d, STNkd
    net = PointNet()
    x = torch.zeros(2, 3, 8)
    bad = [([8], "shape"), ([8, 8, 8], "shape"), ([[8, 8]], "shape"), ([0, 8], r"lengths\[0\]=0"), ([8, 9], r"lengths\[1\]=9"),
           (torch.tensor([8, -1]), r"lengths\[1\]=-1")]
    for lengths, what in bad:
        with pytest.raises(ValueError, match=what):
            net(x, lengths=lengths)
        with pytest.raises(ValueError, match=what):
            PointNet_partseg().forward_packed(x, torch.zeros(2, 16), lengths=lengths)
    with pytest.raises(TypeError, match="integers"):
        net(x, lengths=[8.0, 8.0])
    with pytest.raises(TypeError, match="integers"):
        ops.packed_layout([8.0, 3.0], 2, 8, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="GPU"):                                     # good lengths: there is no CPU path
        net(x, lengths=[8, 3])
    assert callable(getattr(STNkd, "forward_packed")) and STN3d.forward_packed is STNkd.forward_packed
    for name in ("row_cloud", "segment_max", "broadcast_rows"):
        assert name in ops.__all__
