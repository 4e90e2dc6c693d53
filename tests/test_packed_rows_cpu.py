"""Packed rows of a ragged batch (csrc/pack.hip) without a GPU: the five entry points are declared, typed and
exported; every launcher rejects bad arguments on the host before any HIP call; ``row_offsets`` validates host-side lengths like
every other ragged operator; the dense ``forward`` of the part-seg networks still refuses ``lengths``."""
import ctypes

import pytest
import torch

PACKED = {"pcl_row_offsets_i32": 5, "pcl_fp_pack_rows_f32": 16, "pcl_fp_pack_rows_bwd_f32": 15, "pcl_pack_rows_b32": 11,
          "pcl_unpack_rows_b32": 11}


def test_packed_entry_points_are_declared_typed_and_exported():
    from pointcloudlib_amd import _lib
    L = ctypes.CDLL(_lib.so_path())
    for name, arity in PACKED.items():
        assert name in _lib.declared_symbols(), f"{name} not declared in include/pcl_hip.h"
        assert name in _lib._SIGS
        assert hasattr(L, name), f"{name} not exported"
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == arity, name
        assert args[-1] is ctypes.c_void_p, f"{name}: the stream comes last"
    # pack and unpack are each other's gradient: one signature
    assert _lib._SIGS["pcl_pack_rows_b32"] == _lib._SIGS["pcl_unpack_rows_b32"]
    # the header's arities are those of the table (a declaration's parameters are its top-level commas + 1)
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(_lib._HEADER).read(), flags=re.S)
    for name, arity in PACKED.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt).group(1)
        assert params.count(",") + 1 == arity, name


def _ptr():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_packed_launchers_reject_bad_arguments_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    keep, p = _ptr()
    err = lib.pcl_last_error
    # row offsets
    assert lib.pcl_row_offsets_i32(None, 2, 8, p, None) == -1 and b"pcl_row_offsets_i32: null" in err()
    assert lib.pcl_row_offsets_i32(p, 2, 8, None, None) == -1 and b"null" in err()
    assert lib.pcl_row_offsets_i32(p, 65536, 8, p, None) == -1 and b"bad sizes" in err()
    assert lib.pcl_row_offsets_i32(p, 0, 8, p, None) == -1 and b"bad sizes" in err()
    # FP rows, forward: (onehot, n_onehot, skip, CS, points2, idx3, w3, n_valid, row_off, B, N, S, D2, n_rows, rows, stream)
    fwd = lib.pcl_fp_pack_rows_f32
    assert fwd(p, 16, p, 6, None, p, p, p, p, 2, 8, 4, 128, 10, p, None) == -1 and b"pcl_fp_pack_rows_f32: null pointer" in err()
    assert fwd(p, 16, p, 6, p, p, p, None, p, 2, 8, 4, 128, 10, p, None) == -1 and b"null pointer" in err()
    assert fwd(p, 16, p, 6, p, p, p, p, None, 2, 8, 4, 128, 10, p, None) == -1 and b"null pointer" in err()
    assert fwd(p, 16, p, 6, p, p, p, p, p, 2, 8, 4, 128, 10, None, None) == -1 and b"null pointer" in err()
    assert fwd(None, 16, p, 6, p, p, p, p, p, 2, 8, 4, 128, 10, p, None) == -1 and b"onehot" in err()
    assert fwd(p, 16, None, 6, p, p, p, p, p, 2, 8, 4, 128, 10, p, None) == -1 and b"skip" in err()
    assert fwd(p, 16, p, 6, p, None, p, p, p, 2, 8, 4, 128, 10, p, None) == -1 and b"idx3 / w3" in err()
    assert fwd(p, 16, p, 6, p, p, None, p, p, 2, 8, 4, 128, 10, p, None) == -1 and b"idx3 / w3" in err()
    assert fwd(p, 16, p, 6, p, p, p, p, p, 2, 8, 0, 128, 10, p, None) == -1 and b"S=0" in err()
    assert fwd(p, 16, p, 6, p, p, p, p, p, 65536, 8, 4, 128, 10, p, None) == -1 and b"B <= 65535" in err()
    assert fwd(p, 16, p, 6, p, p, p, p, p, 2, 8, 4, 128, -1, p, None) == -1 and b"n_rows=-1" in err()
    assert fwd(p, 16, p, 6, p, p, p, p, p, 2, 8, 4, 128, 17, p, None) == -1 and b"n_rows=17" in err()
    # nothing to do is not an error and launches nothing: no cloud, no row (nullable blocks absent, S == 1 without idx3 / w3)
    assert fwd(None, 0, None, 0, p, None, None, p, p, 0, 8, 1, 128, 0, p, None) == 0
    assert fwd(None, 0, None, 0, p, None, None, p, p, 2, 8, 1, 128, 0, p, None) == 0
    # FP rows, backward: (grows, n_onehot, CS, idx3, w3, n_valid, row_off, B, N, S, D2, n_rows, gpoints2, gskip, stream)
    bwd = lib.pcl_fp_pack_rows_bwd_f32
    assert bwd(None, 16, 6, p, p, p, p, 2, 8, 4, 128, 10, p, None, None) == -1 and b"pcl_fp_pack_rows_bwd_f32: null pointer" in err()
    assert bwd(p, 16, 6, p, p, p, p, 2, 8, 4, 128, 10, None, None, None) == -1 and b"null pointer" in err()
    assert bwd(p, 16, 6, None, p, p, p, 2, 8, 4, 128, 10, p, None, None) == -1 and b"idx3 / w3" in err()
    assert bwd(p, 16, 6, p, p, p, p, 2, 8, 0, 128, 10, p, None, None) == -1 and b"S=0" in err()
    assert bwd(p, 16, 6, p, p, p, p, 65536, 8, 4, 128, 10, p, None, None) == -1 and b"B <= 65535" in err()
    assert bwd(p, 16, 6, p, p, p, p, 2, 8, 4, 128, -1, p, None, None) == -1 and b"n_rows=-1" in err()
    assert bwd(p, 16, 0, p, p, p, p, 2, 8, 4, 128, 10, p, p, None) == -1 and b"gskip given with CS=0" in err()
    # generic rows: (src, n_valid, row_off, B, N, W, ld, col0, n_rows, dst, stream)
    for name in ("pcl_pack_rows_b32", "pcl_unpack_rows_b32"):
        fn = getattr(lib, name)
        assert fn(None, p, p, 2, 8, 2, 2, 0, 10, p, None) == -1 and (name + ": null pointer").encode() in err()
        assert fn(p, None, p, 2, 8, 2, 2, 0, 10, p, None) == -1 and b"null pointer" in err()
        assert fn(p, p, None, 2, 8, 2, 2, 0, 10, p, None) == -1 and b"null pointer" in err()
        assert fn(p, p, p, 2, 8, 2, 2, 0, 10, None, None) == -1 and b"null pointer" in err()
        assert fn(p, p, p, 65536, 8, 2, 2, 0, 10, p, None) == -1 and b"B <= 65535" in err()
        assert fn(p, p, p, 2, 8, 2, 2, 0, -1, p, None) == -1 and b"n_rows=-1" in err()
        assert fn(p, p, p, 2, 8, 0, 2, 0, 10, p, None) == -1 and b"bad window" in err()
        assert fn(p, p, p, 2, 8, 6, 150, 145, 10, p, None) == -1 and b"bad window" in err()          # col0 + W > ld
        assert fn(p, p, p, 2, 8, 6, 150, -1, 10, p, None) == -1 and b"bad window" in err()
        assert fn(p, p, p, 0, 8, 2, 2, 0, 0, p, None) == 0
    del keep


def test_row_offsets_rejects_what_lengths_rejects():
    """Host-side lengths are validated before any library call; with good lengths on the CPU the call then says there is no CPU path."""
    from pointcloudlib_amd.misc import ops
    cpu = torch.device("cpu")
    bad = [([8], "shape"), ([8, 8, 8], "shape"), ([[8, 8]], "shape"), ([0, 8], r"lengths\[0\]=0"), ([8, 9], r"lengths\[1\]=9"),
           (torch.tensor([8, -1]), r"lengths\[1\]=-1")]
    for lengths, what in bad:
        with pytest.raises(ValueError, match=what):
            ops.row_offsets(lengths, 2, 8, cpu)
    with pytest.raises(TypeError, match="integers"):
        ops.row_offsets([8.0, 8.0], 2, 8, cpu)
    with pytest.raises(ValueError, match="None"):
        ops.row_offsets(None, 2, 8, cpu)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.row_offsets([8, 3], 2, 8, cpu)
    # the other three operators refuse CPU tensors and odd element sizes
    x = torch.zeros(2, 8, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pack_rows(x, [8, 3], torch.zeros(3, dtype=torch.int32), 11)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.unpack_rows(torch.zeros(11, 5), [8, 3], torch.zeros(3, dtype=torch.int32), 8)
    with pytest.raises(ValueError, match=r"lengths\[1\]=9"):
        ops.pack_rows(x, [8, 9], torch.zeros(3, dtype=torch.int32), 11)
    with pytest.raises(TypeError, match="4 or 8 bytes"):
        ops._words(torch.zeros(2, dtype=torch.float16), "rows")
    assert ops._words(torch.zeros(2, dtype=torch.int64), "rows") == 2 and ops._words(torch.zeros(2), "rows") == 1
    with pytest.raises(ValueError, match="S == 1"):
        ops.interpolate_pack(torch.zeros(2, 4, 7), None, None, [8, 3], torch.zeros(3, dtype=torch.int32), 11, 8)
    for name in ("row_offsets", "pack_rows", "unpack_rows", "interpolate_pack"):
        assert name in ops.__all__


def test_partseg_dense_forward_still_refuses_lengths_and_names_the_packed_entry():
    from pointcloudlib_amd.networks.seg.pointnet2_partseg import PointNet2_partseg, PointNetMSG
    x = torch.zeros(2, 1024, 3)
    for cls in (PointNet2_partseg, PointNetMSG):
        assert callable(getattr(cls, "forward_packed"))
        with pytest.raises(NotImplementedError, match=r"frozen\(net\)") as e:
            cls()(x, x, torch.zeros(2, 16), lengths=[1024, 600])
        assert "forward_packed" in str(e.value)
        # the packed entry validates host-side lengths before anything touches the device
        with pytest.raises(ValueError, match=r"lengths\[1\]=511 is less than n_samples=512"):
            cls().forward_packed(x, x, torch.zeros(2, 16), lengths=[1024, 511])
    from pointcloudlib_amd.misc.ops import PointNetFeaturePropagation
    assert callable(getattr(PointNetFeaturePropagation, "forward_packed"))
