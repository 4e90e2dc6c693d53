"""Ragged batches (``lengths=`` / ``n_valid``) without a GPU: the entry points are declared, typed and exported; every launcher
rejects bad arguments on the host; the Python helper validates host-side lengths before any library call; the networks that cannot
take ``lengths`` say so."""
import ctypes

import pytest
import torch

RAGGED = ["pcl_fps_ragged_f32", "pcl_ball_query_ragged_f32", "pcl_ball_query_multi_ragged_f32", "pcl_three_nn_ragged_f32",
          "pcl_fp_level_infer_ragged_f32"]


def test_ragged_entry_points_are_declared_typed_and_exported():
    from pointcloudlib_amd import _lib
    L = ctypes.CDLL(_lib.so_path())
    for name in RAGGED:
        assert name in _lib.declared_symbols()
        assert name in _lib._SIGS
        assert hasattr(L, name), f"{name} not exported"
    dense = {"pcl_fps_ragged_f32": "pcl_fps_f32", "pcl_ball_query_ragged_f32": "pcl_ball_query_f32",
             "pcl_ball_query_multi_ragged_f32": "pcl_ball_query_multi_f32", "pcl_fp_level_infer_ragged_f32": "pcl_fp_level_infer_f32"}
    for r, d in dense.items():            # the dense signature plus ONE pointer
        assert len(_lib._SIGS[r][1]) == len(_lib._SIGS[d][1]) + 1
    assert len(_lib._SIGS["pcl_three_nn_ragged_f32"][1]) == len(_lib._SIGS["pcl_three_nn_f32"][1]) + 2


def _ptr():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_ragged_launchers_reject_bad_arguments_on_the_host():
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    keep, p = _ptr()
    err = lib.pcl_last_error
    # FPS
    assert lib.pcl_fps_ragged_f32(p, None, 1, 8, 4, 1, 1e-3, None, p, None, None) == -1 and b"pcl_fps_ragged_f32: null" in err()
    assert lib.pcl_fps_ragged_f32(None, p, 1, 8, 4, 1, 1e-3, None, p, None, None) == -1 and b"null" in err()
    assert lib.pcl_fps_ragged_f32(p, p, 1, 8, 9, 1, 1e-3, None, p, None, None) == -1 and b"m <= N" in err()
    assert lib.pcl_fps_ragged_f32(p, p, 1, 8, 4, 3, 1e-3, None, p, None, None) == -1 and b"tie_stride" in err()
    # ball query
    assert lib.pcl_ball_query_ragged_f32(p, p, None, 1, 4, 8, 0.2, 4, p, None, None) == -1 and b"pcl_ball_query_ragged_f32: null" in err()
    assert lib.pcl_ball_query_ragged_f32(p, p, p, 1, 4, 0, 0.2, 4, p, None, None) == -1 and b"bad sizes" in err()
    assert lib.pcl_ball_query_ragged_f32(p, p, p, 65536, 4, 8, 0.2, 4, p, None, None) == -1 and b"grid.y" in err()
    # multi-radius ball query
    radii = (ctypes.c_float * 3)(0.1, 0.2, 0.4)
    ns = (ctypes.c_int32 * 3)(4, 4, 4)
    outs = (ctypes.c_void_p * 3)(p, p, p)
    assert lib.pcl_ball_query_multi_ragged_f32(p, p, None, 1, 4, 8, 3, radii, ns, outs, None, None) == -1
    assert b"pcl_ball_query_multi_ragged_f32: null" in err()
    assert lib.pcl_ball_query_multi_ragged_f32(p, p, p, 1, 4, 8, 5, radii, ns, outs, None, None) == -1 and b"n_radii" in err()
    assert lib.pcl_ball_query_multi_ragged_f32(p, p, p, 65536, 4, 8, 3, radii, ns, outs, None, None) == -1 and b"bad sizes" in err()
    ns0 = (ctypes.c_int32 * 3)(4, 0, 4)
    assert lib.pcl_ball_query_multi_ragged_f32(p, p, p, 1, 4, 8, 3, radii, ns0, outs, None, None) == -1 and b"radius 1" in err()
    # 3-NN: either count pointer may be null, the clouds and outputs may not
    assert lib.pcl_three_nn_ragged_f32(None, p, p, p, 1, 8, 4, p, p, None) == -1 and b"pcl_three_nn_ragged_f32: null" in err()
    assert lib.pcl_three_nn_ragged_f32(p, None, p, None, 1, 8, 0, p, p, None) == -1 and b"bad sizes" in err()
    assert lib.pcl_three_nn_ragged_f32(p, None, p, None, 65536, 8, 4, p, p, None) == -1 and b"bad sizes" in err()
    # FP level: no kernel for the widths; a null count pointer
    ptrs = (ctypes.c_void_p * 2)(p, p)
    w_bad = (ctypes.c_int32 * 2)(200, 100)
    w_ok = (ctypes.c_int32 * 2)(256, 256)
    args = lambda w, nv: (p, None, None, 0, 0, None, None, None, 1, None, nv, 1, 8, 2, w, ptrs, ptrs, ptrs, 3, 0.0, p, 256, None, -1, 0, None)
    assert lib.pcl_fp_level_infer_ragged_f32(*args(w_bad, p)) == -1 and b"no kernel" in err()
    assert lib.pcl_fp_level_infer_ragged_f32(*args(w_ok, None)) == -1 and b"pcl_fp_level_infer_ragged_f32: null pointer (n_valid)" in err()
    del keep


def test_host_side_lengths_are_validated_before_any_library_call():
    """With CPU clouds the length error must win over "expected a tensor on the GPU"; good lengths then reach that error."""
    from pointcloudlib_amd.misc import ops
    x = torch.zeros(2, 8, 3)
    q = torch.zeros(2, 4, 3)
    bad = [([8], "shape"), ([8, 8, 8], "shape"), ([[8, 8]], "shape"), ([0, 8], r"lengths\[0\]=0"), ([8, 9], r"lengths\[1\]=9"),
           (torch.tensor([8, -1]), r"lengths\[1\]=-1")]
    for lengths, what in bad:
        for fn in (lambda: ops.furthest_point_sample(x, 4, lengths=lengths), lambda: ops.ball_query(q, x, 0.1, 2, lengths=lengths),
                   lambda: ops.ball_query_multi(q, x, [0.1, 0.2], [2, 2], lengths=lengths),
                   lambda: ops.FurthestPointSampler(4)(x, lengths=lengths),
                   lambda: ops.BallQueryGrouper(0.1, 2, True)(q, x, None, lengths=lengths)):
            with pytest.raises(ValueError, match=what):
                fn()
        with pytest.raises(ValueError, match=what.replace("lengths", "lengths1")):
            ops.three_nn(x, q, lengths1=lengths)
    with pytest.raises(ValueError, match=r"lengths2\[1\]=5 must be in \[1, N=4\]"):
        ops.three_nn(x, q, lengths2=[4, 5])
    with pytest.raises(ValueError, match=r"lengths\[1\]=3 is less than n_samples=4"):
        ops.furthest_point_sample(x, 4, lengths=[8, 3])
    with pytest.raises(TypeError, match="integers"):
        ops.furthest_point_sample(x, 4, lengths=[8.0, 8.0])
    for fn in (lambda: ops.furthest_point_sample(x, 4, lengths=[8, 4]), lambda: ops.ball_query(q, x, 0.1, 2, lengths=(8, 1)),
               lambda: ops.three_nn(x, q, lengths1=torch.tensor([8, 1]), lengths2=[1, 4])):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()
    # the helper itself: None stays None (the dense path), a host sequence becomes int32 [B]
    assert ops._lengths(None, 2, 8, x.device) is None
    t = ops._lengths([8, 5], 2, 8, x.device)
    assert t.dtype == torch.int32 and t.tolist() == [8, 5]


def test_sampling_rejects_bad_lengths_and_group_all_on_a_ragged_cloud():
    from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls, PointnetModule
    x = torch.zeros(2, 1024, 3)
    net = PointNet2_cls()
    with pytest.raises(ValueError, match=r"lengths\[1\]=511 is less than n_samples=512"):
        net.pointnet_modules[0].sample(x, lengths=[1024, 511])
    with pytest.raises(NotImplementedError, match="masked max"):
        PointnetModule(mlp=[3, 8]).sample(x, lengths=[1024, 600])


def test_partseg_training_forward_refuses_lengths():
    from pointcloudlib_amd.networks.seg.pointnet2_partseg import PointNet2_partseg, PointNetMSG
    x = torch.zeros(2, 1024, 3)
    for cls in (PointNet2_partseg, PointNetMSG):
        with pytest.raises(NotImplementedError, match=r"frozen\(net\)"):
            cls()(x, x, torch.zeros(2, 16), lengths=[1024, 600])


def test_frozen_still_rejects_other_networks():
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.networks.cls.dgcnn import DGCNN
    with pytest.raises(TypeError, match="PointNet2_cls or PointNetMSG"):
        frozen(DGCNN())
