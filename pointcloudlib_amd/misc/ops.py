"""Point-cloud operators -- host-side mirror of the reference's ``misc/ops.py``.

Same class names, constructor arguments, call arguments, shapes, dtypes and channel-last layouts as
/root/reference/misc/ops.py (FurthestPointSampler :114, BallQueryGrouper :289, GroupAll :410,
KNN :422, PointNetFeaturePropagation :54, index_points :12), written as ``torch.nn.Module``s with an
``execute`` alias for Jittor's method name.  All arithmetic runs in ``libpcl_hip.so`` (hand-written
gfx950 kernels) through the C ABI of ``include/pcl_hip.h``; PyTorch only owns the device buffers, the
stream and autograd bookkeeping.  CPU tensors are rejected: there is no fallback path.
"""
import math

import os

import torch
from torch import nn

from .. import _lib

__all__ = [
    "optimal_block", "furthest_point_sample", "ball_query", "ball_query_multi", "group_offsets_multi", "group_points", "group_points_compact", "RowSet", "group_all",
    "index_points",
    "knn_indices", "edge_features", "three_nn", "three_interpolate", "row_offsets", "pack_rows", "unpack_rows", "interpolate_pack",
    "row_cloud", "packed_layout", "segment_max", "mlp_segment_max", "broadcast_rows",
    "FurthestPointSampler", "BallQueryGrouper", "GroupAll",
    "KNN", "PointNetFeaturePropagation",
]


# ----------------------------------------------------------------------------- plumbing
def _dev(t, name, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the GPU (libpcl_hip has no CPU path), got {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    # the raw hipStream_t of torch's current stream (torch.cuda.current_stream().cuda_stream costs ~10 us of Python per call)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _lengths(lengths, B, N, device, name="lengths", n_samples=None):
    """Per-cloud point counts of a ragged batch -> device int32 [B] (``None`` stays ``None``: the dense path).

    A batch is [B, N, .] with N the capacity; cloud b is its first ``lengths[b]`` rows, the rest are pad rows that influence no
    result.  A Python sequence or a CPU tensor is validated here (shape [B], ``1 <= lengths[b] <= N`` and, for FPS,
    ``n_samples <= lengths[b]``) and copied once.  A device tensor must be int32 [B] and is NOT read back (no host
    synchronisation): the same bounds are the caller's precondition, and the kernels clamp every count to [1, N]."""
    if lengths is None:
        return None
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if lengths.dtype != torch.int32:
            raise TypeError(f"{name}: a device tensor must be torch.int32, got {lengths.dtype}")
        if lengths.dim() != 1 or lengths.shape[0] != B:
            raise ValueError(f"{name}: expected shape [{B}], got {tuple(lengths.shape)}")
        if lengths.device != device:
            raise ValueError(f"{name}: on {lengths.device}, the clouds on {device}")
        return lengths.contiguous()
    host = lengths.detach() if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths)
    if host.dtype.is_floating_point or host.dtype == torch.bool or host.dtype.is_complex:
        raise TypeError(f"{name}: expected integers, got {host.dtype}")
    if host.dim() != 1 or host.shape[0] != B:
        raise ValueError(f"{name}: expected shape [{B}] (one count per cloud), got {tuple(host.shape)}")
    vals = host.tolist()
    for b, v in enumerate(vals):
        if not 1 <= v <= N:
            raise ValueError(f"{name}[{b}]={v} must be in [1, N={N}]")
        if n_samples is not None and v < n_samples:
            raise ValueError(f"{name}[{b}]={v} is less than n_samples={n_samples}: a cloud cannot be sampled beyond its own points")
    return torch.tensor(vals, dtype=torch.int32).to(device)


def _xyz_shape(xyz, name="xyz"):
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"{name} must be [B,N,3], got {tuple(getattr(xyz, 'shape', ()))}")
    return xyz.shape[0], xyz.shape[1]


def optimal_block(batch_size):
    """misc/ops.py:110-111 -- ``2 ** int(math.log(batch_size))`` (natural log, as written)."""
    return 2 ** int(math.log(batch_size)) if batch_size >= 1 else 1


# ----------------------------------------------------------------------------- index producers
def furthest_point_sample(xyz, n_samples, tie_stride=None, skip_sqnorm_le=1e-3, start_idx=None, lengths=None):
    """xyz [B,N,3] f32 -> (idx [B,n] int32, new_xyz [B,n,3]).  misc/ops.py:124-234, :280-284.

    ``tie_stride`` defaults to the reference's launch block size ``optimal_block(B)``, which fixes how
    exact distance ties are broken; ``skip_sqnorm_le=None`` disables the near-origin skip
    (misc/pointconv_utils.py:74-116 has none).  ``lengths`` (see ``_lengths``): per-cloud point counts of a ragged batch --
    every cloud is sampled from its own first ``lengths[b]`` points, with the picks of that cloud alone for the same
    ``tie_stride`` (the default stride is a function of B: pass it explicitly to compare with a B = 1 call)."""
    if lengths is not None:          # host-side length errors come first, before anything touches the device
        Bh, Nh = _xyz_shape(xyz)
        lengths = _lengths(lengths, Bh, Nh, xyz.device, n_samples=n_samples)
    xyz = _dev(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"xyz must be [B,N,3], got {tuple(xyz.shape)}")
    B, N, _ = xyz.shape
    if not (1 <= n_samples <= N):
        raise ValueError(f"n_samples={n_samples} must be in [1, N={N}]")  # assert at misc/ops.py:269
    if tie_stride is None:
        tie_stride = optimal_block(B)
    start_idx = _dev(start_idx, "start_idx", torch.int32)
    idx = torch.empty((B, n_samples), dtype=torch.int32, device=xyz.device)
    new_xyz = torch.empty((B, n_samples, 3), dtype=torch.float32, device=xyz.device)
    thr = -1.0 if skip_sqnorm_le is None else float(skip_sqnorm_le)
    if lengths is not None:
        _lib.call("pcl_fps_ragged_f32", _p(xyz), _p(_dev(lengths, "lengths", torch.int32)), B, N, n_samples, int(tie_stride), thr,
                  _p(start_idx), _p(idx), _p(new_xyz), _stream(), algo_bytes=B * (12 * N + 16 * n_samples))
        return idx, new_xyz
    _lib.call("pcl_fps_f32", _p(xyz), B, N, n_samples, int(tie_stride), thr, _p(start_idx), _p(idx),
                                      _p(new_xyz), _stream(), algo_bytes=B * (12 * N + 16 * n_samples))
    return idx, new_xyz


def ball_query(new_xyz, xyz, radius, n_samples, return_cnt=False, lengths=None):
    """new_xyz [B,m,3], xyz [B,N,3] -> idx [B,m,ns] int32.  misc/ops.py:291-330.  ``lengths``: per-cloud point counts of
    ``xyz`` (ragged batch, see ``_lengths``): the lists of every cloud alone, no index >= lengths[b]."""
    if lengths is not None:
        Bh, Nh = _xyz_shape(xyz)
        lengths = _lengths(lengths, Bh, Nh, xyz.device)
    new_xyz = _dev(new_xyz, "new_xyz")
    xyz = _dev(xyz, "xyz")
    if new_xyz.dim() != 3 or new_xyz.shape[2] != 3 or xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError("new_xyz / xyz must be [B,*,3]")
    if new_xyz.shape[0] != xyz.shape[0]:
        raise ValueError("batch size mismatch")   # assert at misc/ops.py:361
    B, m, _ = new_xyz.shape
    N = xyz.shape[1]
    idx = torch.empty((B, m, n_samples), dtype=torch.int32, device=xyz.device)
    cnt = torch.empty((B, m), dtype=torch.int32, device=xyz.device) if return_cnt else None
    if lengths is not None:
        _lib.call("pcl_ball_query_ragged_f32", _p(new_xyz), _p(xyz), _p(_dev(lengths, "lengths", torch.int32)), B, m, N, float(radius),
                  int(n_samples), _p(idx), _p(cnt), _stream(), algo_bytes=B * (12 * (N + m) + 4 * m * n_samples))
        return (idx, cnt) if return_cnt else idx
    _lib.call("pcl_ball_query_f32", _p(new_xyz), _p(xyz), B, m, N, float(radius), int(n_samples), _p(idx),
                                             _p(cnt), _stream(), algo_bytes=B * (12 * (N + m) + 4 * m * n_samples))
    return (idx, cnt) if return_cnt else idx


BALL_QUERY_MULTI_MAX = 4          # radii per pcl_ball_query_multi_f32 call


def ball_query_multi(new_xyz, xyz, radii, n_samples, return_cnt=False, lengths=None):
    """Ball queries of several radii around the same centres in ONE scan of the cloud (multi-scale grouping: one BallQueryGrouper per
    scale on the same new_xyz, reference networks/seg/pointnet2_partseg.py:93-103).  -> [idx [B,m,ns_r]] or [(idx, cnt)] per radius,
    each identical to ``ball_query(new_xyz, xyz, radii[r], n_samples[r])`` (``lengths`` as there)."""
    import ctypes
    if lengths is not None:
        Bh, Nh = _xyz_shape(xyz)
        lengths = _lengths(lengths, Bh, Nh, xyz.device)
    new_xyz = _dev(new_xyz, "new_xyz")
    xyz = _dev(xyz, "xyz")
    if new_xyz.dim() != 3 or new_xyz.shape[2] != 3 or xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError("new_xyz / xyz must be [B,*,3]")
    if new_xyz.shape[0] != xyz.shape[0]:
        raise ValueError("batch size mismatch")
    n = len(radii)
    if n != len(n_samples) or not 1 <= n <= BALL_QUERY_MULTI_MAX:
        raise ValueError(f"{n} radii / {len(n_samples)} sample counts: 1..{BALL_QUERY_MULTI_MAX} of each")
    B, m, _ = new_xyz.shape
    N = xyz.shape[1]
    idx = [torch.empty((B, m, int(s)), dtype=torch.int32, device=xyz.device) for s in n_samples]
    cnt = [torch.empty((B, m), dtype=torch.int32, device=xyz.device) for _ in range(n)] if return_cnt else None
    c_r = (ctypes.c_float * n)(*[float(r) for r in radii])
    c_s = (ctypes.c_int32 * n)(*[int(s) for s in n_samples])
    c_i = (ctypes.c_void_p * n)(*[t.data_ptr() for t in idx])
    c_c = (ctypes.c_void_p * n)(*[t.data_ptr() for t in cnt]) if return_cnt else None
    if lengths is not None:
        _lib.call("pcl_ball_query_multi_ragged_f32", _p(new_xyz), _p(xyz), _p(_dev(lengths, "lengths", torch.int32)), B, m, N, n, c_r, c_s,
                  c_i, c_c, _stream(), algo_bytes=B * (12 * (N + m) + 4 * m * sum(int(s) for s in n_samples)))
    else:
        _lib.call("pcl_ball_query_multi_f32", _p(new_xyz), _p(xyz), B, m, N, n, c_r, c_s, c_i, c_c, _stream(),
                  algo_bytes=B * (12 * (N + m) + 4 * m * sum(int(s) for s in n_samples)))
    return list(zip(idx, cnt)) if return_cnt else idx


# The k-NN distance has two definitions in this library: the default rounds `tmp*tmp` and the sum
# separately, as the reference's source text reads (misc/ops.py:488-491); "fma" is the NAMED second definition -- what nvcc's
# default -fmad=true makes of that line -- one VALU operation fewer per element.  Opt-in: PCL_KNN_CONTRACT=fma or
# ``ops.KNN_CONTRACT = "fma"``; each is bit-exact against the oracle evaluated under the same reading.
KNN_CONTRACT = os.environ.get("PCL_KNN_CONTRACT", "")


def knn_indices(x_q, x_r, k, contract=None):
    """KNN(k).execute(x_q [B,C,Nq], x_r [B,C,Nr]) -> int32 [B,k,Nq].  misc/ops.py:651-663."""
    contract = KNN_CONTRACT if contract is None else contract
    if contract not in ("", "fma"):
        raise ValueError(f"knn contract {contract!r}: '' (source reading) or 'fma'")
    x_q = _dev(x_q, "x_q")
    x_r = _dev(x_r, "x_r")
    if x_q.dim() != 3 or x_r.dim() != 3 or x_q.shape[:2] != x_r.shape[:2]:
        raise ValueError(f"x_q/x_r must be [B,C,N*] with equal B and C, got {tuple(x_q.shape)} {tuple(x_r.shape)}")
    B, C, Nq = x_q.shape
    Nr = x_r.shape[2]
    idx = torch.empty((B, k, Nq), dtype=torch.int32, device=x_q.device)
    nbytes = _lib.lib().pcl_knn_workspace_bytes(B, C, Nr, Nq, k)
    ws = torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.float32, device=x_q.device)   # the reference's tmp_dist
    _lib.call("pcl_knn_fma_f32" if contract == "fma" else "pcl_knn_f32", _p(x_r), _p(x_q), B, C, Nr, Nq, int(k), _p(idx), _p(ws), nbytes,
              _stream(), algo_bytes=4 * B * C * (Nr + Nq) + 4 * B * k * Nq, algo_flops=3 * B * Nr * Nq * C)
    return idx


_KNN_NK = os.environ.get("PCL_KNN_NK", "1") != "0"          # lab switch (A/B on one box): 0 = the reference-layout search + a permute copy


def knn_lists(x_q, x_r, k):
    """``knn_indices(x_q, x_r, k).permute(0, 2, 1).contiguous()`` -- the neighbour lists as [B, Nq, k] rows (what ``get_graph_feature``
    makes of KNN's result, networks/cls/dgcnn.py:34-35) -- written in that layout by the search itself where the fused kernel applies."""
    if _KNN_NK and KNN_CONTRACT == "" and x_r.is_cuda and _lib.lib().pcl_knn_nk_supported(x_r.shape[2]):
        x_q, x_r = _dev(x_q, "x_q"), _dev(x_r, "x_r")
        B, C, Nq = x_q.shape
        Nr = x_r.shape[2]
        idx = torch.empty((B, Nq, k), dtype=torch.int32, device=x_q.device)
        _lib.call("pcl_knn_nk_f32", _p(x_r), _p(x_q), B, C, Nr, Nq, int(k), _p(idx), _stream(),
                  algo_bytes=4 * B * C * (Nr + Nq) + 4 * B * k * Nq, algo_flops=3 * B * Nr * Nq * C)
        return idx
    return knn_indices(x_q, x_r, k).permute(0, 2, 1).contiguous()


def three_nn(xyz1, xyz2, lengths1=None, lengths2=None):
    """xyz1 [B,N,3] targets, xyz2 [B,S,3] sources -> (idx [B,N,3] int32, weight [B,N,3]).  ``lengths1`` / ``lengths2``: per-cloud
    counts of the targets / sources (ragged batch, see ``_lengths``; either may be None): valid targets get the triple of the
    clouds alone (no source index >= lengths2[b]), target rows beyond lengths1[b] get idx 0, weight 0."""
    if lengths1 is not None:
        Bh, Nh = _xyz_shape(xyz1, "xyz1")
        lengths1 = _lengths(lengths1, Bh, Nh, xyz1.device, "lengths1")
    if lengths2 is not None:
        Bh, Sh = _xyz_shape(xyz2, "xyz2")
        lengths2 = _lengths(lengths2, Bh, Sh, xyz2.device, "lengths2")
    xyz1 = _dev(xyz1, "xyz1")
    xyz2 = _dev(xyz2, "xyz2")
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    idx = torch.empty((B, N, 3), dtype=torch.int32, device=xyz1.device)
    w = torch.empty((B, N, 3), dtype=torch.float32, device=xyz1.device)
    if lengths1 is not None or lengths2 is not None:
        _lib.call("pcl_three_nn_ragged_f32", _p(xyz1), _p(_dev(lengths1, "lengths1", torch.int32)), _p(xyz2),
                  _p(_dev(lengths2, "lengths2", torch.int32)), B, N, S, _p(idx), _p(w), _stream())
        return idx, w
    _lib.call("pcl_three_nn_f32", _p(xyz1), _p(xyz2), B, N, S, _p(idx), _p(w), _stream())
    return idx, w


# ----------------------------------------------------------------------------- differentiable gathers
class _GroupPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, new_xyz, feat, idx, use_xyz):
        idx = _dev(idx, "idx", torch.int32)
        B, m, ns = idx.shape
        xyz = _dev(xyz, "xyz")
        new_xyz = _dev(new_xyz, "new_xyz")
        feat = _dev(feat, "feature")
        N = xyz.shape[1]
        C = 0 if feat is None else feat.shape[2]
        D = (3 if use_xyz else 0) + C
        out = torch.empty((B, m, ns, D), dtype=torch.float32, device=idx.device)
        _lib.call("pcl_group_f32", _p(xyz), _p(new_xyz), _p(feat), _p(idx), B, N, m, ns, C, int(use_xyz),
                                            _p(out), _stream(),
                  algo_bytes=B * (4 * m * ns + 12 * m + 4 * N * (3 + C) + 4 * m * ns * D))
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, m, ns, C, int(use_xyz))
        return out

    @staticmethod
    def backward(ctx, gout):
        (idx,) = ctx.saved_tensors
        B, N, m, ns, C, use_xyz = ctx.dims
        gfeat = None
        if C > 0 and ctx.needs_input_grad[2]:
            gout = _dev(gout, "grad")
            gfeat = torch.empty((B, N, C), dtype=torch.float32, device=gout.device)
            _lib.call("pcl_group_bwd_f32", _p(gout), _p(idx), B, N, m, ns, C, use_xyz, _p(gfeat), _stream(),
                      algo_bytes=B * (4 * m * ns * C + 4 * m * ns + 4 * N * C))
        return None, None, gfeat, None, None


def group_points(xyz, new_xyz, feature, idx, use_xyz=True):
    """[B,m,ns,(3)+C] = concat(xyz[idx]-new_xyz, feature[idx]).  misc/ops.py:383-407."""
    if not use_xyz and feature is None:
        raise ValueError("use_xyz=False needs features")
    return _GroupPoints.apply(xyz, new_xyz, feature, idx, bool(use_xyz))


_GROUP_ALL_BWD_VIEW = __import__("os").environ.get("PCL_GROUP_ALL_BWD_VIEW", "1") != "0"      # lab switch (A/B on one box): 0 = the copy kernel


class _GroupAll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, feat, use_xyz):
        xyz = _dev(xyz, "xyz")
        feat = _dev(feat, "feature")
        B, N, _ = xyz.shape
        C = 0 if feat is None else feat.shape[2]
        D = (3 if use_xyz else 0) + C
        out = torch.empty((B, 1, N, D), dtype=torch.float32, device=xyz.device)
        _lib.call("pcl_group_all_f32", _p(xyz), _p(feat), B, N, C, int(use_xyz), _p(out), _stream())
        ctx.dims = (B, N, C, int(use_xyz))
        return out

    @staticmethod
    def backward(ctx, gout):
        B, N, C, use_xyz = ctx.dims
        gfeat = None
        if C > 0 and ctx.needs_input_grad[1]:
            D = (3 if use_xyz else 0) + C
            if _GROUP_ALL_BWD_VIEW and gout.is_contiguous() and gout.is_cuda and gout.dtype == torch.float32:
                # the feature columns of the gradient AS A VIEW (row stride D): the stack below reads its gout in place through gout_ld
                # (csrc/stack.hip), any other consumer makes it dense itself -- no copy launch here (round 6)
                return None, gout.view(B, N, D)[:, :, D - C:], None
            gout = _dev(gout, "grad")
            gfeat = torch.empty((B, N, C), dtype=torch.float32, device=gout.device)
            _lib.call("pcl_group_all_bwd_f32", _p(gout), B, N, C, use_xyz, _p(gfeat), _stream())
        return None, gfeat, None


class RowSet:
    """Metadata of duplicate-compacted grouped rows (see include/pcl_hip.h, 'ragged groups')."""

    def __init__(self, B, m, ns, row_meta, row_src, group_off):
        self.B, self.m, self.ns = B, m, ns
        self.G = B * m
        self.row_meta, self.row_src, self.group_off = row_meta, row_src, group_off
        self.n_rows_dev = group_off[self.G:]            # 1-element view: the valid-row count stays on the device

    @property
    def capacity(self):
        return self.G * self.ns


def group_offsets(cnt):
    """cnt int32 [B,m] (ball-query hit counts) -> group_off int32 [B*m+1]: exclusive scan of max(cnt,1); the last entry
    is the number of distinct rows.  Depends on the indices only, so it can be produced with them (side stream)."""
    cnt = _dev(cnt, "cnt", torch.int32)
    G = cnt.numel()
    group_off = torch.empty((G + 1,), dtype=torch.int32, device=cnt.device)
    _lib.call("pcl_group_offsets_i32", _p(cnt), G, _p(group_off), _stream())
    return group_off


def group_offsets_multi(cnts):
    """``group_offsets`` of up to four count arrays of one size in one launch (the scales of a multi-scale level)."""
    import ctypes
    cnts = [_dev(c, "cnt", torch.int32) for c in cnts]
    n, G = len(cnts), cnts[0].numel()
    if not 1 <= n <= BALL_QUERY_MULTI_MAX or any(c.numel() != G for c in cnts):
        raise ValueError("group_offsets_multi: 1..4 count arrays of equal size")
    offs = [torch.empty((G + 1,), dtype=torch.int32, device=cnts[0].device) for _ in range(n)]
    c_c = (ctypes.c_void_p * n)(*[t.data_ptr() for t in cnts])
    c_o = (ctypes.c_void_p * n)(*[t.data_ptr() for t in offs])
    _lib.call("pcl_group_offsets_multi_i32", n, c_c, G, c_o, _stream())
    return offs


class _GroupCompact(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, new_xyz, feat, idx, cnt, group_off, use_xyz, pad_to):
        idx = _dev(idx, "idx", torch.int32)
        cnt = _dev(cnt, "cnt", torch.int32)
        group_off = _dev(group_off, "group_off", torch.int32)
        B, m, ns = idx.shape
        xyz = _dev(xyz, "xyz")
        new_xyz = _dev(new_xyz, "new_xyz")
        feat = _dev(feat, "feature")
        N = xyz.shape[1]
        C = 0 if feat is None else feat.shape[2]
        D = (3 if use_xyz else 0) + C
        S = (D + pad_to - 1) // pad_to * pad_to            # row stride: zero columns up to a multiple of pad_to
        cap = B * m * ns
        dev = idx.device
        rows = torch.empty((cap, S), dtype=torch.float32, device=dev)
        row_meta = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        row_src = torch.empty((cap,), dtype=torch.int32, device=dev)
        _lib.call("pcl_group_compact_f32", _p(xyz), _p(new_xyz), _p(feat), _p(idx), _p(cnt), _p(group_off), B, N, m, ns, C,
                  int(use_xyz), S, _p(rows), _p(row_meta), _p(row_src), _stream())
        ctx.dims = (B, N, C, S, int(use_xyz), m, ns)
        ctx.mark_non_differentiable(row_meta, row_src)
        ctx.save_for_backward(row_src, group_off)        # saved properly, never as ctx attributes (no cycles)
        return rows, row_meta, row_src

    @staticmethod
    def backward(ctx, grows, *_):
        B, N, C, S, use_xyz, m, ns = ctx.dims
        gfeat = None
        if C > 0 and ctx.needs_input_grad[2]:
            row_src, group_off = ctx.saved_tensors
            grows = _dev(grows, "grad")
            gfeat = torch.empty((B, N, C), dtype=torch.float32, device=grows.device)
            _lib.call("pcl_scatter_rows_add_f32", _p(grows), _p(row_src), _p(group_off[B * m:]), B * m * ns, S,
                      3 if use_xyz else 0, C, B * N, _p(gfeat), _stream())
        return None, None, gfeat, None, None, None, None, None


def group_points_compact(xyz, new_xyz, feature, idx, cnt, use_xyz=True, group_off=None, pad_to=4):
    """Duplicate-compacted grouping: (rows [B*m*ns (capacity), S], RowSet).  Only the first ``group_off[-1]`` rows are
    valid: the DISTINCT points of every ball-query group in (group, slot) order, each with its multiplicity.  Rows are
    ``[xyz - centre | features]`` padded with zero columns to a multiple of ``pad_to`` (S >= 3+C) so that every consumer
    moves them as 16-byte pieces; ``PointwiseMLP`` pads its first weight matrix to match."""
    if group_off is None:
        group_off = group_offsets(cnt)
    rows, row_meta, row_src = _GroupCompact.apply(xyz, new_xyz, feature, idx, cnt, group_off, bool(use_xyz), int(pad_to))
    B, m, ns = idx.shape
    return rows, RowSet(B, m, ns, row_meta, row_src, group_off)


def group_all(xyz, feature, use_xyz=True):
    """[B,1,N,3+C] = concat(xyz, feature) (xyz not re-centred).  misc/ops.py:415-419."""
    return _GroupAll.apply(xyz, feature, bool(use_xyz))


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, idx):
        src = _dev(src, "points")
        idx = _dev(idx, "idx", torch.int32)
        B, N, C = src.shape
        M = idx.numel() // B
        out = torch.empty(tuple(idx.shape) + (C,), dtype=torch.float32, device=src.device)
        _lib.call("pcl_gather_rows_f32", _p(src), _p(idx), B, N, M, C, _p(out), _stream())
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, M, C)
        return out

    @staticmethod
    def backward(ctx, gout):
        (idx,) = ctx.saved_tensors
        B, N, M, C = ctx.dims
        gout = _dev(gout, "grad")
        gsrc = torch.empty((B, N, C), dtype=torch.float32, device=gout.device)
        _lib.call("pcl_gather_rows_bwd_f32", _p(gout), _p(idx), B, N, M, C, _p(gsrc), _stream())
        return gsrc, None


def index_points(points, idx):
    """points [B,N,C], idx [B,S] or [B,S,K] (int32) -> [B,S,(K,)C].  misc/ops.py:12-27."""
    return _GatherRows.apply(points, idx.to(torch.int32))


class _EdgeFeature(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx):
        x = _dev(x, "x")
        idx = _dev(idx, "idx", torch.int32)
        B, N, C = x.shape
        k = idx.shape[2]
        out = torch.empty((B, N, k, 2 * C), dtype=torch.float32, device=x.device)
        _lib.call("pcl_edge_feature_f32", _p(x), _p(idx), B, N, k, C, _p(out), _stream(),
                  algo_bytes=4 * B * N * (C + k + 2 * C * k))
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, k, C)
        return out

    @staticmethod
    def backward(ctx, gout):
        (idx,) = ctx.saved_tensors
        B, N, k, C = ctx.dims
        gout = _dev(gout, "grad")
        gx = torch.empty((B, N, C), dtype=torch.float32, device=gout.device)
        _lib.call("pcl_edge_feature_bwd_f32", _p(gout), _p(idx), B, N, k, C, _p(gx), _stream(),
                  algo_bytes=4 * B * N * (C + k + 2 * C * k))
        return gx, None


def edge_features(x, idx):
    """x [B,N,C] channel-last, idx [B,N,k] int32 -> [B,N,k,2C] = concat(x[idx]-x, x).  dgcnn.py:29-50."""
    return _EdgeFeature.apply(x, idx)


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points2, idx3, w3):
        points2 = _dev(points2, "points2")
        idx3 = _dev(idx3, "idx3", torch.int32)
        w3 = _dev(w3, "w3")
        B, S, D = points2.shape
        N = idx3.shape[1]
        out = torch.empty((B, N, D), dtype=torch.float32, device=points2.device)
        _lib.call("pcl_three_interp_f32", _p(points2), _p(idx3), _p(w3), B, N, S, D, _p(out), _stream())
        ctx.save_for_backward(idx3, w3)
        ctx.dims = (B, N, S, D)
        return out

    @staticmethod
    def backward(ctx, gout):
        idx3, w3 = ctx.saved_tensors
        B, N, S, D = ctx.dims
        gout = _dev(gout, "grad")
        g = torch.empty((B, S, D), dtype=torch.float32, device=gout.device)
        _lib.call("pcl_three_interp_bwd_f32", _p(gout), _p(idx3), _p(w3), B, N, S, D, _p(g), _stream())
        return g, None, None


def three_interpolate(points2, idx3, w3):
    """sum_j w3[b,n,j] * points2[b, idx3[b,n,j], :]  ->  [B,N,D].  misc/ops.py:93."""
    return _ThreeInterpolate.apply(points2, idx3, w3)


# ----------------------------------------------------------------------------- packed rows of a ragged batch (csrc/pack.hip)
def row_offsets(lengths, B, N, device, n_rows=None):
    """Per-cloud counts of a ragged batch -> (row_off int32 [B+1] on the device, R): the exclusive scan of the counts and their
    sum.  Packed row ``row_off[b] + i`` is point i of cloud b; R rows in all.  Host-side ``lengths`` (a
    sequence or a CPU tensor, validated as by ``_lengths``) give R as a host sum: no synchronisation.  A device tensor is not read
    back when the caller states ``n_rows``; that it equals the sum is then the caller's precondition (a wrong value loses rows,
    the kernels never leave the buffers).  A device tensor WITHOUT ``n_rows`` costs one ``.item()``: a host synchronisation."""
    if lengths is None:
        raise ValueError("row_offsets: lengths is None (a dense batch has no packed rows to offset)")
    on_device = isinstance(lengths, torch.Tensor) and lengths.is_cuda
    if not on_device and n_rows is None:
        host = lengths.detach() if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths)
    lengths = _lengths(lengths, B, N, device)
    if not lengths.is_cuda:
        raise RuntimeError(f"row_offsets: expected the GPU as device (libpcl_hip has no CPU path), got {lengths.device}")
    row_off = torch.empty((B + 1,), dtype=torch.int32, device=lengths.device)
    _lib.call("pcl_row_offsets_i32", _p(lengths), B, N, _p(row_off), _stream())
    if n_rows is None:
        n_rows = int(row_off[B].item()) if on_device else int(host.sum())
    return row_off, int(n_rows)


def _words(t, name):
    if t.dtype.itemsize not in (4, 8) or t.dtype.is_complex:
        raise TypeError(f"{name}: rows move as 32-bit words: a dtype of 4 or 8 bytes, got {t.dtype}")
    return t.dtype.itemsize // 4


def _move_rows(pack, src, lengths, row_off, N, R):
    """pack: src [B, N, ...] -> [R, ...];  unpack: src [R, ...] -> [B, N, ...] with zero pad rows."""
    if not src.is_cuda:
        raise RuntimeError(f"{'pack_rows' if pack else 'unpack_rows'}: expected a tensor on the GPU (libpcl_hip has no CPU path), got {src.device}")
    src = src.contiguous()
    B = lengths.shape[0]
    tail = tuple(src.shape[2:] if pack else src.shape[1:])
    W = _words(src, "rows") * int(math.prod(tail))
    if W == 0:
        raise ValueError("rows without columns")
    out = torch.empty(((R,) if pack else (B, N)) + tail, dtype=src.dtype, device=src.device)
    _lib.call("pcl_pack_rows_b32" if pack else "pcl_unpack_rows_b32", _p(src), _p(lengths), _p(row_off), B, N, W, W, 0, R, _p(out), _stream(),
              algo_bytes=8 * R * W)
    return out


class _PackRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, lengths, row_off, R):
        if t.dim() < 2 or t.shape[0] != lengths.shape[0]:
            raise ValueError(f"pack_rows: expected [B={lengths.shape[0]}, N, ...], got {tuple(t.shape)}")
        ctx.save_for_backward(lengths, row_off)
        ctx.dims = (t.shape[1], R)
        return _move_rows(True, t, lengths, row_off, t.shape[1], R)

    @staticmethod
    def backward(ctx, g):
        lengths, row_off = ctx.saved_tensors
        N, R = ctx.dims
        return _move_rows(False, g, lengths, row_off, N, R), None, None, None


class _UnpackRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, lengths, row_off, N):
        ctx.save_for_backward(lengths, row_off)
        ctx.dims = (N, rows.shape[0])
        return _move_rows(False, rows, lengths, row_off, N, rows.shape[0])

    @staticmethod
    def backward(ctx, g):
        lengths, row_off = ctx.saved_tensors
        N, R = ctx.dims
        return _move_rows(True, g, lengths, row_off, N, R), None, None, None


def _packed_args(lengths, row_off, B, N, device):
    lengths = _dev(_lengths(lengths, B, N, device), "lengths", torch.int32)
    row_off = _dev(row_off, "row_off", torch.int32)
    if row_off.dim() != 1 or row_off.shape[0] != B + 1:
        raise ValueError(f"row_off: expected shape [{B + 1}] (row_offsets), got {tuple(row_off.shape)}")
    return lengths, row_off


def pack_rows(t, lengths, row_off, R):
    """t [B, N, ...] -> [R, ...]: the valid rows of every cloud, cloud after cloud (``row_off``, R from ``row_offsets``).  Any dtype of
    4 or 8 bytes (features, logits, int64 labels); pad rows are never read.  Differentiable: the gradient is ``unpack_rows``."""
    if t.dim() < 2:
        raise ValueError(f"pack_rows: expected [B, N, ...], got {tuple(t.shape)}")
    lengths, row_off = _packed_args(lengths, row_off, t.shape[0], t.shape[1], t.device)
    return _PackRows.apply(t, lengths, row_off, int(R))


def unpack_rows(rows, lengths, row_off, N):
    """rows [R, ...] -> [B, N, ...] with every pad row zero bits; the inverse of ``pack_rows`` on the valid rows, and its gradient."""
    B = row_off.shape[0] - 1
    lengths, row_off = _packed_args(lengths, row_off, B, int(N), rows.device)
    return _UnpackRows.apply(rows, lengths, row_off, int(N))


class _InterpolatePack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points2, skip, onehot, idx3, w3, lengths, row_off, N, R):
        points2 = _dev(points2, "points2")
        skip, onehot = _dev(skip, "skip"), _dev(onehot, "onehot")
        idx3, w3 = _dev(idx3, "idx3", torch.int32), _dev(w3, "w3")
        B, S, D2 = points2.shape
        CS = 0 if skip is None else skip.shape[2]
        n1 = 0 if onehot is None else onehot.shape[1]
        rows = torch.empty((R, n1 + CS + D2), dtype=torch.float32, device=points2.device)
        _lib.call("pcl_fp_pack_rows_f32", _p(onehot), n1, _p(skip), CS, _p(points2), _p(idx3), _p(w3), _p(lengths), _p(row_off), B, N, S, D2,
                  R, _p(rows), _stream(), algo_bytes=4 * R * (n1 + 2 * CS + D2 + 6) + 4 * B * S * D2)
        ctx.save_for_backward(idx3, w3, lengths, row_off)
        ctx.dims = (B, N, S, D2, CS, n1, R)
        return rows

    @staticmethod
    def backward(ctx, grows):
        idx3, w3, lengths, row_off = ctx.saved_tensors
        B, N, S, D2, CS, n1, R = ctx.dims
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 9
        grows = _dev(grows, "grad")
        gskip = torch.empty((B, N, CS), dtype=torch.float32, device=grows.device) if ctx.needs_input_grad[1] else None
        if not ctx.needs_input_grad[0]:           # the skip alone: the column window of the gradient, pad rows zero
            _lib.call("pcl_unpack_rows_b32", _p(grows), _p(lengths), _p(row_off), B, N, CS, n1 + CS + D2, n1, R, _p(gskip), _stream())
            return None, gskip, None, None, None, None, None, None, None
        g2 = torch.empty((B, S, D2), dtype=torch.float32, device=grows.device)
        _lib.call("pcl_fp_pack_rows_bwd_f32", _p(grows), n1, CS, _p(idx3), _p(w3), _p(lengths), _p(row_off), B, N, S, D2, R, _p(g2),
                  _p(gskip), _stream(), algo_bytes=4 * R * (4 * D2 + 6 + 2 * CS))
        return g2, gskip, None, None, None, None, None, None, None


def interpolate_pack(points2, idx3, w3, lengths, row_off, n_rows, N, skip=None, onehot=None):
    """Feature propagation's "interpolate, concatenate" written straight as the packed rows of a ragged batch, one launch:
    ``[n_rows, n_onehot + CS + D2]``, row ``row_off[b] + i`` = ``[onehot[b] | skip[b, i] | sum_k w3[b,i,k] points2[b, idx3[b,i,k]]]`` for
    ``i < lengths[b]`` -- bit for bit ``three_interpolate`` + ``cat`` on the cloud's own rows.  points2 [B,S,D2]; idx3 / w3 [B,N,3] from
    ``three_nn(lengths1=lengths)`` (None when S == 1: the one source row is broadcast); skip [B,N,CS] and onehot [B,n_onehot] optional.
    Gradients reach points2 (fp32 atomic adds like ``three_interpolate``'s; S == 1: a fixed-order sum) and skip (zero on pad rows);
    the one-hot block is a label and gets none."""
    if points2.dim() != 3:
        raise ValueError(f"points2 must be [B,S,D2], got {tuple(points2.shape)}")
    B, S, _ = points2.shape
    if onehot is not None and onehot.requires_grad:
        raise ValueError("interpolate_pack: onehot is a per-cloud label block and gets no gradient")
    if (idx3 is None or w3 is None) and S != 1:
        raise ValueError(f"interpolate_pack: idx3 / w3 may be None only for S == 1, S = {S}")
    for name, t, shape in (("idx3", idx3, (B, N, 3)), ("w3", w3, (B, N, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected {list(shape)}, got {tuple(t.shape)}")
    if skip is not None and (skip.dim() != 3 or tuple(skip.shape[:2]) != (B, N)):
        raise ValueError(f"skip: expected [{B},{N},CS], got {tuple(skip.shape)}")
    if onehot is not None and (onehot.dim() != 2 or onehot.shape[0] != B):
        raise ValueError(f"onehot: expected [{B},n_onehot], got {tuple(onehot.shape)}")
    lengths, row_off = _packed_args(lengths, row_off, B, int(N), points2.device)
    if S == 1:
        idx3 = w3 = None
    return _InterpolatePack.apply(points2, skip, onehot, idx3, w3, lengths, row_off, int(N), int(n_rows))


# ----------------------------------------------------------------------------- pooling over the clouds of packed rows (csrc/segpool.hip)
def row_cloud(row_off, B, R):
    """row_off int32 [B+1] (``row_offsets``) -> int32 [R]: the cloud that owns each packed row.  Made once per batch; the pooling
    backward and ``broadcast_rows`` read it."""
    row_off = _dev(row_off, "row_off", torch.int32)
    if row_off.dim() != 1 or row_off.shape[0] != B + 1:
        raise ValueError(f"row_off: expected shape [{B + 1}] (row_offsets), got {tuple(row_off.shape)}")
    out = torch.empty((int(R),), dtype=torch.int32, device=row_off.device)
    _lib.call("pcl_row_cloud_i32", _p(row_off), int(B), int(R), _p(out), _stream())
    return out


def packed_layout(lengths, B, N, device, n_rows=None):
    """Everything the packed form of a batch [B, N, .] needs, made once: (lengths int32 [B] on the device, row_off int32 [B+1], R,
    row_cloud int32 [R]).  ``lengths`` as for ``row_offsets`` (host sequences are validated and give R without a synchronisation; a
    device tensor wants ``n_rows`` or costs one ``.item()``); None = a dense batch, every cloud N rows."""
    if lengths is None:
        lengths, n_rows = torch.full((B,), N, dtype=torch.int32, device=device), B * N
    elif isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        lengths = _lengths(lengths, B, N, device)
    else:
        given = lengths
        lengths = _lengths(given, B, N, device)                      # validated on the host (its errors come first), copied once
        if n_rows is None:
            n_rows = int((given.detach() if isinstance(given, torch.Tensor) else torch.as_tensor(given)).sum())
    row_off, R = row_offsets(lengths, B, N, device, n_rows=n_rows)
    return lengths, row_off, R, row_cloud(row_off, B, R)


class _SegmentMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Y, row_off, row_cloud, B, scale, shift, slope, link):
        Y = _dev(Y, "Y")
        if Y.dim() != 2:
            raise ValueError(f"segment_max: expected packed rows [R, C], got {tuple(Y.shape)}")
        R, C = Y.shape
        out = torch.empty((B, C), dtype=torch.float32, device=Y.device)
        arg = torch.empty((B, C), dtype=torch.int32, device=Y.device)
        _lib.call("pcl_bn_act_seg_max_f32", _p(Y), _p(row_off), _p(scale), _p(shift), float(slope), B, C, R, _p(out), _p(arg), _stream(),
                  algo_bytes=4 * R * C)
        ctx.link, ctx.slope, ctx.B = link, float(slope), B
        ctx.save_for_backward(Y, arg, scale, shift, row_off, row_cloud)
        return out

    @staticmethod
    def backward(ctx, gout):
        import ctypes
        Y, arg, scale, shift, row_off, row_cloud = ctx.saved_tensors
        R, C = Y.shape
        if gout.is_cuda and gout.dtype == torch.float32 and gout.stride(1) == 1 and C <= gout.stride(0) < 2 ** 31:
            ldg = gout.stride(0)                                       # a column slice of a wider gradient is read in place
        else:
            gout, ldg = _dev(gout, "grad"), C
        du = torch.empty_like(Y)
        stats = torch.empty((1024, 2, C), dtype=torch.float64, device=Y.device)
        rows = ctypes.c_int(0)
        _lib.call("pcl_bn_act_seg_max_bwd_f32", _p(gout), ldg, _p(arg), _p(Y), _p(scale), _p(shift), ctx.slope, _p(row_off), _p(row_cloud),
                  ctx.B, C, R, _p(du), _p(stats), ctypes.byref(rows), _stream(), algo_bytes=8 * R * C)
        if ctx.link is not None:
            ctx.link.stats, ctx.link.rows = stats, rows.value
        return du, None, None, None, None, None, None, None


def segment_max(Y, row_off, row_cloud, B, scale=None, shift=None, slope=1.0, link=None):
    """Max over each cloud's packed rows: Y [R, C] -> [B, C], ``out[b] = max_r lrelu(scale * Y[r] + shift, slope)`` over the rows
    ``row_off[b] .. row_off[b+1] - 1`` (csrc/segpool.hip).  Two forms, as ``edgeconv.conv_max_mean_pool``:
    ``link`` = the ``DeferLink`` of ``mlp_hip.stack_plain_deferred``: Y is that stack's PRE-BatchNorm output, scale / shift / slope
    are the link's, and the backward hands the stack du and its BatchNorm-backward sums through the link;
    otherwise Y is pooled as it is (scale 1, shift 0, slope 1 unless given: ``fmaf(1, y, 0)`` is exact, a plain segmented max) and
    the gradient w.r.t. Y is the winner's, scale / shift being constants.  ``mlp_segment_max`` chooses between them."""
    if link is not None:
        scale, shift, slope = link.scale, link.shift, link.slope
    elif scale is None or shift is None:
        if scale is not None or shift is not None:
            raise ValueError("segment_max: scale and shift come together")
        from .mlp_hip import _unit_consts
        scale, shift = _unit_consts(Y.device, Y.shape[-1])
    if not 1 <= B <= 65535 or row_off.shape[0] != B + 1:
        raise ValueError(f"segment_max: B={B} (1 .. 65535) with row_off {tuple(row_off.shape)}")
    if row_cloud.shape[0] != Y.shape[0]:
        raise ValueError(f"segment_max: row_cloud holds {row_cloud.shape[0]} rows, Y {Y.shape[0]}")
    return _SegmentMax.apply(Y, _dev(row_off, "row_off", torch.int32), _dev(row_cloud, "row_cloud", torch.int32), int(B),
                             _dev(scale, "scale"), _dev(shift, "shift"), float(slope), link)


def mlp_segment_max(mlp, rows, row_off, row_cloud, B):
    """``segment_max(mlp(rows))`` for a ``PointwiseMLP`` on packed rows [R, C0] -> [B, CL].  Training on the per-stack path: the
    stack stops at its last pre-BatchNorm output and the pooling applies BatchNorm + activation while it reduces, so the activated
    [R, CL] tensor is never written.  Otherwise (evaluation, synchronised BatchNorm, the per-kernel path): ``mlp(rows)``, pooled."""
    from . import mlp_hip
    if rows.is_cuda and rows.dtype == torch.float32 and mlp.resolved_backend(rows) == "hip" and mlp.last_act:
        r = mlp_hip.stack_plain_deferred(mlp, rows.contiguous())
        if r is not None:
            return segment_max(r[0], row_off, row_cloud, B, link=r[1])
    return segment_max(mlp(rows), row_off, row_cloud, B)


class _BroadcastRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, row_off, row_cloud, R):
        v = _dev(v, "v")
        B, C = v.shape
        out = torch.empty((R, C), dtype=torch.float32, device=v.device)
        _lib.call("pcl_seg_broadcast_rows_f32", _p(v), _p(row_cloud), B, C, R, _p(out), _stream(), algo_bytes=4 * R * C)
        ctx.save_for_backward(row_off)
        ctx.dims = (B, C, R)
        return out

    @staticmethod
    def backward(ctx, g):
        row_off, = ctx.saved_tensors
        B, C, R = ctx.dims
        g = _dev(g, "grad")
        gv = torch.empty((B, C), dtype=torch.float32, device=g.device)
        _lib.call("pcl_seg_sum_rows_f32", _p(g), _p(row_off), B, C, R, _p(gv), _stream(), algo_bytes=4 * R * C)
        return gv, None, None, None


def broadcast_rows(v, row_off, row_cloud, R):
    """A per-cloud vector onto the cloud's packed rows: v [B, C] -> [R, C], row r = ``v[row_cloud[r]]``.  The gradient is the
    per-cloud column sum (fp64, a fixed order: run-to-run identical)."""
    if v.dim() != 2 or not 1 <= v.shape[0] <= 65535 or row_off.shape[0] != v.shape[0] + 1:
        raise ValueError(f"broadcast_rows: expected v [B, C] with row_off [B+1], got {tuple(v.shape)} and {tuple(row_off.shape)}")
    if row_cloud.shape[0] != int(R):
        raise ValueError(f"broadcast_rows: row_cloud holds {row_cloud.shape[0]} rows, R = {R}")
    return _BroadcastRows.apply(v, _dev(row_off, "row_off", torch.int32), _dev(row_cloud, "row_cloud", torch.int32), int(R))


# ----------------------------------------------------------------------------- modules (reference names)
class _Module(nn.Module):
    def execute(self, *a, **k):   # Jittor's name for forward
        return self(*a, **k)


class FurthestPointSampler(_Module):
    """misc/ops.py:114-286: ``FurthestPointSampler(n_samples)(x[B,N,3]) -> [B,n_samples,3]``."""

    def __init__(self, n_samples, tie_stride=None):
        super().__init__()
        self.n_samples = n_samples
        self.tie_stride = tie_stride

    def forward(self, x, return_idx=False, lengths=None):
        idx, y = furthest_point_sample(x, self.n_samples, self.tie_stride, lengths=lengths)
        return (y, idx) if return_idx else y


class BallQueryGrouper(_Module):
    """misc/ops.py:289-407: ``(new_xyz[B,m,3], pointset[B,N,3], feature[B,N,C]|None) -> [B,m,ns,3+C]``."""

    def __init__(self, radius, n_samples, use_xyz):
        super().__init__()
        self.radius = radius
        self.n_samples = n_samples
        self.use_xyz = use_xyz

    def forward(self, new_xyz, pointset, feature, return_idx=False, lengths=None):
        idx = ball_query(new_xyz, pointset, self.radius, self.n_samples, lengths=lengths)
        if self.use_xyz or feature is not None:
            out = group_points(pointset, new_xyz, feature, idx, self.use_xyz)
        else:
            out = None   # misc/ops.py:405: use_xyz=False and feature=None returns None
        return (out, idx) if return_idx else out


class GroupAll(_Module):
    """misc/ops.py:410-419 (``use_xyz=False`` is a latent NameError upstream; here it returns features only)."""

    def __init__(self, use_xyz):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, new_xyz, pointset, feature):
        return group_all(pointset, feature, self.use_xyz)


class KNN(_Module):
    """misc/ops.py:422-663: ``KNN(k)(x_q[B,C,Nq], x_r[B,C,Nr]) -> int32 [B,k,Nq]``."""

    def __init__(self, k):
        super().__init__()
        self.k = k

    def forward(self, x_q, x_r):
        return knn_indices(x_q, x_r, self.k)


class PointNetFeaturePropagation(_Module):
    """misc/ops.py:54-107.  ``(xyz1[B,N,3], xyz2[B,S,3], points1[B,N,D1]|None, points2[B,S,D2]) -> [B,N,mlp[-1]]``.

    3-NN inverse-distance interpolation (HIP three_nn + three_interpolate instead of the reference's
    dense matrix + full argsort), concat, then Conv1d(k=1, bias)+BatchNorm1d+ReLU per ``mlp`` entry."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        from .layers import PointwiseMLP
        self.mlp = PointwiseMLP([in_channel] + list(mlp), bias=True)

    def forward(self, xyz1, xyz2, points1, points2):
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        if S == 1:
            interpolated = points2.expand(B, N, points2.shape[2])          # :83-84
        else:
            idx, w = three_nn(xyz1, xyz2)
            interpolated = three_interpolate(points2, idx, w)              # :86-93
        new_points = torch.cat([points1, interpolated], dim=-1) if points1 is not None else interpolated
        return self.mlp(new_points.contiguous())

    def forward_packed(self, xyz1, xyz2, points1, points2, lengths, row_off, n_rows, onehot=None):
        """The same level on a ragged batch whose TARGETS have ``lengths[b]`` valid rows (sources dense), as packed rows:
        -> [n_rows, mlp[-1]], row ``row_off[b] + i`` = target i of cloud b (``row_offsets``).  The MLP's input is built directly as
        ``[n_rows, n_onehot + D1 + D2]`` rows (``interpolate_pack``; ``onehot`` [B, n_onehot]: a per-cloud block in front of points1 that
        is never expanded to [B, N, n_onehot]), so its training-mode BatchNorm takes its statistics over the valid points alone and
        no pad row of xyz1 / points1 is read.  When points1 needs no gradient the MLP's input gradient is produced from the first
        interpolated column on (``x_grad_from``)."""
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        lengths = _lengths(lengths, B, N, xyz1.device)
        idx = w = None
        if S > 1:
            idx, w = three_nn(xyz1, xyz2, lengths1=lengths)
        rows = interpolate_pack(points2, idx, w, lengths, row_off, n_rows, N, skip=points1, onehot=onehot)
        skip_grad = points1 is not None and points1.requires_grad and torch.is_grad_enabled()
        return self.mlp(rows, x_grad_from=0 if skip_grad else rows.shape[1] - points2.shape[2])
