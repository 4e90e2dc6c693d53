"""The yardsticks of the op-level EdgeConv tests (csrc/edgeconv.hip, misc/edgeconv.py).  TEST INFRASTRUCTURE, no test of its own;
NumPy only (``edge_tensor_stage`` also takes PyTorch modules, on whatever device they live), needs no GPU.

* ``gather_ref``      the gather kernel restated in ``np.float32`` in the kernel's own operation order.  The library is built with
                      -ffp-contract=off, so max / min / positions / sumU are reproduced BIT FOR BIT; the BatchNorm sums are fp64 sums
                      whose order within a block of 32 points is the atomics' (compare within 1e-12 of ``stats_scale``).
* ``transpose_ref``   the transposed neighbour lists by a stable sort of the edges by end point.
* ``scatter_ref``     the per-edge definition of the backward (include/pcl_hip.h), in fp64 (the truth) or fp32 (the yardstick).
* ``wcat_ref``        W = [Wa | Wb] <-> Wcat = [Wa ; Wb - Wa] in fp32.
* ``knn_like`` / ``hubs`` / ``with_duplicates``: neighbour lists with the properties the kernels' branches depend on.
* ``edge_tensor_stage``: the stage as the reference network writes it (edge tensor -> conv -> BatchNorm -> LeakyReLU -> max), on a
                      double-precision copy of the stage's module: output and every gradient.

tests/test_edgeconv_ref_cpu.py holds these to brute force and to ``torch.autograd``.
"""
import numpy as np

PB = 32          # points per workgroup of the gather kernel == points per BatchNorm partial row (csrc/edgeconv.hip: EC_PB)


def _flat_idx(idx, B, N, k):
    idx = np.asarray(idx).reshape(B * N, k).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < N
    return idx


def gather_ref(UV, UVlo, idx, B, N, k, C):
    """UV [B*N, 2C] (U | V) float32, UVlo the same shape or None, idx [B,N,k] -> dict of
    ``ymax``, ``ymin`` [B*N,C] float32, ``jmax``, ``jmin`` [B*N,C] int32 (first position attaining them), ``sumU`` [B*N,C] float32
    (left-to-right fp32 sum of U[nbr]), ``stats`` [rows,2,C] float64 (sum y, sum y*y over the 32 consecutive points of row r, all their
    neighbours) in logical block order and ``stats_scale`` [rows,2,C] (sum |y|, sum y*y), what the rows' rounding is relative to."""
    UV = np.asarray(UV)
    assert UV.dtype == np.float32 and UV.shape == (B * N, 2 * C)
    if UVlo is not None:
        UVlo = np.asarray(UVlo)
        assert UVlo.dtype == np.float32 and UVlo.shape == UV.shape
    idx = _flat_idx(idx, B, N, k)
    P = B * N
    base = (np.arange(P) // N) * N
    U, V = UV[:, :C], UV[:, C:]
    vmax = np.full((P, C), -np.inf, np.float32)
    vmin = np.full((P, C), np.inf, np.float32)
    jmax, jmin = np.zeros((P, C), np.int32), np.zeros((P, C), np.int32)
    su = np.zeros((P, C), np.float32)
    s, q, sa = (np.zeros((P, C), np.float64) for _ in range(3))
    for j in range(k):
        nb = base + idx[:, j]
        u = U[nb]
        y = u + V                                            # one fp32 addition
        if UVlo is not None:
            y = y + (UVlo[nb, :C] + UVlo[:, C:])             # two more: (Ulo + Vlo), then onto y
        assert y.dtype == np.float32
        su = su + u
        y64 = y.astype(np.float64)
        s += y64; q += y64 * y64; sa += np.abs(y64)          # (y*y is exact in fp64: 24 x 24 bits)
        m = y > vmax                                         # strict: the first position wins a tie
        vmax[m] = y[m]; jmax[m] = j
        m = y < vmin
        vmin[m] = y[m]; jmin[m] = j
    rows = (P + PB - 1) // PB

    def by_row(a):
        pad = np.zeros((rows * PB, C), np.float64)
        pad[:P] = a
        return pad.reshape(rows, PB, C).sum(1)

    stats = np.stack([by_row(s), by_row(q)], axis=1)
    scale = np.stack([by_row(sa), by_row(q)], axis=1)
    return {"ymax": vmax, "ymin": vmin, "jmax": jmax, "jmin": jmin, "sumU": su, "stats": stats, "stats_scale": scale}


def transpose_ref(idx, B, N, k):
    """idx [B,N,k] -> (in_off [B*N+1] int32: global offsets into in_src, in_src [B*N*k] int32: for every point n of a cloud the sources i
    (index within the cloud) of the edges i -> n, ascending; a row that names n twice is listed twice)."""
    idx = _flat_idx(idx, B, N, k).reshape(B, N * k)
    E = N * k
    in_off = np.zeros(B * N + 1, np.int64)
    in_src = np.empty(B * E, np.int32)
    for b in range(B):
        order = np.argsort(idx[b], kind="stable")            # edges e = i*k + j by end point; equal end points keep the edge order
        in_src[b * E:(b + 1) * E] = order // k
        in_off[b * N + 1:(b + 1) * N + 1] = b * E + np.cumsum(np.bincount(idx[b], minlength=N))
    return in_off.astype(np.int32), in_src


def scatter_ref(UV, idx, gz, arg, a, k1, k2, mu, B, N, k, C, dtype):
    """The per-edge definition: d(i,j) = [j == arg[i]] a gz[i] - k1 - k2 (U[nbr(i,j)] + V[i] - mu) per channel;
    dV[i] = sum_j d(i,j), dU[n] = sum over the edges (i,j) that end in n.  Every operand is converted to ``dtype`` first and every
    operation is one of ``dtype``: np.float64 is the truth, np.float32 the yardstick (sums in edge order).  -> dUV [B*N, 2C] (dU | dV)."""
    UV, gz, a, k1, k2, mu = (np.asarray(t).astype(dtype) for t in (UV, gz, a, k1, k2, mu))
    arg = np.asarray(arg).reshape(B * N, C)
    idx = _flat_idx(idx, B, N, k)
    P = B * N
    base = (np.arange(P) // N) * N
    U, V = UV[:, :C], UV[:, C:]
    g = a * gz.reshape(P, C)
    zero = np.zeros((), dtype)
    dU, dV = np.zeros((P, C), dtype), np.zeros((P, C), dtype)
    for j in range(k):
        nb = base + idx[:, j]
        y = U[nb] + V
        d = np.where(arg == j, g, zero) - k1 - k2 * (y - mu)
        assert d.dtype == dtype
        dV += d
        np.add.at(dU, nb, d)
    return np.concatenate([dU, dV], axis=1)


def wcat_ref(W, back):
    """back = False: W = [Wa | Wb] [Co, 2C] -> Wcat = [Wa ; Wb - Wa] [2Co, C];  back = True: dWcat [2Co, C] -> dW = [top - bottom | bottom]
    [Co, 2C].  float32 in, float32 out, one subtraction per element."""
    W = np.asarray(W)
    assert W.dtype == np.float32 and W.ndim == 2
    if not back:
        C = W.shape[1] // 2
        return np.concatenate([W[:, :C], W[:, C:] - W[:, :C]], axis=0)
    Co = W.shape[0] // 2
    return np.concatenate([W[:Co] - W[Co:], W[Co:]], axis=1)


# ---- neighbour lists ---------------------------------------------------------------------------------------------------------------------

def _distinct_rows(rng, rows, pool, m):
    """[rows, m] int64: every row m distinct values of range(pool), uniformly."""
    if m == 0:
        return np.zeros((rows, 0), np.int64)
    assert m <= pool
    if rows * pool <= 1 << 23:
        return np.argsort(rng.random((rows, pool)), axis=1)[:, :m]
    out = rng.integers(0, pool, size=(rows, m))               # few of many: draw, and draw again the rows in which two agree
    for _ in range(64):
        srt = np.sort(out, axis=1)
        bad = np.nonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))[0]
        if bad.size == 0:
            return out
        out[bad] = rng.integers(0, pool, size=(bad.size, m))
    for r in bad:
        out[r] = rng.permutation(pool)[:m]
    return out


def knn_like(B, N, k, seed):
    """[B,N,k] int32 as a k-NN search returns it: row i names i itself at position 0, then k-1 other points, all distinct."""
    assert 1 <= k <= N
    rng = np.random.default_rng(seed)
    idx = np.empty((B, N, k), np.int64)
    me = np.arange(N)
    for b in range(B):
        off = _distinct_rows(rng, N, N - 1, k - 1) + 1        # distinct offsets 1 .. N-1 round the cloud
        idx[b, :, 0] = me
        idx[b, :, 1:] = (me[:, None] + off) % N
    return idx.astype(np.int32)


def hubs(B, N, k, n_hubs, seed):
    """[B,N,k] int32: EVERY row names the points 0 .. n_hubs-1 (in-degree N, as the hubs of a feature-space k-NN graph have), its other
    k - n_hubs entries are distinct points of n_hubs .. N - N//8 - 1, so the last ``N // 8`` points of every cloud have in-degree 0.
    The positions within a row are shuffled."""
    n_orphans = N // 8
    pool = N - n_hubs - n_orphans
    assert 0 < n_hubs <= k and k - n_hubs <= pool and n_orphans >= 1
    rng = np.random.default_rng(seed)
    idx = np.empty((B, N, k), np.int64)
    for b in range(B):
        idx[b, :, :n_hubs] = np.arange(n_hubs)
        idx[b, :, n_hubs:] = n_hubs + _distinct_rows(rng, N, pool, k - n_hubs)
        sh = np.argsort(rng.random((N, k)), axis=1)
        idx[b] = np.take_along_axis(idx[b], sh, axis=1)
    return idx.astype(np.int32)


def with_duplicates(B, N, k, seed):
    """``knn_like`` in which every third row names one of its points twice (at two positions drawn per row)."""
    assert k >= 2
    idx = knn_like(B, N, k, seed)
    rng = np.random.default_rng(seed + 1)
    for b in range(B):
        for i in range(b % 3, N, 3):
            j1, j2 = rng.permutation(k)[:2]
            idx[b, i, j2] = idx[b, i, j1]
    return idx


# ---- the stage as the reference network writes it -------------------------------------------------------------------------------------

def edge_tensor_stage(ref_mlp, x, idx, g):
    """``ref_mlp``: a double-precision copy of the stage's ``PointwiseMLP`` with ``backend = "torch"`` (oracle/torch_backend.py), in
    training or evaluation mode; x [B,N,C], idx [B,N,k], g [B,N,Cout] the gradient fed to the output.  Builds e[i,j] = [x_nbr - x_i, x_i],
    runs conv -> BatchNorm -> LeakyReLU -> max over k in fp64 and its autograd backward (networks/cls/dgcnn.py:29-50, :100-102).
    -> {"out", "dx", <parameter name>: gradient ...} (the module's running statistics move as a training forward moves them)."""
    import torch
    B, k = x.shape[0], idx.shape[2]
    xb = x.detach().double().clone().requires_grad_(True)
    nb = xb[torch.arange(B, device=x.device)[:, None, None], idx.long()]
    e = torch.cat([nb - xb[:, :, None, :], xb[:, :, None, :].expand_as(nb)], -1)
    want = ref_mlp(e, group_max=k)
    want.backward(g.double())
    return {"out": want.detach(), "dx": xb.grad, **{n: p.grad for n, p in ref_mlp.named_parameters()}}
