"""CPU: the yardsticks of the op-level EdgeConv tests (tests/edgeconv_ref.py) are right -- the transposed lists against a brute-force
double loop, the per-edge backward in fp64 against ``torch.autograd`` on the edge-tensor formulation, the gather's max / min / positions
against ``np.max`` / ``np.argmax`` of the fp32 edge values (with constructed ties), its BatchNorm rows against the fp64 sums."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edgeconv_ref as R


# ---- neighbour-list builders ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,k", [(2, 17, 5), (1, 16, 16), (1, 9, 1), (1, 5000, 3)])
def test_knn_like_rows_are_distinct_with_self_first(B, N, k):
    idx = R.knn_like(B, N, k, 3)
    assert idx.shape == (B, N, k) and idx.dtype == np.int32
    assert (idx[:, :, 0] == np.arange(N)).all()
    srt = np.sort(idx, axis=2)
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all() and srt.min() >= 0 and srt.max() < N


def test_hubs_have_in_degree_n_and_orphans_none():
    B, N, k, h = 2, 40, 7, 2
    idx = R.hubs(B, N, k, h, 5)
    srt = np.sort(idx, axis=2)
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all()
    for b in range(B):
        deg = np.bincount(idx[b].ravel(), minlength=N)
        assert (deg[:h] == N).all() and (deg[N - N // 8:] == 0).all() and deg.sum() == N * k
    assert len({int(np.nonzero(idx[0, i] == 0)[0][0]) for i in range(N)}) > 1          # the hub sits at different positions


def test_with_duplicates_names_a_point_twice_in_some_rows():
    idx = R.with_duplicates(3, 16, 4, 7)
    srt = np.sort(idx, axis=2)
    dup = (srt[:, :, 1:] == srt[:, :, :-1]).any(axis=2)
    assert dup.any() and not dup.all()


# ---- transposed lists ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [lambda: (R.knn_like(2, 17, 5, 1), 2, 17, 5), lambda: (R.knn_like(1, 6, 6, 2), 1, 6, 6),
                                  lambda: (R.hubs(2, 24, 6, 2, 3), 2, 24, 6), lambda: (R.with_duplicates(3, 16, 4, 4), 3, 16, 4)],
                         ids=["knn", "k=N", "hubs", "duplicates"])
def test_transpose_ref_is_the_brute_force_list(make):
    idx, B, N, k = make()
    off, src = R.transpose_ref(idx, B, N, k)
    assert off.shape == (B * N + 1,) and src.shape == (B * N * k,) and off[0] == 0 and off[-1] == B * N * k
    for b in range(B):
        for n in range(N):
            want = [i for i in range(N) for j in range(k) if idx[b, i, j] == n]          # ascending sources, duplicates kept
            assert src[off[b * N + n]:off[b * N + n + 1]].tolist() == want, (b, n)


# ---- the per-edge backward ---------------------------------------------------------------------------------------------------------------

def _stage_fp64(UV, idx, gamma, beta, gout, B, N, k, C, eps, slope, running):
    """torch.autograd in fp64 on U[nbr] + V -> BatchNorm -> LeakyReLU(slope) -> max over k.  -> dUV, and what the forward hands the backward
    kernels: (gz, arg, a, k1, k2, mu) built as pcl_maxgrad_prep_f32 / pcl_bn_bwd_consts_f32 document them."""
    P = B * N
    UVt = torch.from_numpy(UV).requires_grad_(True)
    it = torch.from_numpy(idx.astype(np.int64))
    U, V = UVt[:, :C].view(B, N, C), UVt[:, C:].view(B, N, C)
    y = U[torch.arange(B)[:, None, None], it] + V[:, :, None, :]                          # [B,N,k,C]
    g_t, b_t = torch.from_numpy(gamma), torch.from_numpy(beta)
    if running is None:
        u = F.batch_norm(y.reshape(-1, C), None, None, g_t, b_t, True, 0.0, eps)
    else:
        u = F.batch_norm(y.reshape(-1, C), torch.from_numpy(running[0]), torch.from_numpy(running[1]), g_t, b_t, False, 0.0, eps)
    z = F.leaky_relu(u, slope).view(B, N, k, C)
    out, arg = z.max(dim=2)
    out.backward(torch.from_numpy(gout).view(B, N, C))
    # the same forward by hand, for the constants
    yn = y.detach().numpy().reshape(P, k, C)
    if running is None:
        mean, var = yn.reshape(-1, C).mean(0), yn.reshape(-1, C).var(0)
    else:
        mean, var = running
    invstd = 1.0 / np.sqrt(var + eps)
    argn = arg.numpy().reshape(P, C)
    ysel = np.take_along_axis(yn, argn[:, None, :], axis=1)[:, 0, :]
    usel = gamma * invstd * (ysel - mean) + beta
    assert np.abs(np.where(usel > 0, usel, slope * usel) - out.detach().numpy().reshape(P, C)).max() < 1e-12
    gz = gout.reshape(P, C) * np.where(usel > 0, 1.0, slope)
    a = gamma * invstd
    if running is None:
        dbeta, dgamma, Pk = gz.sum(0), (gz * (ysel - mean)).sum(0) * invstd, P * k
        k1, k2 = a * dbeta / Pk, a * dgamma * invstd / Pk
    else:
        k1, k2 = np.zeros(C), np.zeros(C)
    return UVt.grad.numpy(), (gz, argn.astype(np.int32), a, k1, k2, mean)


@pytest.mark.parametrize("gamma_sign", ["positive", "negative", "mixed"])
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("B,N,k,C,lists", [(2, 19, 5, 6, "knn"), (1, 24, 7, 3, "hubs")])
def test_scatter_ref_fp64_is_autograd_of_the_edge_tensor_stage(B, N, k, C, lists, mode, gamma_sign):
    rng = np.random.default_rng(N + C)
    UV = rng.standard_normal((B * N, 2 * C))
    idx = R.knn_like(B, N, k, 11) if lists == "knn" else R.hubs(B, N, k, 2, 11)
    gamma = rng.uniform(0.5, 1.5, C)
    gamma *= {"positive": 1.0, "negative": -1.0, "mixed": np.where(np.arange(C) % 2, -1.0, 1.0)}[gamma_sign]
    beta = rng.uniform(-0.5, 0.5, C)
    gout = rng.standard_normal((B * N, C))
    running = None if mode == "train" else (rng.uniform(-0.5, 0.5, C), rng.uniform(0.5, 2.0, C))
    want, (gz, arg, a, k1, k2, mu) = _stage_fp64(UV, idx, gamma, beta, gout, B, N, k, C, 1e-5, 0.2, running)
    if mode == "eval":
        assert not k1.any() and not k2.any()
    got = R.scatter_ref(UV, idx, gz, arg, a, k1, k2, mu, B, N, k, C, np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    # the fp32 evaluation is the same definition: a rounding away, not a formula away
    got32 = R.scatter_ref(UV.astype(np.float32), idx, gz, arg, a, k1, k2, mu, B, N, k, C, np.float32)
    assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 1e-4 * np.abs(want).max()


# ---- the gather ----------------------------------------------------------------------------------------------------------------------------

def _edge_values(UV, UVlo, idx, B, N, k, C):
    base = (np.arange(B * N) // N * N)[:, None]
    nb = base + idx.reshape(B * N, k)
    y = UV[nb, :C] + UV[:, None, C:]
    if UVlo is not None:
        y = y + (UVlo[nb, :C] + UVlo[:, None, C:])
    assert y.dtype == np.float32
    return y, UV[nb, :C]


@pytest.mark.parametrize("hilo", [False, True])
@pytest.mark.parametrize("B,N,k,C,ties", [(2, 40, 7, 5, False), (3, 33, 8, 5, True), (1, 16, 16, 9, False)])
def test_gather_ref_is_max_min_argmax_of_the_fp32_edge_values(B, N, k, C, ties, hilo):
    rng = np.random.default_rng(k + C)
    UV = rng.standard_normal((B * N, 2 * C)).astype(np.float32)
    UVlo = (rng.standard_normal((B * N, 2 * C)) * 2.0 ** -24).astype(np.float32) if hilo else None
    if ties:                                     # four distinct U rows per cloud: every row of 8 neighbours meets one of them twice
        src = np.arange(B * N) // N * N + np.arange(B * N) % N % 4
        UV[:, :C] = UV[src, :C]
        if hilo:
            UVlo[:, :C] = UVlo[src, :C]
    idx = R.knn_like(B, N, k, 2)
    r = R.gather_ref(UV, UVlo, idx, B, N, k, C)
    y, u = _edge_values(UV, UVlo, idx, B, N, k, C)
    assert np.array_equal(r["ymax"], y.max(1)) and np.array_equal(r["ymin"], y.min(1))
    assert np.array_equal(r["jmax"], y.argmax(1)) and np.array_equal(r["jmin"], y.argmin(1))          # np.argmax: the FIRST maximum
    if ties:
        later_equal = (y[:, ::-1, :].argmax(1) != k - 1 - y.argmax(1))
        assert later_equal.mean() > 0.3, "the tie case has no ties at the maximum"
    su = np.zeros_like(r["sumU"])
    for j in range(k):
        su = su + u[:, j, :]
    assert np.array_equal(r["sumU"], su)
    y64 = y.astype(np.float64)
    tot, sq = y64.sum((0, 1)), (y64 * y64).sum((0, 1))
    assert r["stats"].shape == ((B * N + 31) // 32, 2, C)
    assert np.abs(r["stats"][:, 0].sum(0) - tot).max() <= 1e-12 * np.abs(y64).sum((0, 1)).max()
    assert np.abs(r["stats"][:, 1].sum(0) - sq).max() <= 1e-12 * sq.max()
    # a row is the sum over ITS 32 points
    last = y64[(r["stats"].shape[0] - 1) * 32:]
    assert np.abs(r["stats"][-1, 0] - last.sum((0, 1))).max() <= 1e-12 * np.abs(last).sum((0, 1)).max()
    assert np.abs(r["stats_scale"][-1, 0] - np.abs(last).sum((0, 1))).max() <= 1e-12 * np.abs(last).sum((0, 1)).max()


def test_gather_ref_first_position_wins_a_constructed_tie():
    """One point, four neighbours whose U rows are (1, 3, 3, 1): max at position 1 (not 2), min at position 0 (not 3)."""
    C = 2
    UV = np.zeros((4, 2 * C), np.float32)
    UV[:, :C] = np.array([1, 3, 3, 1], np.float32)[:, None]
    UV[:, C:] = 0.5
    idx = np.tile(np.arange(4, dtype=np.int32), (1, 4, 1))
    r = R.gather_ref(UV, None, idx, 1, 4, 4, C)
    assert (r["jmax"] == 1).all() and (r["jmin"] == 0).all() and (r["ymax"] == 3.5).all() and (r["ymin"] == 1.5).all()
    assert (r["sumU"] == 8.0).all()


# ---- the weight forms ---------------------------------------------------------------------------------------------------------------------

def test_wcat_ref_is_the_factorisation_and_its_adjoint():
    rng = np.random.default_rng(0)
    Co, C, n = 5, 3, 7
    W = rng.standard_normal((Co, 2 * C)).astype(np.float32)
    Wcat = R.wcat_ref(W, False)
    assert Wcat.shape == (2 * Co, C) and Wcat.dtype == np.float32
    x, xn = rng.standard_normal((n, C)), rng.standard_normal((n, C))
    edge = np.concatenate([xn - x, x], axis=1) @ W.astype(np.float64).T                    # W [x_nbr - x_i, x_i]
    UVn, UVi = xn @ Wcat.astype(np.float64).T, x @ Wcat.astype(np.float64).T
    assert np.abs(edge - (UVn[:, :Co] + UVi[:, Co:])).max() <= 1e-6                        # (Wb - Wa is rounded to fp32 once)
    G = rng.standard_normal((2 * Co, C)).astype(np.float32)
    dW = R.wcat_ref(G, True)
    assert dW.shape == (Co, 2 * C)
    assert np.array_equal(dW[:, :C], G[:Co] - G[Co:]) and np.array_equal(dW[:, C:], G[Co:])
    # adjoint: <wcat(W), G> == <W, wcat_back(G)>
    assert abs((Wcat.astype(np.float64) * G).sum() - (W.astype(np.float64) * dW).sum()) <= 1e-5
