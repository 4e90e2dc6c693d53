"""GPU: the EdgeConv kernels (csrc/edgeconv.hip) and their autograd wrapper (misc/edgeconv.py) one operation at a time, against the
plain restatements of tests/edgeconv_ref.py (held to brute force and to torch.autograd by tests/test_edgeconv_ref_cpu.py).

* the gather, plain and with the products' residuals (``pcl_edgeconv_gather_hilo_f32``): max / min / positions / sumU BIT FOR BIT against
  ``gather_ref`` (the library is built with -ffp-contract=off), every BatchNorm partial row against the fp64 sums of ITS 32 points --
  with and without the XCD block remap, whole unrolled rounds and tails, k = 1, k = N, C > 256, ties at different positions;
* ``Y_lo`` of ``pcl_frag_linear_fwd_f32``: half an ulp at most, Y unchanged by asking for it, nothing written outside [P][N];
* the transposed neighbour lists with hubs (in-degree N, the insertion branch of the sorted form), at every wave count of the ordered
  form and with duplicates, against ``transpose_ref``;
* the backward, list form and per-edge form, against the per-edge definition in fp64 with the fp32 evaluation as yardstick: every
  channel-chunk width of the LDS kernel, channel tails, zero gradients, points of in-degree 0 and N, the global-atomic form;
* ``edge_conv`` through autograd against the fp64 edge-tensor formulation in training and evaluation mode, fp32 chains / flushed /
  flushed with residuals, at DGCNN's channel pairs with the block remap on; ``want_t``, ``cat_slice``, ``x`` without a gradient;
* ``pcl_edgeconv_wcat_f32`` both ways bit for bit, past one grid.
Shapes are the smallest that reach the path named beside them.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import oracle  # (the tests that search neighbours take the ``oracle`` fixture, which builds it)
import oracle.torch_backend  # noqa: F401  (registers the plain-PyTorch composite the fp64 reference evaluates with)

import edgeconv_ref as R
from pointcloudlib_amd import _lib

pytestmark = pytest.mark.gpu

SENT = -77.0


def P(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gpu(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- the gather ----------------------------------------------------------------------------------------------------------------------------

GATHER_SHAPES = [
    # B, N, k, C
    (2, 64, 20, 64), (1, 64, 40, 64),      # whole rounds of 10 and of 5
    (3, 33, 8, 5),                         # tail loop only (plain), one round + 3 (hilo); clouds straddle the 32-point blocks; last block ragged
    (1, 40, 33, 3),                        # k = 33
    (2, 17, 1, 7),                         # k = 1
    (1, 16, 16, 9),                        # k = N
    (1, 32, 20, 300),                      # C > 256: the channel stride of a workgroup's lanes
    (8, 64, 20, 40), (16, 32, 5, 64),      # the XCD block remap is on
    (8, 40, 20, 40),                       # B % 8 == 0 but N % 32 != 0: remap off
]


def _gather_inputs(B, N, k, C, hilo, ties):
    rng = np.random.default_rng(1000 * B + 10 * N + k + C)
    UV = rng.standard_normal((B * N, 2 * C)).astype(np.float32)
    UVlo = (rng.standard_normal((B * N, 2 * C)) * 2.0 ** -24).astype(np.float32) if hilo else None
    if ties:                               # eight distinct U rows per cloud: every row's neighbours meet some of them more than once
        src = np.arange(B * N) // N * N + np.arange(B * N) % N % 8
        UV[:, :C] = UV[src, :C]
        if hilo:
            UVlo[:, :C] = UVlo[src, :C]
    return UV, UVlo, R.knn_like(B, N, k, B + N + k)


def _run_gather(dev, UV, UVlo, idx, B, N, k, C, with_sumU=True):
    """-> outputs as NumPy arrays; one guard row behind every output must keep its sentinel."""
    G = B * N
    rows = _lib.lib().pcl_edgeconv_stat_rows(B, N)
    assert rows == (G + 31) // 32
    UVd, UVlod, idxd = _gpu(dev, UV), _gpu(dev, UVlo), _gpu(dev, idx)
    f = lambda: torch.full((G + 1, C), SENT, device=dev)
    i = lambda: torch.full((G + 1, C), -7, dtype=torch.int32, device=dev)
    ymax, ymin, jmax, jmin, sumU = f(), f(), i(), i(), (f() if with_sumU else None)
    stats = torch.full((rows + 1, 2, C), SENT, dtype=torch.float64, device=dev)
    if UVlo is None:
        _lib.call("pcl_edgeconv_gather_f32", P(UVd), P(idxd), B, N, k, C, P(ymax), P(ymin), P(jmax), P(jmin), P(stats), P(sumU), _st())
    else:
        _lib.call("pcl_edgeconv_gather_hilo_f32", P(UVd), P(UVlod), P(idxd), B, N, k, C, P(ymax), P(ymin), P(jmax), P(jmin), P(stats),
                  P(sumU), _st())
    torch.cuda.synchronize()
    out = {"ymax": ymax, "ymin": ymin, "jmax": jmax, "jmin": jmin, "stats": stats}
    if with_sumU:
        out["sumU"] = sumU
    for n, t in out.items():
        guard = t[-1].cpu()
        assert (guard == (-7 if t.dtype == torch.int32 else SENT)).all(), f"{n}: written past its last row"
    return {n: t[:-1].cpu().numpy() for n, t in out.items()}


def _check_gather(got, want):
    for n in ("ymax", "ymin", "jmax", "jmin", "sumU"):
        if n in got:
            assert np.array_equal(got[n].view(np.int32), want[n].view(np.int32)), f"{n}: not bit for bit the restatement"
    err = np.abs(got["stats"] - want["stats"])
    bound = 1e-12 * want["stats_scale"]
    worst = (err / np.maximum(want["stats_scale"], 1e-300)).max()
    assert (err <= bound).all(), f"stats rows: worst |err| / (sum|y|, sum y^2) = {worst:.3e} (row {np.unravel_index((err - bound).argmax(), err.shape)})"


@pytest.mark.parametrize("hilo", [False, True], ids=["plain", "hilo"])
@pytest.mark.parametrize("B,N,k,C", GATHER_SHAPES)
def test_gather_is_the_restatement_bit_for_bit(dev, B, N, k, C, hilo):
    UV, UVlo, idx = _gather_inputs(B, N, k, C, hilo, ties=False)
    _check_gather(_run_gather(dev, UV, UVlo, idx, B, N, k, C), R.gather_ref(UV, UVlo, idx, B, N, k, C))


@pytest.mark.parametrize("hilo", [False, True], ids=["plain", "hilo"])
@pytest.mark.parametrize("B,N,k,C", [(2, 64, 20, 64), (3, 33, 8, 5)])
def test_gather_first_position_wins_a_tie(dev, B, N, k, C, hilo):
    """Duplicated U rows: equal edge values at different positions of a row, at the maximum and the minimum among them."""
    UV, UVlo, idx = _gather_inputs(B, N, k, C, hilo, ties=True)
    want = R.gather_ref(UV, UVlo, idx, B, N, k, C)
    base = (np.arange(B * N) // N * N)[:, None]
    y = UV[base + idx.reshape(B * N, k), :C] + UV[:, None, C:]
    if hilo:
        y = y + (UVlo[base + idx.reshape(B * N, k), :C] + UVlo[:, None, C:])
    tied_max = (k - 1 - y[:, ::-1, :].argmax(1)) != y.argmax(1)              # the last maximum is not the first
    assert tied_max.mean() > 0.3, "the inputs have no ties at the maximum"
    _check_gather(_run_gather(dev, UV, UVlo, idx, B, N, k, C), want)


@pytest.mark.parametrize("hilo", [False, True], ids=["plain", "hilo"])
def test_gather_without_sumU(dev, hilo):
    B, N, k, C = 3, 33, 8, 5
    UV, UVlo, idx = _gather_inputs(B, N, k, C, hilo, ties=False)
    got = _run_gather(dev, UV, UVlo, idx, B, N, k, C, with_sumU=False)
    assert "sumU" not in got
    _check_gather(got, R.gather_ref(UV, UVlo, idx, B, N, k, C))


# ---- Y_lo of the flushed few-row GEMM ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flush", [8, 32])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("Pr,K,N", [(70, 3, 128), (130, 64, 128), (65, 128, 256), (33, 20, 40)])
def test_frag_forward_residual(dev, Pr, K, N, pad, flush):
    """pcl_frag_linear_fwd_f32(Y_lo): the residual of rounding the fp64 sum to fp32.  Asking for it leaves Y as it was; |Y_lo| <= 2^-24 |Y|
    (half an ulp: the residual of a round-to-nearest); rows behind P and the pad columns of both buffers keep their sentinels; Y + Y_lo is
    no further from the fp64 product than Y alone (mean absolute error)."""
    g = torch.Generator().manual_seed(Pr * 31 + K)
    X = torch.randn(Pr, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    want = X.double() @ W.double().t()
    ldy = N + pad
    Xd, Wd = X.to(dev), W.to(dev)

    def run(with_lo):
        Y = torch.full((Pr + 2, ldy), SENT, device=dev)
        Ylo = torch.full((Pr + 2, ldy), SENT, device=dev) if with_lo else None
        _lib.call("pcl_frag_linear_fwd_f32", P(Xd), K, P(Wd), K, None, None, None, 0.0, Pr, K, N, P(Y), ldy, P(Ylo), None, flush, _st())
        torch.cuda.synchronize()
        return Y.cpu(), (None if Ylo is None else Ylo.cpu())

    Y0, _ = run(False)
    Y1, Ylo = run(True)
    assert torch.equal(Y0, Y1), "Y changes when Y_lo is requested"
    for name, t in (("Y", Y1), ("Y_lo", Ylo)):
        assert (t[Pr:] == SENT).all(), f"{name}: rows behind P were written"
        assert (t[:, N:] == SENT).all(), f"{name}: columns past N were written"
    y, lo = Y1[:Pr, :N], Ylo[:Pr, :N]
    assert (y != SENT).all() and (lo != SENT).all()
    assert (lo.abs() <= y.abs() * 2.0 ** -24).all(), f"|Y_lo| exceeds half an ulp of Y: worst ratio {(lo.abs() / y.abs()).max().item() * 2 ** 24:.3f} x 2^-24"
    e_y = (y.double() - want).abs().mean().item()
    e_sum = (y.double() + lo.double() - want).abs().mean().item()
    print(f"\n[Y_lo P={Pr} K={K} N={N} ldy={ldy} flush={flush}] mean |err| vs fp64: Y {e_y:.3e}, Y + Y_lo {e_sum:.3e}")
    assert e_sum <= e_y


# ---- transposed neighbour lists ---------------------------------------------------------------------------------------------------------

LIST_CASES = [
    # B, N, k, builder
    (2, 300, 70, "hubs"),         # sorted form; in-degree 300 > 256: the insertion branch of the sort
    (1, 130, 65, "knn"),          # either side of the switch between the forms
    (1, 130, 64, "knn"),
    (2, 512, 20, "hubs"),         # ordered form, in-degree N
    (1, 8192, 3, "knn"),          # two waves file the sources
    (1, 2048, 5, "knn"),          # eight
    (1, 1927, 4, "knn"),          # the last N with sixteen
    (1, 1928, 4, "knn"),          # the first with eight
    (3, 64, 8, "dup"),            # a row names a point twice
]


def _lists(B, N, k, builder, seed):
    if builder == "hubs":
        return R.hubs(B, N, k, 2, seed)
    return R.with_duplicates(B, N, k, seed) if builder == "dup" else R.knn_like(B, N, k, seed)


@pytest.mark.parametrize("B,N,k,builder", LIST_CASES)
def test_transposed_lists_with_hubs_and_at_every_wave_count(dev, B, N, k, builder):
    idx = _lists(B, N, k, builder, N + k)
    want_off, want_src = R.transpose_ref(idx, B, N, k)
    if builder == "hubs":
        deg = np.diff(want_off).reshape(B, N)
        assert (deg[:, :2] == N).all() and (deg[:, N - N // 8:] == 0).all()
    idxd = _gpu(dev, idx)
    in_off = torch.full((B * N + 2,), -7, dtype=torch.int32, device=dev)
    in_src = torch.full((B * N * k + 1,), -7, dtype=torch.int32, device=dev)
    _lib.call("pcl_knn_transpose_i32", P(idxd), B, N, k, P(in_off), P(in_src), _st())
    torch.cuda.synchronize()
    off, src = in_off.cpu().numpy(), in_src.cpu().numpy()
    assert off[-1] == -7 and src[-1] == -7, "written past the end"
    off, src = off[:-1], src[:-1]
    assert np.array_equal(off, want_off)
    if builder == "dup":          # two edges of one row into one list: their mutual order is unspecified -- compare every list as a sorted multiset
        lid = np.repeat(np.arange(B * N), np.diff(want_off))
        src, want_src = src[np.lexsort((src, lid))], want_src[np.lexsort((want_src, lid))]
    assert np.array_equal(src, want_src)


# ---- the backward -------------------------------------------------------------------------------------------------------------------------

SCATTER_CASES = [
    # B, N, k, C, builder, lists
    (2, 33, 8, 5, "knn", True),           # N * CH < 1024: the clamp of the LDS kernel's unrolled pairs; C % 16 != 0
    (8, 64, 20, 40, "knn", True),         # the list sum's block remap on
    (8, 66, 20, 40, "knn", True),         # ... off (N % 4 != 0)
    # N * CH fp64 cells <= 64 KiB: CH = 16 up to N = 512, then 8 / 4 / 2 / 1 at N = 1024 / 2048 / 4096 / 8192
    (1, 1024, 6, 12, "knn", True),        # CH = 8 (DGCNN cls runs N = 1024), two channel blocks, the last with 4 of 8 channels
    (1, 2048, 6, 12, "knn", True),        # CH = 4, three whole channel blocks (DGCNN part-seg runs N = 2048)
    (1, 2048, 6, 14, "knn", True),        # CH = 4, the last block with 2 of 4 channels
    (1, 4096, 4, 6, "knn", True),         # CH = 2, three whole blocks
    (1, 4096, 4, 7, "knn", True),         # CH = 2, the last block with 1 of 2 channels
    (1, 8192, 3, 5, "knn", True),         # CH = 1, five channel blocks: the largest N of the LDS form
    (2, 256, 20, 64, "hubs", True),       # in-degrees 0 and N
    (1, 16400, 2, 3, "knn", True),        # N * 8 B > 64 KiB at CH = 1: global atomics + memset
    (1, 16400, 2, 3, "knn", False),       # the per-edge form above 8192 points
]


@pytest.mark.parametrize("B,N,k,C,builder,lists", SCATTER_CASES)
def test_scatter_is_the_per_edge_definition(dev, B, N, k, C, builder, lists):
    """Both forms of pcl_edgeconv_scatter_f32 against ``scatter_ref`` in fp64; lists from ``transpose_ref`` and sumU from ``gather_ref``, so
    no other kernel stands between the inputs and the result.  Per output half: max |got - fp64| <= max(2e-5 max(1, |fp64|_max) (the bound
    of the lists-vs-atomics test), 4 x the error of the fp32 evaluation of the definition (covers the hub sums over N terms))."""
    G = B * N
    rng = np.random.default_rng(N + 7 * k + C)
    UV = rng.standard_normal((G, 2 * C)).astype(np.float32)
    idx = _lists(B, N, k, builder, N + C)
    gz = rng.standard_normal((G, C)).astype(np.float32)
    gz[rng.random((G, C)) < 0.25] = 0.0                                      # about a quarter exactly zero: the kernels skip those atomics
    arg = rng.integers(0, k, size=(G, C)).astype(np.int32)
    a, k1, k2, mu = ((rng.standard_normal(C) * s).astype(np.float32) for s in (1.0, 0.01, 0.01, 0.5))
    want = R.scatter_ref(UV, idx, gz, arg, a, k1, k2, mu, B, N, k, C, np.float64)
    yard = R.scatter_ref(UV, idx, gz, arg, a, k1, k2, mu, B, N, k, C, np.float32)
    keep = [_gpu(dev, t) for t in (UV, idx, gz, arg, a, k1, k2, mu)]
    in_off = in_src = sumU = None
    if lists:
        off, src = R.transpose_ref(idx, B, N, k)
        in_off, in_src = _gpu(dev, off), _gpu(dev, src)
        sumU = _gpu(dev, R.gather_ref(UV, None, idx, B, N, k, C)["sumU"])
    dUV = torch.full((G + 1, 2 * C), SENT, device=dev)
    _lib.call("pcl_edgeconv_scatter_f32", *(P(t) for t in keep), B, N, k, C, P(in_off), P(in_src), P(sumU), P(dUV), _st())
    torch.cuda.synchronize()
    got = dUV.cpu().numpy()
    assert (got[-1] == SENT).all(), "dUV: written past its last row"
    got = got[:-1].astype(np.float64)
    for name, sl in (("dU", slice(0, C)), ("dV", slice(C, 2 * C))):
        e_got = np.abs(got[:, sl] - want[:, sl]).max()
        e_yard = np.abs(yard[:, sl].astype(np.float64) - want[:, sl]).max()
        bound = max(2e-5 * max(1.0, np.abs(want[:, sl]).max()), 4 * e_yard)
        print(f"\n[scatter B={B} N={N} k={k} C={C} {builder} lists={lists}] {name}: max |err| vs fp64 {e_got:.3e}, fp32 per-edge evaluation {e_yard:.3e}, "
              f"|fp64|_max {np.abs(want[:, sl]).max():.3e}, bound {bound:.3e}")
        assert e_got <= bound, name


# ---- edge_conv through autograd -----------------------------------------------------------------------------------------------------------

STAGE_SHAPES = [
    # B, N, C, Cout, k
    (8, 64, 64, 64, 20), (8, 64, 64, 128, 20), (8, 32, 128, 256, 20),      # DGCNN's channel pairs beyond 3 -> 64, block remap on
    (2, 96, 64, 64, 40),                                                   # the part-seg stage's k
    (3, 50, 5, 40, 7),                                                     # nothing divides anything
]
SETTINGS = {"flush0": (0, False), "flush8": (8, False), "hilo": (8, True)}


@functools.lru_cache(maxsize=None)
def _stage_inputs(shape, training):
    """Module, input, lists, output gradient and the fp64 edge-tensor evaluation of one (shape, mode): built once and shared.  Nobody may
    run or modify the returned module: ``_run_stage`` deep-copies it for every call, so its running statistics stay the initial ones."""
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    B, N, C, Cout, k = shape
    dev = torch.device("cuda:0")
    torch.manual_seed(N + C + Cout)
    mlp = PointwiseMLP([2 * C, Cout], slope=0.2).to(dev)
    mlp.gammas[0].data.uniform_(-1.0, 1.5)                 # both signs: the max / min choice
    mlp.betas[0].data.uniform_(-0.5, 0.5)
    mlp.running_mean_0.uniform_(-0.5, 0.5)                 # evaluation mode normalises with these
    mlp.running_var_0.uniform_(0.5, 2.0)
    mlp.train(training)
    x = torch.randn(B, N, C, device=dev)
    xn = x.cpu().numpy().transpose(0, 2, 1).copy()
    idx = torch.from_numpy(oracle.knn(xn, xn, k).transpose(0, 2, 1).copy()).to(dev)
    g = torch.randn(B, N, Cout, device=dev)
    ref = copy.deepcopy(mlp).double(); ref.backend = "torch"
    exp = R.edge_tensor_stage(ref, x, idx, g)
    exp["running_mean_0"], exp["running_var_0"] = ref.running_mean_0.clone(), ref.running_var_0.clone()
    return mlp, x, idx, g, {n: t.cpu() for n, t in exp.items()}


def _run_stage(shape, training, flush_k, hilo, x_grad=True, **kw):
    """One forward + backward of ``edge_conv`` on a fresh copy of the shared module -> ({name: CPU tensor}, whatever else edge_conv returned)."""
    from pointcloudlib_amd.misc.edgeconv import edge_conv
    mlp0, x, idx, g, _ = _stage_inputs(shape, training)
    mlp = copy.deepcopy(mlp0)
    mlp.flush_k, mlp.edge_hilo = flush_k, hilo
    xa = x.clone().requires_grad_(x_grad)
    res = edge_conv(mlp, xa, idx, **kw)
    out, out_t = res if kw.get("want_t") else (res, None)
    out.backward(g)
    torch.cuda.synchronize()
    got = {"out": out.detach().cpu(), **{n: p.grad.cpu() for n, p in mlp.named_parameters()},
           "running_mean_0": mlp.running_mean_0.cpu(), "running_var_0": mlp.running_var_0.cpu()}
    if x_grad:
        got["dx"] = xa.grad.cpu()
    return got, out_t


@functools.lru_cache(maxsize=None)
def _stage(shape, training, setting):
    return _run_stage(shape, training, *SETTINGS[setting])[0]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_conv_matches_the_fp64_edge_tensor_stage(oracle, dev, shape, training, setting):
    """Output, dx, every parameter gradient and the running statistics within 2e-5 max(1, |reference|_max) of the fp64 edge-tensor
    formulation (the reference and bound of test_networks_gpu.py::test_edgeconv_factorised_matches_edge_tensor), in training mode (batch
    statistics) and evaluation mode (running statistics; dgamma / dbeta formed on the host, k1 = k2 = 0)."""
    mlp0, _, _, _, exp = _stage_inputs(shape, training)
    got = _stage(shape, training, setting)
    assert set(got) == set(exp)
    line = []
    for n in exp:
        s = max(1.0, exp[n].abs().max().item())
        err = (got[n].double() - exp[n]).abs().max().item()
        line.append(f"{n} {err:.2e}/{s:.2f}")
    print(f"\n[edge_conv {shape} {'train' if training else 'eval'} {setting}] max |err| / scale: " + ", ".join(line))
    for n in exp:
        s = max(1.0, exp[n].abs().max().item())
        assert (got[n].double() - exp[n]).abs().max().item() <= 2e-5 * s, n
    if not training:
        for b in ("running_mean_0", "running_var_0"):
            assert torch.equal(got[b], getattr(mlp0, b).cpu()), f"{b} moved in evaluation mode"


@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_conv_residuals_do_not_lose_accuracy(oracle, dev, shape):
    """The residual-carrying gather is the more accurate form by design: on equal inputs its output is no further from the
    fp64 evaluation than the flushed products without residuals."""
    exp = _stage_inputs(shape, True)[4]["out"]
    e = {s: (_stage(shape, True, s)["out"].double() - exp).abs().max().item() for s in SETTINGS}
    print(f"\n[edge_conv {shape} train] max |out - fp64|: residuals {e['hilo']:.3e}, flush 8 {e['flush8']:.3e}, fp32 chains {e['flush0']:.3e}")
    assert e["hilo"] <= e["flush8"]
    # the residuals must have been USED: with more than flush_k = 8 terms per product they are not zero and move last bits of y, hence of
    # the output or of which neighbour wins (dW); with C = 5 there is one fp32 chain, the residuals are exactly zero and nothing may move
    hilo, plain = _stage(shape, True, "hilo"), _stage(shape, True, "flush8")
    same = all(torch.equal(hilo[n], plain[n]) for n in ("out", "weights.0", "dx"))
    assert same == (shape[2] <= 8), "edge_hilo made no difference" if same else "zero residuals changed the result"


@pytest.mark.parametrize("setting", ["flush8", "hilo"])
def test_edge_conv_calls_the_gather_its_setting_names(oracle, dev, monkeypatch, setting):
    """``edge_hilo`` reaches pcl_edgeconv_gather_hilo_f32 with a residual buffer; without it the plain gather runs."""
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **kw: (called.append(name), real(name, *a, **kw))[1])
    _run_stage((3, 50, 5, 40, 7), True, *SETTINGS[setting])
    gathers = [n for n in called if n.startswith("pcl_edgeconv_gather")]
    assert gathers == ["pcl_edgeconv_gather_hilo_f32" if setting == "hilo" else "pcl_edgeconv_gather_f32"]


def _assert_same_bits(got, base, what):
    """Every tensor of two runs on equal inputs, bit for bit (dW and dx pass through dU, whose hits edgeconv_hits_lds_kernel sums in fp64
    cells so that the order of its atomics does not show: DESIGN 18)."""
    for n in got:
        assert torch.equal(got[n], base[n]), (n, what)


CAT_SHAPES = [(2, 64, 5, 40, 7), (3, 50, 5, 40, 7)]          # N = 64, Cout = 40: pcl_group_minmax_finalize_t_f32 with a channel tail; N = 50: the fallback


@pytest.mark.parametrize("shape", CAT_SHAPES, ids=["N64-Cout40", "N50-fallback"])
def test_edge_conv_transposed_copy_and_concat_slice(oracle, dev, shape):
    """``want_t``: out_t is out transposed per cloud.  ``cat_slice`` (columns 7 .. 7 + Cout of a sentinel-filled [B, N, Cout + 20] buffer):
    the slice receives the output, every other column keeps its sentinel, and the result and every gradient are those of the call without
    it bit for bit."""
    B, N, C, Cout, k = shape
    base = _stage(shape, True, "flush8")
    for want_t in (False, True):
        buf = torch.full((B, N, Cout + 20), SENT, device=dev)
        got, out_t = _run_stage(shape, True, 8, False, cat_slice=buf[:, :, 7:7 + Cout], **({"want_t": True} if want_t else {}))
        assert set(got) == set(base)
        _assert_same_bits(got, base, want_t)
        buf = buf.cpu()
        assert torch.equal(buf[:, :, 7:7 + Cout], base["out"]), want_t
        assert (buf[:, :, :7] == SENT).all() and (buf[:, :, 7 + Cout:] == SENT).all(), "cat_slice: columns outside the slice were written"
        if want_t:
            assert out_t.shape == (B, Cout, N) and out_t.is_contiguous() and not out_t.requires_grad
            assert torch.equal(out_t.cpu(), base["out"].transpose(1, 2))
    got, out_t = _run_stage(shape, True, 8, False, want_t=True)              # the transposed copy alone
    assert out_t.shape == (B, Cout, N) and torch.equal(out_t.cpu(), base["out"].transpose(1, 2))
    assert set(got) == set(base)
    _assert_same_bits(got, base, "want_t")


NO_GRAD_CASES = [((3, 50, 5, 40, 7), "flush0"), ((8, 64, 64, 64, 20), "flush8"), ((2, 96, 64, 64, 40), "hilo")]


@pytest.mark.parametrize("shape,setting", NO_GRAD_CASES, ids=[s for _, s in NO_GRAD_CASES])
def test_edge_conv_input_without_gradient(oracle, dev, shape, setting):
    """``x`` without requires_grad: no dx is formed; the output, the parameter gradients and the running statistics are bit for bit those
    of the call with it."""
    base = _stage(shape, True, setting)
    got, _ = _run_stage(shape, True, *SETTINGS[setting], x_grad=False)
    assert set(got) == set(base) - {"dx"}
    _assert_same_bits(got, base, setting)


# ---- the weight forms ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Co,C", [(64, 3), (256, 128), (520, 512)])          # (520 x 512 = 266 240 elements: past one grid of 1024 x 256)
def test_wcat_both_ways_bit_for_bit(dev, Co, C):
    rng = np.random.default_rng(Co + C)
    for back, shape in ((0, (Co, 2 * C)), (1, (2 * Co, C))):
        src = rng.standard_normal(shape).astype(np.float32)
        want = R.wcat_ref(src, bool(back))
        srcd = _gpu(dev, src)
        dst = torch.full((want.size + 64,), SENT, device=dev)
        _lib.call("pcl_edgeconv_wcat_f32", P(srcd), Co, C, back, P(dst), _st())
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert (got[want.size:] == SENT).all(), "written past the end"
        assert np.array_equal(got[:want.size].view(np.int32), want.ravel().view(np.int32)), ("backward" if back else "forward")
