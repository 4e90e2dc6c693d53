"""GPU: the reference's own index kernels (their CUDA text compiled by hipcc for gfx950, oracle/ref_kernels.py) beside the oracle
and the HIP library, on the same inputs (oracle/ref_cases.py).  Integer equality everywhere, no tolerance.

The -ffp-contract=off build is the gate: it must equal ``oracle.*`` in its default reading and ``ops.*`` with
``tie_stride = block_size``.  The -ffp-contract=fast build is asserted where its result does not depend on which products a
compiler fuses.  The reference's output is the truth; the only place where the library deliberately differs is the row of a ball
query without a hit, which the reference leaves unwritten and the library defines as zeros."""
import numpy as np
import pytest
import torch

from oracle import ref_cases as rc
from oracle import ref_kernels
from pointcloudlib_amd.misc import ops

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.cpu().numpy()


def _load(contract):
    ref = ref_kernels.load(contract)
    if ref is None:
        pytest.skip(f"oracle/_ref/libpcl_ref_{contract}.so not built: __graft_entry__.build() makes it where a reference checkout "
                    "is present (tests/test_reference_golden_cpu.py fails there if it did not)")
    return ref


@pytest.fixture(scope="module")
def ref(dev):
    return _load("off")


@pytest.fixture(scope="module")
def ref_fast(dev):
    return _load("fast")


_CACHE = {}


def cached(key, fn):
    """inputs and CPU results are computed once and shared between the gate and the fast-build tests; nobody writes to them"""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ------------------------------------------------------------------------------------ FPS
FPS_NAMES = ["plain300", "plain37", "lattice100", "lattice257", "skips64", "capped128"]


def fps_case(oracle, name):
    def make():
        xyz, m = cached("fps_cases", rc.fps_cases)[name]
        return xyz, m, {S: oracle.fps(xyz, m, block_size=S) for S in rc.FPS_BLOCKS}
    return cached(("fps", name), make)


def test_fps_case_list_is_complete():
    assert sorted(FPS_NAMES) == sorted(rc.fps_cases())


@pytest.mark.parametrize("name", FPS_NAMES)
def test_fps_reference_kernel_equals_oracle_and_library(oracle, dev, ref, name):
    xyz, m, want = fps_case(oracle, name)
    B, N, _ = xyz.shape
    assert B <= 4 and N <= 300
    x = T(xyz, dev)
    for S in rc.FPS_BLOCKS:
        truth = N_(ref.fps(x, m, S))
        assert truth.min() >= 0 and truth.max() < N, (name, S)                      # every slot written, every index in range
        assert np.array_equal(want[S], truth), f"oracle.fps differs from the reference kernel: {name} block_size={S}"
        got, got_xyz = ops.furthest_point_sample(x, m, tie_stride=S)
        assert np.array_equal(N_(got), truth), f"ops.furthest_point_sample differs from the reference kernel: {name} tie_stride={S}"
        assert np.array_equal(N_(got_xyz), np.take_along_axis(xyz, truth[..., None].astype(np.int64), 1))
    # what each case is there for, read off the reference's own output
    if name.startswith("lattice"):
        # m = N: after the last distinct live site every pick is an exact tie at distance 0 (the picks repeat earlier sites);
        # the tie order depends on the block size, so the block sizes must not all agree
        sites = len({tuple(p) for p in xyz[0].tolist()} - {(0.0, 0.0, 0.0)})
        assert sites < m
        assert len({N_(ref.fps(x, m, S)).tobytes() for S in rc.FPS_BLOCKS}) > 1
    if name == "skips64":
        truth = N_(ref.fps(x, m, 8))
        live = rc.sqnorm_f32(xyz).astype(np.float64) > rc.SKIP
        assert not live[0, 0] and not live[1, 0] and (truth[:, 0] == 0).all()        # a dead point 0 is still the first pick
        assert not live[3].any() and (truth[3] == 0).all()                           # no live point: every pick is 0
        for b in range(3):
            assert set(truth[b, 1:].tolist()) - {0} == set(np.flatnonzero(live[b]).tolist()) - {0}, b
        for b, i in rc.SKIPS_BOUNDARY["kept"]:                                       # mag == float32(1e-3) > 1e-3: sampled
            assert rc.sqnorm_f32(xyz[b, i]) == rc.SKIP_F32 and i in truth[b]
        for b, i in rc.SKIPS_BOUNDARY["skipped"]:                                    # one float below: not sampled
            assert float(rc.sqnorm_f32(xyz[b, i])) < rc.SKIP and i not in truth[b]
    if name == "capped128":
        d = ((xyz[:, :, None].astype(np.float64) - xyz[:, None]) ** 2).sum(-1)
        assert (d[:, 0] > 1e10).any()                                                # the first step already meets the cap


@pytest.mark.parametrize("name", FPS_NAMES)
def test_fps_fast_build_where_contraction_cannot_matter(oracle, dev, ref_fast, name):
    """a*a + b*b + c*c can be contracted in more than one way and the oracle's second reading is nvcc's, so the fast build is
    compared only where the oracle's two readings give the same indices (checked first); the lattice clouds do so by construction
    (every product exact).  The boundary points of skips64 are built for one rounding sequence of `mag`: they are made dead here."""
    xyz, m, want = fps_case(oracle, name)
    if name == "skips64":
        xyz = xyz.copy()
        for b, i in rc.SKIPS_BOUNDARY["kept"] + rc.SKIPS_BOUNDARY["skipped"]:
            xyz[b, i] = 0
        want = {S: oracle.fps(xyz, m, block_size=S) for S in rc.FPS_BLOCKS}
    with oracle.contract("fma"):
        for S in rc.FPS_BLOCKS:
            assert np.array_equal(oracle.fps(xyz, m, block_size=S), want[S]), f"precondition: pick another seed for {name}"
    x = T(xyz, dev)
    for S in rc.FPS_BLOCKS:
        truth = N_(ref_fast.fps(x, m, S))
        assert np.array_equal(want[S], truth), (name, S)
        assert np.array_equal(N_(ops.furthest_point_sample(x, m, tie_stride=S)[0]), truth), (name, S)


# ------------------------------------------------------------------------------------ ball query
BQ_NAMES = ["saturation", "exact_radius", "hitless", "rim"]


def bq_case(oracle, name):
    def make():
        q, xyz, radii, n_hitless = cached("bq_cases", lambda: rc.bq_cases(oracle))[name]
        want = {(r, ns): oracle.ball_query(q, xyz, r, ns, return_cnt=True) for r in radii for ns in rc.BQ_NSAMPLES}
        return q, xyz, radii, n_hitless, want
    return cached(("bq", name), make)


def check_ball_query(name, truth, tcnt, want, wcnt, got, gcnt, n_hitless):
    """reference (idx prefilled with -1) against the oracle and the library: rows with a hit in full, rows without as defined"""
    B, m, ns = truth.shape
    hitless = np.zeros((B, m), bool)
    if n_hitless:
        hitless[:, m - n_hitless:] = True
    assert np.array_equal(tcnt == 0, hitless), f"{name}: rows without a hit are not exactly the {n_hitless} appended ones"
    assert (truth[hitless] == -1).all(), f"{name}: the reference wrote a row that has no hit"
    assert (truth[~hitless] >= 0).all()
    for who, idx, cnt in (("oracle.ball_query", want, wcnt), ("ops.ball_query", got, gcnt)):
        assert np.array_equal(cnt, tcnt), f"{who}: counts differ from the reference kernel ({name})"
        assert np.array_equal(idx[~hitless], truth[~hitless]), f"{who}: lists differ from the reference kernel ({name})"
        assert (idx[hitless] == 0).all(), f"{who}: a row without a hit is defined as zeros ({name})"


def test_bq_case_list_is_complete(oracle):
    assert sorted(BQ_NAMES) == sorted(rc.bq_cases(oracle))


@pytest.mark.parametrize("name", BQ_NAMES)
def test_ball_query_reference_kernel_equals_oracle_and_library(oracle, dev, ref, name):
    q, xyz, radii, n_hitless, want = bq_case(oracle, name)
    B, m, _ = q.shape
    assert B <= 3 and xyz.shape[1] <= 300 and m <= 64
    Q, X = T(q, dev), T(xyz, dev)
    for r in radii:
        for ns in rc.BQ_NSAMPLES:
            got, gcnt = ops.ball_query(Q, X, r, ns, return_cnt=True)
            for block in (ops.optimal_block(B), 64):
                truth, tcnt = ref.ball_query(Q, X, r, ns, block)
                check_ball_query((name, r, ns, block), N_(truth), N_(tcnt), *want[(r, ns)], N_(got), N_(gcnt), n_hitless)
    if name == "saturation":
        for r in radii:                                  # lists that fill up and lists that do not, at both radii
            cnt = want[(r, 8)][1]
            assert (cnt == 8).any() and (cnt < 8).any(), r
    if name == "exact_radius":
        # all arithmetic on the lattice is exact: the fp32 distances ARE the distances.  At nsample = 64 no list is full, so each
        # holds every hit: exactly the points with d2 < 0.25, none of the many at d2 == 0.25 = fl(0.5 * 0.5)
        d2 = ((q[:, :, None] - xyz[:, None]) ** 2).sum(-1)
        assert d2.dtype == np.float32 and (d2 == 0.25).sum() > 100
        truth, tcnt = (N_(t) for t in ref.ball_query(Q, X, 0.5, 64, 64))
        assert (tcnt < 64).all()
        for b in range(B):
            for j in range(m):
                assert truth[b, j, :tcnt[b, j]].tolist() == np.flatnonzero(d2[b, j] < 0.25).tolist(), (b, j)


    if name == "rim":
        # query 0 is the origin: a point at exactly float32(r) on an axis has d2 == fl(r*r) == radius2 -> excluded by the strict
        # `<` on the fp32 product (at 0.3 the exact square is larger: a radius2 kept in double would take it); one float inside -> in
        for i, r in enumerate(radii):
            truth, tcnt = (N_(t) for t in ref.ball_query(Q, X, r, 64, 64))
            assert (q[:, 0] == 0).all() and tcnt[:, 0].max() < 64
            for b in range(B):
                hits = truth[b, 0, :tcnt[b, 0]].tolist()
                for on in rc.RIM_ON[i]:
                    assert rc.sqnorm_f32(xyz[b, on]) == np.float32(r) * np.float32(r) and on not in hits, (r, b, on)
                assert rc.RIM_INSIDE[i] in hits, (r, b)
        r3 = np.float32(0.3)
        assert float(r3 * r3) < float(r3) * float(r3)


@pytest.mark.parametrize("name", ["saturation", "hitless"])
def test_ball_query_multi_equals_reference_kernel_per_radius(oracle, dev, ref, name):
    q, xyz, radii, n_hitless, want = bq_case(oracle, name)
    Q, X = T(q, dev), T(xyz, dev)
    nss = [8, 64]
    multi = ops.ball_query_multi(Q, X, list(radii), nss, return_cnt=True)
    for (got, gcnt), r, ns in zip(multi, radii, nss):
        truth, tcnt = ref.ball_query(Q, X, r, ns, ops.optimal_block(q.shape[0]))
        check_ball_query((name, "multi", r, ns), N_(truth), N_(tcnt), *want[(r, ns)], N_(got), N_(gcnt), n_hitless)


@pytest.mark.parametrize("name", BQ_NAMES)
def test_ball_query_fast_build_where_contraction_cannot_matter(oracle, dev, ref_fast, name):
    """as for FPS: compared where the oracle's two readings agree (checked first); exact_radius is such an input by construction"""
    q, xyz, radii, n_hitless, want = bq_case(oracle, name)
    Q, X = T(q, dev), T(xyz, dev)
    for r in radii:
        for ns in rc.BQ_NSAMPLES:
            with oracle.contract("fma"):
                assert np.array_equal(oracle.ball_query(q, xyz, r, ns), want[(r, ns)][0]), f"precondition: pick another seed for {name}"
            truth, tcnt = ref_fast.ball_query(Q, X, r, ns, 64)
            got, gcnt = ops.ball_query(Q, X, r, ns, return_cnt=True)
            check_ball_query((name, "fast", r, ns), N_(truth), N_(tcnt), *want[(r, ns)], N_(got), N_(gcnt), n_hitless)


# ------------------------------------------------------------------------------------ k-NN
KNN_NAMES = [rc.knn_name(s) for s in rc.KNN_SHAPES] + ["lattice", "lattice_kNr", "zeros"]


def knn_case(oracle, name):
    def make():
        x_q, x_r, k = cached("knn_cases", rc.knn_cases)[name]
        want = oracle.knn(x_q, x_r, k)
        with oracle.contract("fma"):
            want_fma = oracle.knn(x_q, x_r, k)
        return x_q, x_r, k, want, want_fma
    return cached(("knn", name), make)


def test_knn_case_list_is_complete():
    assert sorted(KNN_NAMES) == sorted(rc.knn_cases())
    assert [tuple(s) for s in rc.KNN_SHAPES] == [(2, 3, 64, 64, 5), (2, 5, 33, 20, 33), (1, 7, 100, 37, 1), (2, 64, 257, 130, 20),
                                                 (1, 130, 300, 50, 7), (1, 3, 5000, 70, 9)]


@pytest.mark.parametrize("name", KNN_NAMES)
def test_knn_reference_kernels_equal_oracle_and_library(oracle, dev, ref, name):
    x_q, x_r, k, want, _ = knn_case(oracle, name)
    Q, R = T(x_q, dev), T(x_r, dev)
    truth = N_(ref.knn(Q, R, k))
    assert truth.shape == (x_q.shape[0], k, x_q.shape[2]) and truth.min() >= 0 and truth.max() < x_r.shape[2]
    assert np.array_equal(want, truth), f"oracle.knn differs from the reference kernels: {name}"
    assert np.array_equal(N_(ops.knn_indices(Q, R, k, contract="")), truth), f"ops.knn_indices differs from the reference kernels: {name}"
    assert np.array_equal(N_(ops.knn_lists(Q, R, k)), truth.transpose(0, 2, 1)), f"ops.knn_lists differs from the reference kernels: {name}"
    if name == "zeros":                                   # every distance 0: the stable sort keeps 0..k-1
        assert (truth == np.arange(k)[None, :, None]).all()
    if name.startswith("lattice"):
        # repeated references: exact ties.  Lattice arithmetic is exact, so the fp32 distances ARE the distances and the answer is
        # known without any kernel: the k smallest by (distance, index) -- a stable sort
        d2 = ((x_r[:, :, :, None] - x_q[:, :, None, :]) ** 2).sum(1)
        assert d2.dtype == np.float32 and (np.sort(d2, 1)[:, 1:k] == np.sort(d2, 1)[:, : k - 1]).any()
        assert np.array_equal(truth, np.argsort(d2, axis=1, kind="stable")[:, :k])


@pytest.mark.parametrize("name", KNN_NAMES)
def test_knn_fast_build_equals_the_fma_reading(oracle, dev, ref_fast, name):
    """`ssd += tmp*tmp` has one possible contraction, ssd = fma(tmp, tmp, ssd): the fast build must equal the oracle's second
    reading and the library's named second definition on every case."""
    x_q, x_r, k, _, want_fma = knn_case(oracle, name)
    Q, R = T(x_q, dev), T(x_r, dev)
    truth = N_(ref_fast.knn(Q, R, k))
    assert np.array_equal(want_fma, truth), f"oracle.knn under contract('fma') differs from the fast build: {name}"
    assert np.array_equal(N_(ops.knn_indices(Q, R, k, contract="fma")), truth), f"ops.knn_indices(contract='fma') differs from the fast build: {name}"
