"""GPU: the fused SGD step (``pcl_sgd_momentum_f32``, csrc/sgd.hip) at the tensor counts, sizes and alignments a real step has,
against the fp64 restatement of tests/sgd_ref.py BIT FOR BIT (the library is built with -ffp-contract=off: every statement is
fp64 arithmetic on fp32 operands and one rounding, which the CPU reproduces exactly -- no tolerance anywhere in this file except
the second witness, torch's own fused kernel, which contracts: one ulp per statement, see ``assert_witness``).

Every tensor of a case is a slice of one of three flat device arenas (p, g, v) filled with a sentinel bit pattern; the start
offset of a slice modulo 4 floats is chosen per tensor and per arena and neighbouring slices are at least one sentinel apart.
After every call: each p / v slice equals the restatement, every float outside the slices still holds its sentinel (both in one
whole-arena comparison of int32 views), and the g arena is unchanged in full.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import sgd_ref as R

pytestmark = pytest.mark.gpu

PCL_EINVAL = -1
MAXT, CHUNK = 96, 4096                                   # csrc/sgd.hip: tensors per launch, elements per block
SENTINEL = (0x5A5A5A5A, 0x4B4B4B4B, 0x3C3C3C3C)          # p, g, v arenas: three different normal fp32 numbers
OFFSETS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (2, 2, 2), (3, 1, 2)]       # (p, g, v) start offsets mod 4 floats
SIZES_FULL = [1, 3, 4, 255, 256, 257, 1023, 1024, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 5, 65536, 1048576]
SIZES_REDUCED = [1, 3, 4, 257, 4095, 4096, 4097, 8193, 3 * 4096 + 5, 65536]
FULL_HYPER = R.HYPER[2]                                  # weight decay AND dampening: the tuple the full sweep and torch's witness run with


class Arenas:
    """Three sentinel-filled fp32 arenas on the device and the tensors of a case as slices of them.  ``numels[i] == 0`` is an empty
    entry: no slice, null pointers.  The host keeps the tensors densely concatenated (``P``, ``G``, ``V``: what the restatement takes)."""

    def __init__(self, dev, numels, offsets, seed):
        assert len(numels) == len(offsets)
        self.dev, self.numels, self.n = dev, list(numels), len(numels)
        self.dense = np.concatenate([[0], np.cumsum(self.numels)]).astype(np.int64)
        self.starts = [[], [], []]
        for a in range(3):
            cursor = 4
            for n, off in zip(self.numels, offsets):
                s = cursor + 1                           # at least one sentinel float after the previous slice
                s += (off[a] - s) % 4
                self.starts[a].append(s if n else -1)
                if n:
                    cursor = s + n
        rng = np.random.default_rng(seed)
        total = int(self.dense[-1])
        # normal numbers only: |x| < 2^-126 has probability ~1e-38 under these scales (drawn in fp64 and rounded: the fp32
        # generator's grid near 0 is coarse enough to hit 0.0 itself among a million draws); a RESULT that is no normal number -- an
        # exact 0 where two terms cancel -- is a property of the pair (state, gradient): ``normal_grad`` redraws such gradient
        # elements, and the callers assert the precondition on the restatement's outputs
        self.P = rng.standard_normal(total).astype(np.float32)
        self.V = (0.25 * rng.standard_normal(total)).astype(np.float32)
        self.G = self.fresh_grad(rng)
        self.rng = rng
        self.redraw = np.random.default_rng(seed + 7919)  # (a stream of its own: a redrawn element does not move any later draw)
        self.host = [self.arena(a, d) for a, d in enumerate((self.P, self.G, self.V))]
        self.device = [torch.from_numpy(h).to(dev) for h in self.host]
        assert all(t.data_ptr() % 16 == 0 for t in self.device)
        self.ptr = [[0 if s < 0 else t.data_ptr() + 4 * s for s in self.starts[a]] for a, t in enumerate(self.device)]
        U64, I64 = ctypes.c_uint64 * max(self.n, 1), ctypes.c_int64 * max(self.n, 1)
        self.tables = [U64(*self.ptr[a]) for a in range(3)]
        self.numel_table = I64(*self.numels)

    def fresh_grad(self, rng=None):
        return (0.5 * (rng or self.rng).standard_normal(int(self.dense[-1]))).astype(np.float32)

    def arena(self, a, dense):
        """The int32 image of arena ``a`` with ``dense`` in its slices and the sentinel everywhere else."""
        h = np.full(self.starts_end(a), SENTINEL[a], np.int32)
        f = h.view(np.float32)
        for i, n in enumerate(self.numels):
            if n:
                s = self.starts[a][i]
                f[s:s + n] = dense[self.dense[i]:self.dense[i + 1]]
        return h

    def starts_end(self, a):
        live = [s + n for s, n in zip(self.starts[a], self.numels) if n]
        return (max(live) if live else 4) + 8

    def gather(self, a, image):
        """The dense fp32 array of the slices of an arena image."""
        f = image.view(np.float32)
        parts = [f[self.starts[a][i]:self.starts[a][i] + n] for i, n in enumerate(self.numels) if n]
        return np.concatenate(parts) if parts else np.empty(0, np.float32)

    def normal_grad(self, hyper, fresh):
        """The gradient of the next call (``fresh``: a new draw) with every element redrawn for which an operand, the intermediate
        gradient or a result of the RESTATEMENT is no normal number under ``hyper`` (decided by the yardstick alone, before the
        library runs).  In practice: the few-in-10^8 elements whose two terms of a statement cancel to an exact 0."""
        G = self.fresh_grad() if fresh else self.G.copy()
        for _ in range(10):
            bad = R.abnormal_elements(self.P, G, self.V, *hyper)
            if not bad.any():
                break
            G[bad] = (0.5 * self.redraw.standard_normal(int(bad.sum()))).astype(np.float32)
        if fresh or not np.array_equal(R.bits(G), R.bits(self.G)):
            self.set_grad(G)

    def set_grad(self, G):
        self.G = G
        self.host[1] = self.arena(1, G)
        self.device[1].copy_(torch.from_numpy(self.host[1]))

    def call(self, lr, mu, wd, damp, tables=None, numel=None):
        """The entry point as ``_LeanFusedSGD.step()`` calls it (host tables of c_uint64 / c_int64) -> return code."""
        from pointcloudlib_amd import _lib
        pa, ga, ba = tables or self.tables
        return _lib.lib().pcl_sgd_momentum_f32(pa, ga, ba, numel or self.numel_table, self.n, float(lr), float(mu), float(wd), float(damp),
                                               torch._C._cuda_getCurrentRawStream(self.dev.index))

    def download(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.device]

    def tensor_of(self, a, j):
        for i, n in enumerate(self.numels):
            if n and self.starts[a][i] <= j < self.starts[a][i] + n:
                return f"tensor {i} (numel {n}, start offsets mod 4 {[self.starts[b][i] % 4 for b in range(3)]}) element {j - self.starts[a][i]}"
        return "a sentinel outside every slice"

    def launches(self):
        return sum(1 for t0 in range(0, self.n, MAXT) if any(self.numels[t0:t0 + MAXT]))


def assert_image(ar, a, got, want, what):
    """Whole-arena comparison of int32 images: slices and sentinels at once.  Where ``want`` is NaN any NaN will do."""
    assert got.shape == want.shape
    nan = np.isnan(want.view(np.float32))
    bad = np.where(nan, ~np.isnan(got.view(np.float32)), got != want)
    if bad.any():
        j = int(np.argmax(bad))
        raise AssertionError(f"{what}: arena {'pgv'[a]}: {int(bad.sum())} floats differ, first at {j} = {ar.tensor_of(a, j)}: "
                             f"got 0x{int(got[j]) & 0xffffffff:08x} ({got.view(np.float32)[j]!r}) want 0x{int(want[j]) & 0xffffffff:08x} "
                             f"({want.view(np.float32)[j]!r})")


def step_and_check(ar, hyper, what, fresh_grad=False, normal=True):
    """One call of the entry point on the arenas' current state, held to the restatement; the host's dense copies move on to the
    restatement's outputs (so consecutive calls compound).  -> the downloaded images."""
    if normal:
        ar.normal_grad(hyper, fresh_grad)
    elif fresh_grad:
        ar.set_grad(ar.fresh_grad())
    p1, v1 = R.sgd_ref(ar.P, ar.G, ar.V, *hyper)
    if normal:
        assert R.all_normal(ar.P, ar.G, ar.V, p1, v1), "test inputs: an operand or a result that is no normal number"
    from pointcloudlib_amd import _lib
    rc = ar.call(*hyper)
    assert rc == 0, _lib.lib().pcl_last_error()
    got = ar.download()
    assert_image(ar, 0, got[0], ar.arena(0, p1), what)
    assert_image(ar, 2, got[2], ar.arena(2, v1), what)
    assert np.array_equal(got[1], ar.host[1]), f"{what}: the gradient arena was written"
    ar.P, ar.V = p1, v1
    return got


def sweep(sizes):
    return [n for n in sizes for _ in OFFSETS], [o for _ in sizes for o in OFFSETS]


# ---------------------------------------------------------------- (a) size x alignment sweep, (d) its second witness

@pytest.fixture(scope="module")
def full_sweep(dev):
    """The full size x alignment sweep, three consecutive calls with a fresh gradient each: run ONCE, nothing asserted here.  Records
    per call the dense inputs as the device held them, the restatement's outputs and the downloaded images."""
    numels, offsets = sweep(SIZES_FULL)
    ar = Arenas(dev, numels, offsets, seed=1)
    calls = []
    for k in range(3):
        ar.normal_grad(FULL_HYPER, fresh=k > 0)
        before = ar.download()
        P, G, V = (ar.gather(a, before[a]) for a in range(3))
        rc = ar.call(*FULL_HYPER)
        after = ar.download()
        calls.append(dict(rc=rc, P=P, G=G, V=V, g_image=ar.host[1], after=after))
        ar.P, ar.V = ar.gather(0, after[0]), ar.gather(2, after[2])      # the state the next gradient is drawn against
    return ar, calls


def test_size_alignment_sweep_three_calls(full_sweep):
    """17 sizes x 7 alignment tuples = 119 tensors in one call (two launches), around every seam of the kernel: below / at / above one
    and two blocks of 4 096, a full block followed by a tail block, hundreds of blocks; all three pointers 16-byte aligned (the
    float4 branch) and each of the three off on its own (the scalar branch).  Three consecutive calls, compared after each."""
    ar, calls = full_sweep
    assert ar.n == 119 and ar.launches() == 2
    al16 = [all(ar.ptr[a][i] % 16 == 0 for a in range(3)) for i in range(ar.n)]
    assert any(al and n >= CHUNK for al, n in zip(al16, ar.numels)), "no 16-byte-aligned tensor with a full block: the float4 branch never runs"
    assert any(not al and n >= CHUNK for al, n in zip(al16, ar.numels)), "no misaligned tensor with a full block"
    for a in range(3):                                   # each pointer is the only misaligned one of some tensor with a full block
        assert any(n >= CHUNK and [ar.ptr[b][i] % 16 != 0 for b in range(3)] == [b == a for b in range(3)] for i, n in enumerate(ar.numels))
    P, V = calls[0]["P"], calls[0]["V"]
    for k, c in enumerate(calls):
        what = f"call {k + 1} of 3"
        assert c["rc"] == 0, what
        assert np.array_equal(R.bits(c["P"]), R.bits(P)) and np.array_equal(R.bits(c["V"]), R.bits(V))   # the chain starts where the last call ended
        p1, v1 = R.sgd_ref(P, c["G"], V, *FULL_HYPER)
        assert R.all_normal(P, c["G"], V, p1, v1), "test inputs: an operand or a result that is no normal number"
        assert_image(ar, 0, c["after"][0], ar.arena(0, p1), what)
        assert_image(ar, 2, c["after"][2], ar.arena(2, v1), what)
        assert np.array_equal(c["after"][1], c["g_image"]), f"{what}: the gradient arena was written"
        assert not np.array_equal(p1, P) and not np.array_equal(v1, V)
        P, V = p1, v1


def torch_fused(dev, numels, P, G, V, hyper):
    """torch's multi-tensor fused SGD on aligned contiguous clones of the same tensors -> dense (p, v)."""
    lr, mu, wd, damp = hyper
    bounds = np.concatenate([[0], np.cumsum(numels)])
    lists = []
    for d in (P, G, V):
        t = torch.from_numpy(d).to(dev)
        lists.append([t[bounds[i]:bounds[i + 1]].clone() for i in range(len(numels))])
    ps, gs, vs = lists
    g_before = [x.clone() for x in gs]
    assert all(x.data_ptr() % 16 == 0 and x.is_contiguous() for l in lists for x in l)
    torch._fused_sgd_(ps, gs, vs, weight_decay=wd, momentum=mu, lr=lr, dampening=damp, nesterov=False, maximize=False,
                      is_first_step=False, grad_scale=None, found_inf=None)
    assert all(torch.equal(a, b) for a, b in zip(gs, g_before))
    return torch.cat(ps).cpu().numpy(), torch.cat(vs).cpu().numpy()


def assert_witness(what, hyper, p_in, lib_p, lib_v, t_p, t_v, g_in=None, v_in=None):
    """torch's fused kernel as a second witness, statement by statement, each within ONE fp32 ulp.

    The library equals the fp64 restatement bit for bit (asserted elsewhere in this file).  torch's kernel is built by others with
    floating-point contraction on: its second and third statements are fp64 fused multiply-adds, v = fma(mu, v, c * g) and
    p = fma(-lr, v, p) (verified offline on every differing element of a run, with exact rational arithmetic), which moves the fp64
    value by one unit in ITS last place and the fp32 result by one ulp where the value sits within ~2e-9 ulp of a rounding
    boundary.  That is common when mu == 1 - dampening (0.9 * (v + g): the sum of two fp32 numbers has few bits) and never seen
    with dampening = 0 and lr = 0.02, the drivers' setting.  So: torch's v is within one ulp of the library's, and torch's p is within
    one ulp of the restatement's third statement applied to torch's OWN v.  (End to end torch's p is further from the library's
    where |p| << lr * ulp(v): its one-ulp-different v enters its p.  Full sweep, first call, hyper-parameters (0.05, 0.9, 1e-3, 0.1):
    13 544 of 16 325 288 elements of p and v differ, v by 1 ulp, p by up to 205 ulp end to end.)  Prints the counts.

    Figures of an MI355X run, calls 1 / 2 / 3 of 8 162 644 elements: v differs in 12 509 / 15 706 / 16 838, p's statement in
    371 / 429 / 460, each by exactly 1 ulp; the four networks (dampening 0, lr 0.02): 0 differing elements of 34.6 M each of p and v.
    One ulp says nothing where the two terms of a statement cancel to an exact 0 (mu == 1 - dampening, v == -g: 0 here, the fp64
    rounding residue of one product there, ~1e-18): such an element is no normal number and the tests' inputs exclude it
    (``Arenas.normal_grad``), as they exclude subnormals.

    A network's own gradients cannot be redrawn, and they do hold such elements: the gradients of parameters that have none in
    theory are rounding noise, small integers times one quantum, where v = 10 q meets g = -9 q (one element of PointConv cls's
    19.6 M in one run of four).  With ``g_in`` / ``v_in`` given, the elements whose restated v or p is no normal number although its
    terms are not both 0 are held to the reach of contraction instead of to one ulp: torch's fused multiply-add skips the rounding
    of one fp64 product, so |difference| <= 2^-52 (|term 1| + |term 2|) of the statement.  Their count is printed."""
    lr, mu, wd, damp = (float(x) for x in hyper)
    p_from_tv = (p_in.astype(np.float64) - lr * t_v.astype(np.float64)).astype(np.float32)
    if g_in is not None:
        g1 = g_in if wd == 0.0 else (g_in.astype(np.float64) + wd * p_in.astype(np.float64)).astype(np.float32)
        terms_v = np.abs(mu * v_in.astype(np.float64)) + np.abs((1.0 - damp) * g1.astype(np.float64))
        terms_p = np.abs(p_in.astype(np.float64)) + np.abs(lr * t_v.astype(np.float64))
        out_v = ~R.normal_mask(lib_v) & (terms_v != 0)
        out_p = ~R.normal_mask(p_from_tv) & (terms_p != 0)
        print(f"torch witness, {what}: {int(out_v.sum())} elements of v and {int(out_p.sum())} of p cancel to no normal number: held to 2^-52 of their terms")
        assert np.all(np.abs(lib_v[out_v].astype(np.float64) - t_v[out_v]) <= 2.0 ** -52 * terms_v[out_v]), what
        assert np.all(np.abs(p_from_tv[out_p].astype(np.float64) - t_p[out_p]) <= 2.0 ** -52 * terms_p[out_p]), what
        keep = ~(out_v | out_p)
        p_in, lib_p, lib_v, t_p, t_v, p_from_tv = (a[keep] for a in (p_in, lib_p, lib_v, t_p, t_v, p_from_tv))
    dv = R.ulp_distance(lib_v, t_v)
    dp = R.ulp_distance(p_from_tv, t_p)
    end_to_end = R.ulp_distance(lib_p, t_p)
    print(f"torch witness, {what}: {dv.size} elements each of p and v; v differs from torch.optim.SGD(fused=True) in {int((dv != 0).sum())} "
          f"(largest {int(dv.max())} ulp), p's statement on torch's v in {int((dp != 0).sum())} (largest {int(dp.max())} ulp), "
          f"p end to end in {int((end_to_end != 0).sum())} (largest {int(end_to_end.max())} ulp)")
    assert dv.max() <= 1, f"{what}: torch's momentum buffer is {int(dv.max())} ulp from the library's"
    assert dp.max() <= 1, f"{what}: torch's parameter is {int(dp.max())} ulp from p - lr * (torch's v)"
    same_v = dv == 0
    assert R.ulp_distance(lib_p[same_v], t_p[same_v]).max() <= 1


def test_torch_fused_sgd_is_a_second_witness(dev, full_sweep):
    """The inputs of each call of the full sweep through ``torch._fused_sgd_`` (aligned contiguous clones: torch takes nothing
    else): every statement within one fp32 ulp of the library, see ``assert_witness``."""
    ar, calls = full_sweep
    live = [n for n in ar.numels if n]
    for k, c in enumerate(calls):
        t_p, t_v = torch_fused(dev, live, c["P"], c["G"], c["V"], FULL_HYPER)
        lib_p, lib_v = ar.gather(0, c["after"][0]), ar.gather(2, c["after"][2])
        assert_witness(f"call {k + 1} of 3", FULL_HYPER, c["P"], lib_p, lib_v, t_p, t_v)


# ---------------------------------------------------------------- (c) hyper-parameters

@pytest.mark.parametrize("hyper", R.HYPER, ids=lambda h: "lr{}-mu{}-wd{}-damp{}".format(*h))
def test_hyper_parameters(dev, hyper):
    """Every (lr, momentum, weight_decay, dampening) tuple on the reduced sweep (10 sizes x 7 alignment tuples, every seam of the
    full one up to 16 blocks): weight decay on and off, dampening, no momentum, lr = 0.  Two consecutive calls."""
    numels, offsets = sweep(SIZES_REDUCED)
    ar = Arenas(dev, numels, offsets, seed=2)
    p0 = ar.host[0].copy()
    for k in range(2):
        got = step_and_check(ar, hyper, f"{hyper} call {k + 1}", fresh_grad=k > 0)
        if hyper[0] == 0.0:
            assert np.array_equal(got[0], p0), "lr = 0 moved a parameter"
        else:
            assert not np.array_equal(got[0], p0)


# ---------------------------------------------------------------- (b) table counts, empty entries

def cycling_sizes(n):
    return [1 + (i * 619) % 5000 for i in range(n)]      # 619 and 5000 are coprime: walks 1 ... 5000, ~18 % of the tensors span two blocks


@pytest.mark.parametrize("n_tensors,empty", [(1, ()), (1, (0,)), (95, (0, 94)), (96, (0, 95)), (97, (0, 95, 96)), (192, (0, 95, 96, 191)),
                                             (193, (0, 95, 96, 192)), (200, tuple(range(96, 192)))],
                         ids=["1", "1-empty", "95", "96", "97", "192", "193", "200-chunk-96..191-empty"])
def test_table_counts_and_empty_entries(dev, n_tensors, empty):
    """One, two and three launches with the table full to the brim and one past it; ``numel == 0`` entries (null pointers: skipped
    before the pointers are looked at) at the head, on both sides of the seam between two tables and at the tail, which shift the
    kernel's table index against the caller's; and a whole table of 96 empty entries between two live ones."""
    numels = cycling_sizes(n_tensors)
    for i in empty:
        numels[i] = 0
    ar = Arenas(dev, numels, [OFFSETS[i % len(OFFSETS)] for i in range(n_tensors)], seed=3 + n_tensors)
    assert all(ar.ptr[a][i] == 0 for a in range(3) for i in empty)
    hyper = R.HYPER[1]
    for k in range(2):
        step_and_check(ar, hyper, f"{n_tensors} tensors call {k + 1}", fresh_grad=k > 0)


# ---------------------------------------------------------------- non-finite gradients

def test_non_finite_gradients_stay_where_they_are(dev):
    """inf / nan in a few elements of g (scalar branch, float4 branch, a tail block): exactly those elements of p and v become
    non-finite, as in the restatement; their neighbours in the same float4 do not."""
    numels, offsets = [5, 4096 + 7, 8192, 300], [(0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 2, 3)]
    ar = Arenas(dev, numels, offsets, seed=4)
    hyper = R.HYPER[1]
    ar.normal_grad(hyper, fresh=False)
    G = ar.G.copy()
    where = {0: [(2, np.inf)], 1: [(0, np.nan), (1029, -np.inf), (4095, np.inf), (4096 + 6, np.nan)], 2: [(4097, np.inf), (8191, -np.nan)],
             3: [(299, -np.inf)]}
    hit = []
    for i, lst in where.items():
        for e, val in lst:
            G[ar.dense[i] + e] = val
            hit.append(int(ar.dense[i] + e))
    ar.set_grad(G)
    p1, v1 = R.sgd_ref(ar.P, ar.G, ar.V, *hyper)
    bad = np.zeros(len(G), bool)
    bad[hit] = True
    assert np.array_equal(~np.isfinite(p1), bad) and np.array_equal(~np.isfinite(v1), bad)      # the restatement itself
    assert R.all_normal(p1[~bad], v1[~bad])
    got = step_and_check(ar, hyper, "non-finite g", normal=False)
    assert np.array_equal(~np.isfinite(ar.gather(0, got[0])), bad) and np.array_equal(~np.isfinite(ar.gather(2, got[2])), bad)


# ---------------------------------------------------------------- a rejected table updates nothing

@pytest.mark.parametrize("kind", ["negative_numel", "null_grad"])
def test_rejected_table_is_not_half_applied(dev, kind):
    """100 live tensors, entry 98 bad (the second table of 96): PCL_EINVAL naming tensor 98, and NOTHING updated -- the whole table
    is validated before the first launch (the first 96 tensors used to be updated before the call failed).  The bad entry is
    rejected on the host; it never reaches a kernel."""
    from pointcloudlib_amd import _lib
    n = 100
    ar = Arenas(dev, cycling_sizes(n), [OFFSETS[i % len(OFFSETS)] for i in range(n)], seed=5)
    tables = [type(t)(*t) for t in ar.tables]
    numel = type(ar.numel_table)(*ar.numel_table)
    if kind == "negative_numel":
        numel[98] = -1
    else:
        tables[1][98] = 0
    rc = ar.call(*R.HYPER[1], tables=tables, numel=numel)
    assert rc == PCL_EINVAL
    assert "tensor 98:" in _lib.lib().pcl_last_error().decode()
    got = ar.download()
    for a in range(3):
        assert_image(ar, a, got[a], ar.host[a], f"rejected table ({kind})")
    step_and_check(ar, R.HYPER[1], "the same arenas with the table mended")      # (the arenas and the other 99 entries were fine)


# ---------------------------------------------------------------- the optimiser on the networks' own gradients

def census(pa, ga, ba, na, n):
    """Which kernel branches a real step takes: launches, blocks (of them on the float4 branch), pointers off 16 bytes."""
    live = [i for i in range(n) if na[i]]
    blocks = sum(-(-na[i] // CHUNK) for i in live)
    al = {i: (pa[i] | ga[i] | ba[i]) % 16 == 0 for i in live}
    vec = sum(na[i] // CHUNK for i in live if al[i])
    return dict(tensors=n, launches=sum(1 for t0 in range(0, n, MAXT) if any(na[i] for i in range(t0, min(n, t0 + MAXT)))), blocks=blocks,
                float4_blocks=vec, elements=sum(na[i] for i in live), largest=max(na[i] for i in live),
                grads_off_16=sum(1 for i in live if ga[i] % 16), params_off_16=sum(1 for i in live if pa[i] % 16),
                bufs_off_16=sum(1 for i in live if ba[i] % 16), numel_not_multiple_of_4=sum(1 for i in live if na[i] % 4))


def _nets(dev):
    from pointcloudlib_amd import synth

    def cloud(B, N, seed):
        return torch.from_numpy(synth.gauss_ball(B, N, seed)).to(dev)

    def onehot(B):
        oh = torch.zeros(B, 16, device=dev)
        oh[torch.arange(B), torch.arange(B) % 16] = 1
        return oh

    def pointnet():
        from pointcloudlib_amd.networks.cls.pointnet import PointNet
        return PointNet(), (cloud(4, 2048, 5).transpose(1, 2).contiguous(),)

    def pointnet2_msg_partseg():
        from pointcloudlib_amd.networks.seg.pointnet2_partseg import PointNetMSG
        x = cloud(4, 2048, 5)
        return PointNetMSG(), (x, x, onehot(4))

    def pointconv():
        from pointcloudlib_amd.networks.cls.pointconv import PointConvDensityClsSsg
        st = [torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)]
        return PointConvDensityClsSsg(), (cloud(4, 512, 8).transpose(1, 2).contiguous(), st)

    def pointconv_partseg():
        from pointcloudlib_amd.networks.seg.pointconv_partseg import PointConvDensity_partseg
        return PointConvDensity_partseg(), (cloud(4, 2048, 9), onehot(4))

    return {"pointnet_cls": (pointnet, 0.0, 0), "pointnet2_msg_partseg": (pointnet2_msg_partseg, 1e-4, 0),
            "pointconv_cls": (pointconv, 0.0, 130), "pointconv_partseg": (pointconv_partseg, 1e-4, 314)}


@pytest.mark.parametrize("name", ["pointnet_cls", "pointnet2_msg_partseg", "pointconv_cls", "pointconv_partseg"])
def test_optimiser_step_on_a_networks_own_gradients(dev, monkeypatch, name):
    """``make_sgd(net.parameters())`` at the batch and point counts of tests/test_networks_gpu.py: the second ``step()`` is ONE call of
    the library's kernel and none of torch's, every parameter and momentum buffer afterwards equals the restatement of the
    snapshot taken before it bit for bit, the gradients are untouched, and a deep copy of the network driven by
    ``torch.optim.SGD(fused=True)`` with cloned gradients ends within one ulp per statement (``assert_witness``; 0
    differing elements on all four networks but for one exactly cancelling element of PointConv cls in one run of four).  Prints the census of DESIGN.md 10.8."""
    from pointcloudlib_amd import _lib
    from pointcloudlib_amd.train_utils import make_sgd
    make, wd, n_expected = _nets(dev)[name]
    torch.manual_seed(21)
    net, args = make()
    net = net.to(dev).train()
    twin = copy.deepcopy(net)
    lr, mu = 0.02, 0.9
    params, twins = list(net.parameters()), list(twin.parameters())
    opt = make_sgd(params, lr=lr, momentum=mu, weight_decay=wd)
    assert type(opt).__name__ == "_LeanFusedSGD"
    witness = torch.optim.SGD(twins, lr=lr, momentum=mu, weight_decay=wd, fused=True)
    if n_expected:
        assert len(params) == n_expected > MAXT

    def forward_backward():
        for p in params:
            p.grad = None
        net(*args).square().mean().backward()
        for p, q in zip(params, twins):
            q.grad = p.grad.detach().clone()

    forward_backward()
    opt.step(); witness.step()                           # torch creates the momentum buffers on this step
    forward_backward()
    bufs = [opt.state[p]["momentum_buffer"] for p in params]
    snap = [[t.detach().cpu().numpy().ravel().copy() for t in ts] for ts in (params, [p.grad for p in params], bufs)]

    seen = {"own": [], "torch": 0}
    real_call, real_fused = _lib.call, torch._fused_sgd_

    def counting_call(fn, *a, **kw):
        if fn == "pcl_sgd_momentum_f32":
            seen["own"].append([list(a[0]), list(a[1]), list(a[2]), list(a[3]), a[4]])
        return real_call(fn, *a, **kw)

    def counting_fused(*a, **kw):
        seen["torch"] += 1
        return real_fused(*a, **kw)

    with monkeypatch.context() as m:
        m.setattr(_lib, "call", counting_call)
        m.setattr(torch, "_fused_sgd_", counting_fused)
        opt.step()
    assert len(seen["own"]) == 1 and seen["torch"] == 0, (len(seen["own"]), seen["torch"])
    witness.step()
    torch.cuda.synchronize()
    print(f"census {name}: {census(*seen['own'][0])}")
    assert seen["own"][0][4] == len(params)

    sizes = [p.numel() for p in params]
    P, G, V = (np.concatenate(s) for s in snap)
    p1, v1 = R.sgd_ref(P, G, V, lr, mu, wd, 0.0)
    got_p = np.concatenate([p.detach().cpu().numpy().ravel() for p in params])
    got_v = np.concatenate([opt.state[p]["momentum_buffer"].cpu().numpy().ravel() for p in params])
    got_g = np.concatenate([p.grad.cpu().numpy().ravel() for p in params])
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    names = [k for k, _ in net.named_parameters()]

    def where(got, want):
        bad = np.flatnonzero(np.where(np.isnan(want), ~np.isnan(got), R.bits(got) != R.bits(want)))
        i = int(np.searchsorted(bounds, bad[0], "right") - 1)
        return f"{bad.size} elements differ, first in {names[i]} (numel {sizes[i]}) at {bad[0] - bounds[i]}: got {got[bad[0]]!r} want {want[bad[0]]!r}"

    assert np.array_equal(R.bits(got_g), R.bits(G)), "the step wrote a gradient"
    assert R.same_bits(got_p, p1), where(got_p, p1)
    assert R.same_bits(got_v, v1), where(got_v, v1)
    assert not np.array_equal(got_p, P)
    t_p = np.concatenate([q.detach().cpu().numpy().ravel() for q in twins])
    t_v = np.concatenate([witness.state[q]["momentum_buffer"].cpu().numpy().ravel() for q in twins])
    assert_witness(name, (lr, mu, wd, 0.0), P, got_p, got_v, t_p, t_v, g_in=G, v_in=V)
