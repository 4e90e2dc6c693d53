"""The inputs on which the reference's own kernels (oracle/ref_kernels.py) are compared with the oracle and the HIP library.

Test infrastructure only; NumPy only.  Shared by tests/test_reference_kernels_gpu.py, tools/gen_reference_golden.py and
tests/test_reference_golden_cpu.py so that the recorded fixture and the live comparison are about the same clouds.  Every
shape is the smallest that still reaches the rule it is there for; each rule is named at its case.
"""
import hashlib

import numpy as np

from pointcloudlib_amd import synth

F = np.float32
FPS_BLOCKS = (1, 2, 8, 64, 512)            # 512 is the largest block the kernel's reduction tree covers; N < 512 in every case
BQ_RADII = (0.2, 0.5)
BQ_NSAMPLES = (1, 8, 64)
SKIP = 1e-3                                 # the double literal of `mag <= 1e-3`
SKIP_F32 = F(1e-3)                          # the nearest float: 0.001000000047..., greater than the literal


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def lattice_cloud(B, N, seed, C=3):
    """Coordinates are multiples of 0.25 in [-0.5, 0.5] (125 sites for C = 3) and every site occurs at least twice -- the
    construction of test_three_nn_ties_across_the_lane_split.  Every difference, product and sum of the distance expressions
    is exact in fp32, so distances tie exactly and do not depend on how a compiler contracts them."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-2, 3, size=(B, N, C)).astype(F) * F(0.25)
    p[:, N // 2:] = p[:, : N - N // 2]
    return p


def sqnorm_f32(p):
    """(x*x) + (y*y) + (z*z), every operation rounded to fp32, as the source writes `mag`."""
    p = np.asarray(p, F)
    return (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]


def boundary_pair():
    """Two points (0.02, y, 0): the first has fp32 squared norm exactly float32(1e-3), which is GREATER than the double 1e-3, so
    the kernel's `mag <= 1e-3` (float against a double literal) keeps it; the second is the nearest y below whose squared norm
    is the next float down, less than 1e-3: skipped.  A float-against-float comparison would skip both."""
    x = F(0.02)
    y0 = np.sqrt(F(SKIP_F32 - x * x), dtype=F)
    ys = [y0]
    up, dn = y0, y0
    for _ in range(2000):
        up, dn = np.nextafter(up, F(1)), np.nextafter(dn, F(0))
        ys += [up, dn]
    ys = np.array(sorted(ys), F)
    mag = sqnorm_f32(np.stack([np.full_like(ys, x), ys, np.zeros_like(ys)], -1))
    on = np.flatnonzero(mag == SKIP_F32)
    assert len(on), "no y with fl(0.02^2 + y^2) == float32(1e-3) within 2000 ulp"
    keep = ys[on[0]]
    below = ys[on[0] - 1]
    assert on[0] > 0 and float(mag[on[0] - 1]) < SKIP < float(mag[on[0]])
    return np.array([x, keep, 0], F), np.array([x, below, 0], F)


def fps_cases():
    """name -> (xyz [B,N,3], m).  Each is run at every block size of FPS_BLOCKS."""
    out = {}
    # plain clouds; N = 37 is below two of the block sizes (threads without a point hold best = -1, besti = 0)
    out["plain300"] = (synth.gauss_ball(3, 300, 4101), 150)
    out["plain37"] = (synth.gauss_ball(2, 37, 4102), 18)
    # ties: m = N on a cloud of at most 125 sites, each at least twice -- once the sites are used up every step is a tie at
    # distance 0 between all live points, decided by the block reduction's order alone
    out["lattice100"] = (lattice_cloud(2, 100, 4103), 100)
    out["lattice257"] = (lattice_cloud(2, 257, 4104), 257)
    # skipped points: m = N, so every live point is picked before the picks degenerate
    p = synth.gauss_ball(4, 64, 4105)
    rng = np.random.default_rng(4106)
    dead = rng.standard_normal((4, 64, 3)).astype(F)
    dead *= (rng.uniform(0.001, 0.03, (4, 64, 1)) / np.linalg.norm(dead, axis=-1, keepdims=True)).astype(F)
    sel = rng.random((4, 64)) < 0.3
    sel[0, 0] = sel[1, 0] = True                   # point 0 is dead and still the first pick
    sel[1, 1:] &= rng.random(63) < 0.5
    sel[2, 0] = False
    sel[3, :] = True                               # a cloud with no live point at all: every pick is 0
    p[sel] = dead[sel]
    keep, below = boundary_pair()
    p[0, 5], p[0, 6] = keep, below                 # see boundary_pair
    p[2, 40], p[2, 41] = below, keep
    out["skips64"] = (p, 64)
    # running distances capped by the 1e10 start value: coordinates up to ~2e5, squared distances up to ~1e11
    out["capped128"] = (synth.gauss_ball(2, 128, 4107) * F(2e5), 64)
    return out


SKIPS_BOUNDARY = {"kept": [(0, 5), (2, 41)], "skipped": [(0, 6), (2, 40)]}      # (cloud, index) of boundary_pair's points


def bq_cases(oracle):
    """name -> (new_xyz [B,m,3], xyz [B,N,3], radii, n_hitless).  Each is run at every nsample of BQ_NSAMPLES.  The last
    ``n_hitless`` queries of every cloud have no point within any radius; no other query of any case is without a hit."""
    out = {}
    # queries are FPS centres -> cloud points -> every row has a hit; dense enough that small lists saturate, large do not
    xyz = synth.gauss_ball(3, 300, 4201)
    q = oracle.fps(xyz, 64, block_size=1, return_xyz=True)[1]
    out["saturation"] = (q, xyz, BQ_RADII, 0)
    # lattice, radius 0.5: neighbours at exactly two lattice steps have d2 = 0.25 = fl(0.5*0.5) and the strict `<` excludes them
    lat = lattice_cloud(2, 100, 4202)
    out["exact_radius"] = (np.ascontiguousarray(lat[:, :32]), lat, (0.5,), 0)
    # rows the reference leaves unwritten: 4 queries far outside the cloud
    xyz = synth.gauss_ball(2, 200, 4203)
    q = oracle.fps(xyz, 28, block_size=1, return_xyz=True)[1]
    far = q[:, :4] + F(10.0)
    out["hitless"] = (np.ascontiguousarray(np.concatenate([q, far], 1)), xyz, BQ_RADII, 4)
    # off the lattice: around a centre at the origin, points at exactly float32(r) along an axis have d2 = fl(r*r) = radius2 and
    # are excluded; the next float inside is included.  0.2 is the network's radius, where fl(r*r) lies above the exact square;
    # at 0.3 it lies below, so a radius2 kept in double would include the point: RIM_RADII adds that radius for this case alone
    xyz = synth.gauss_ball(2, 64, 4204)
    xyz[:, 0] = 0
    for i, r in enumerate(RIM_RADII):
        xyz[:, RIM_ON[i][0]] = (F(r), 0, 0)
        xyz[:, RIM_ON[i][1]] = (0, -F(r), 0)
        xyz[:, RIM_INSIDE[i]] = (0, 0, np.nextafter(F(r), F(0)))
    out["rim"] = (np.ascontiguousarray(xyz[:, :8]), xyz, RIM_RADII, 0)
    return out


RIM_RADII = (0.2, 0.3)
RIM_ON = ((1, 2), (4, 5))            # per radius: indices of the points at d2 == fl(r*r) from query 0
RIM_INSIDE = (3, 6)                  # per radius: index of the point one float inside


# (B, C, Nr, Nq, k); queries are the first Nq references (distance 0 to themselves)
KNN_SHAPES = [
    (2, 3, 64, 64, 5),
    (2, 5, 33, 20, 33),            # k = Nr
    (1, 7, 100, 37, 1),
    (2, 64, 257, 130, 20),
    (1, 130, 300, 50, 7),          # channel tail past a 16-block
    (1, 3, 5000, 70, 9),           # the library's two-pass path
]


def knn_name(shape):
    return "B%d_C%d_Nr%d_Nq%d_k%d" % tuple(shape)


def knn_seed(shape):
    B, C, Nr, Nq, k = shape
    return 4300 + Nr + C


def knn_inputs(shape):
    """(x_q [B,C,Nq], x_r [B,C,Nr]) of one row of KNN_SHAPES, from its seed."""
    B, C, Nr, Nq, k = shape
    r = np.random.default_rng(knn_seed(shape)).standard_normal((B, C, Nr)).astype(F)
    return np.ascontiguousarray(r[:, :, :Nq]), r


def knn_tie_cases():
    """name -> (x_q, x_r, k): lattice features with repeated points (exact ties between different references, stable order: the
    lower index first) and an all-zero cloud (every distance 0: the list is 0..k-1)."""
    lat = np.ascontiguousarray(lattice_cloud(2, 100, 4310).transpose(0, 2, 1))          # [2,3,100]
    z = np.zeros((1, 4, 100), F)
    return {"lattice": (np.ascontiguousarray(lat[:, :, 10:50]), lat, 10),
            "lattice_kNr": (np.ascontiguousarray(lat[:, :, :7]), lat, 100),
            "zeros": (np.ascontiguousarray(z[:, :, :3]), z, 100)}


def knn_cases(with_two_pass=True):
    """name -> (x_q, x_r, k), the rows of KNN_SHAPES (without the Nr = 5000 one on request) and the tie cases."""
    out = {}
    for s in KNN_SHAPES:
        if s[2] > 4096 and not with_two_pass:
            continue
        q, r = knn_inputs(s)
        out[knn_name(s)] = (q, r, s[4])
    out.update(knn_tie_cases())
    return out
