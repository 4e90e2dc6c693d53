"""Ragged batches (``lengths=``) of the index producers on the GPU: FPS, ball query (single and multi-radius), 3-NN.

Truth for cloud b is the CPU oracle on ``x[b:b+1, :n_b]`` with the SAME explicit ``tie_stride`` as the batch call, and as a second
witness the existing dense kernel on that slice.  Everything is integer or bit equality.  Pad rows are filled three ways (copies of
the cloud's own points, NaN, 1e30) and the results must not depend on the filling."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FILLS = ("copies", "nan", "huge")
# the recipe checked with the oracle on the CPU: gauss_ball(6, 1024, 7), 512 samples, tie stride 4, radius 0.2, 64 per group
RECIPE_LENGTHS = [1024, 1000, 777, 640, 513, 512]
TIE = 4


def _fill(x, lengths, how):
    """x [B,N,3] (numpy, every row real) -> a copy whose rows from lengths[b] on are pad rows."""
    out = x.copy()
    N = x.shape[1]
    for b, n in enumerate(lengths):
        k = N - n
        if k == 0:
            continue
        if how == "copies":          # x[b, n:] = x[b, :N - n][::-1] where N - n <= n; cycled through the cloud's own points beyond
            out[b, n:] = x[b, :k][::-1] if k <= n else np.resize(x[b, :n][::-1], (k, 3))
        elif how == "nan":
            out[b, n:] = np.nan
        else:
            out[b, n:] = 1e30
    return out


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _lengths_for(N, m):
    """N, m exactly, m + 1, and values that are multiples neither of 64 nor of any FPS threads-per-cloud."""
    out = [N, m, m + 1, N - 37, (N + m) // 2 | 1, N - 1]
    assert all(m <= v <= N for v in out) and any(v % 64 for v in out)
    return out


def _clouds(B, N, seed, lattice_cloud=None):
    from pointcloudlib_amd import synth
    x = synth.gauss_ball(B, N, seed)
    if lattice_cloud is not None:        # lattice-quantised: many exact distance ties and duplicates (the adversarial tie case)
        x[lattice_cloud] = np.round(x[lattice_cloud] * 8.0) / 8.0 + np.float32(0.0625)
    return x


# ------------------------------------------------------------------------------------------------------------------ FPS
# one wave per cloud (N <= 512), four waves (1024, 2048, 4096), the LDS-resident kernel (N > 8192, modest m)
@pytest.mark.parametrize("N,m", [(512, 128), (1024, 512), (2048, 512), (4096, 256), (9000, 48)])
def test_fps_ragged_equals_every_cloud_alone(dev, oracle, N, m):
    from pointcloudlib_amd.misc import ops
    lengths = _lengths_for(N, m)
    B = len(lengths)
    x = _clouds(B, N, 7, lattice_cloud=3)
    got = {}
    for how in FILLS:
        xp = torch.from_numpy(_fill(x, lengths, how)).to(dev)
        idx, new_xyz = ops.furthest_point_sample(xp, m, tie_stride=TIE, lengths=lengths)
        got[how] = (idx.cpu().numpy(), _bits(new_xyz))
    for how in FILLS[1:]:                                               # pad invariance
        assert np.array_equal(got[how][0], got["copies"][0]) and np.array_equal(got[how][1], got["copies"][1]), how
    idx, nx = got["copies"]
    for b, n in enumerate(lengths):
        assert idx[b].min() >= 0 and idx[b].max() < n, f"cloud {b}: an index beyond its {n} points"
        want_idx, want_xyz = oracle.fps(x[b:b + 1, :n], m, block_size=TIE, return_xyz=True)
        assert np.array_equal(idx[b], want_idx[0]), f"cloud {b} (n={n}): differs from the oracle on the cloud alone"
        assert np.array_equal(nx[b], want_xyz[0].view(np.int32))
        d_idx, d_xyz = ops.furthest_point_sample(torch.from_numpy(x[b:b + 1, :n].copy()).to(dev), m, tie_stride=TIE)
        assert np.array_equal(idx[b], d_idx.cpu().numpy()[0]) and np.array_equal(nx[b], _bits(d_xyz)[0]), f"cloud {b}: dense kernel"
    # a device tensor gives what the list gives; lengths = [N] * B is the dense entry point, bitwise
    xp = torch.from_numpy(_fill(x, lengths, "nan")).to(dev)
    t_idx, t_xyz = ops.furthest_point_sample(xp, m, tie_stride=TIE, lengths=torch.tensor(lengths, dtype=torch.int32, device=dev))
    assert np.array_equal(t_idx.cpu().numpy(), idx) and np.array_equal(_bits(t_xyz), nx)
    xd = torch.from_numpy(x).to(dev)
    f_idx, f_xyz = ops.furthest_point_sample(xd, m, tie_stride=TIE, lengths=[N] * B)
    d_idx, d_xyz = ops.furthest_point_sample(xd, m, tie_stride=TIE)
    assert torch.equal(f_idx, d_idx) and np.array_equal(_bits(f_xyz), _bits(d_xyz))


def test_fps_ragged_other_strides_start_indices_and_the_c_abi(dev, oracle):
    """Tie strides 1 and 16, the near-origin skip off, caller-supplied start indices -- through the C ABI directly."""
    from pointcloudlib_amd import _lib
    N, m = 1024, 300
    lengths = _lengths_for(N, m)
    B = len(lengths)
    x = _clouds(B, N, 11, lattice_cloud=1)
    x[2, :50] *= 0.01                                                   # near-origin points: skipped with the rule on
    start = np.array([n - 1 if b % 2 else n // 3 for b, n in enumerate(lengths)], np.int32)
    nv = torch.tensor(lengths, dtype=torch.int32, device=dev)
    st = torch.from_numpy(start).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    for S, thr in ((1, 1e-3), (16, -1.0)):
        res = []
        for how in FILLS:
            xp = torch.from_numpy(_fill(x, lengths, how)).to(dev)
            idx = torch.full((B, m), -7, dtype=torch.int32, device=dev)
            nx = torch.empty(B, m, 3, device=dev)
            _lib.call("pcl_fps_ragged_f32", xp.data_ptr(), nv.data_ptr(), B, N, m, S, thr, st.data_ptr(), idx.data_ptr(), nx.data_ptr(), stream)
            res.append((idx.cpu().numpy(), _bits(nx)))
        assert all(np.array_equal(r[0], res[0][0]) and np.array_equal(r[1], res[0][1]) for r in res[1:])
        for b, n in enumerate(lengths):
            w_idx, w_xyz = oracle.fps(x[b:b + 1, :n], m, block_size=S, skip=thr > 0, start_idx=start[b:b + 1], return_xyz=True)
            assert np.array_equal(res[0][0][b], w_idx[0]) and np.array_equal(res[0][1][b], w_xyz[0].view(np.int32)), (S, b)
            assert res[0][0][b].max() < n


def test_fps_and_ball_query_recipe_is_sensitive_to_padding(dev, oracle):
    """The conditions that keep the tests above from passing vacuously, on the recipe verified with the oracle: with copy padding the
    DENSE op on the padded batch differs from the ragged result for every short cloud; some ball-query groups are full, some are
    not, and some are partial only because the pad rows are excluded."""
    from pointcloudlib_amd.misc import ops
    N, m, r, ns = 1024, 512, 0.2, 64
    lengths = RECIPE_LENGTHS
    x = _clouds(len(lengths), N, 7)
    xp = torch.from_numpy(_fill(x, lengths, "copies")).to(dev)
    r_idx, r_xyz = ops.furthest_point_sample(xp, m, tie_stride=TIE, lengths=lengths)
    d_idx, _ = ops.furthest_point_sample(xp, m, tie_stride=TIE)
    r_bq, r_cnt = ops.ball_query(r_xyz, xp, r, ns, return_cnt=True, lengths=lengths)
    d_bq, d_cnt = ops.ball_query(r_xyz, xp, r, ns, return_cnt=True)
    for b, n in enumerate(lengths):
        if n < N:
            assert not torch.equal(r_idx[b], d_idx[b]), f"FPS, cloud {b}: padding with copies changes nothing -- the test shows nothing"
            assert not torch.equal(r_bq[b], d_bq[b]), f"ball query, cloud {b}: padding with copies changes nothing"
        want, wcnt = oracle.ball_query(r_xyz[b:b + 1].cpu().numpy(), x[b:b + 1, :n], r, ns, return_cnt=True)
        assert np.array_equal(r_bq[b].cpu().numpy(), want[0]) and np.array_equal(r_cnt[b].cpu().numpy(), wcnt[0])
    rc, dc = r_cnt.cpu().numpy(), d_cnt.cpu().numpy()
    assert (rc == ns).any(), "no full group"
    assert (rc < ns).any(), "no partial group"
    only_pads = (dc == ns) & (rc < ns)
    assert only_pads[1:].any(), "no group that is partial only because the pad rows are excluded"


# ----------------------------------------------------------------------------------------------------------- ball query
def _check_ball_query(dev, oracle, x, centres, lengths, r, ns):
    from pointcloudlib_amd.misc import ops
    B, N, _ = x.shape
    q = torch.from_numpy(centres).to(dev)
    got = []
    for how in FILLS:
        xp = torch.from_numpy(_fill(x, lengths, how)).to(dev)
        idx, cnt = ops.ball_query(q, xp, r, ns, return_cnt=True, lengths=lengths)
        got.append((idx.cpu().numpy(), cnt.cpu().numpy()))
    assert all(np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) for g in got[1:]), "pad rows influence the lists"
    idx, cnt = got[0]
    for b, n in enumerate(lengths):
        assert idx[b].min() >= 0 and idx[b].max() < n, f"cloud {b}: an index beyond its {n} points (padding and zero-hit rows included)"
        want, wcnt = oracle.ball_query(centres[b:b + 1], x[b:b + 1, :n], r, ns, return_cnt=True)
        assert np.array_equal(idx[b], want[0]) and np.array_equal(cnt[b], wcnt[0]), f"cloud {b} (n={n}) vs the oracle on the cloud alone"
        d_idx, d_cnt = ops.ball_query(q[b:b + 1], torch.from_numpy(x[b:b + 1, :n].copy()).to(dev), r, ns, return_cnt=True)
        assert np.array_equal(idx[b], d_idx.cpu().numpy()[0]) and np.array_equal(cnt[b], d_cnt.cpu().numpy()[0]), f"cloud {b}: dense kernel"
    xp = torch.from_numpy(_fill(x, lengths, "huge")).to(dev)
    t_idx, t_cnt = ops.ball_query(q, xp, r, ns, return_cnt=True, lengths=torch.tensor(lengths, dtype=torch.int32, device=dev))
    assert np.array_equal(t_idx.cpu().numpy(), idx) and np.array_equal(t_cnt.cpu().numpy(), cnt), "device lengths tensor"
    assert np.array_equal(ops.ball_query(q, xp, r, ns, lengths=lengths).cpu().numpy(), idx), "return_cnt=False"
    xd = torch.from_numpy(x).to(dev)
    f = ops.ball_query(q, xd, r, ns, return_cnt=True, lengths=[N] * B)
    d = ops.ball_query(q, xd, r, ns, return_cnt=True)
    assert torch.equal(f[0], d[0]) and torch.equal(f[1], d[1]), "lengths = [N] * B is not the dense entry point's result"
    return cnt


def test_ball_query_ragged_lds_variant(dev, oracle):
    N, m = 1024, 512
    lengths = RECIPE_LENGTHS
    x = _clouds(len(lengths), N, 7)
    centres = np.stack([oracle.fps(x[b:b + 1, :n], m, block_size=TIE, return_xyz=True)[1][0] for b, n in enumerate(lengths)])
    centres[:, -1] = 50.0                                               # a query without any hit: zero-filled, cnt 0
    cnt = _check_ball_query(dev, oracle, x, centres, lengths, 0.2, 64)
    assert (cnt == 64).any() and (cnt < 64).any() and (cnt[:, -1] == 0).all()


def test_ball_query_ragged_global_memory_variant(dev, oracle):
    N, m = 13000, 96                                                    # 3 N floats = 152 KiB: beyond the LDS variant's 150 KiB
    lengths = [N, m, m + 1, 6501, 9999, N - 1]
    x = _clouds(len(lengths), N, 5)
    centres = x[:, :m].copy()
    centres[:, -1] = 50.0
    cnt = _check_ball_query(dev, oracle, x, centres, lengths, 0.15, 32)
    assert (cnt == 32).any() and (cnt < 32).any()


@pytest.mark.parametrize("N", [1024, 13000])
def test_ball_query_multi_ragged_three_radii(dev, oracle, N):
    from pointcloudlib_amd.misc import ops
    m = 128
    lengths = RECIPE_LENGTHS if N == 1024 else [N, m, m + 1, 6501, 9999, N - 1]
    radii, nss = [0.1, 0.2, 0.4], [16, 32, 128]
    B = len(lengths)
    x = _clouds(B, N, 7)
    centres = np.stack([oracle.fps(x[b:b + 1, :n], m, block_size=TIE, return_xyz=True)[1][0] for b, n in enumerate(lengths)])
    centres[:, -1] = 50.0
    q = torch.from_numpy(centres).to(dev)
    got = []
    for how in FILLS:
        xp = torch.from_numpy(_fill(x, lengths, how)).to(dev)
        got.append([(i.cpu().numpy(), c.cpu().numpy()) for i, c in ops.ball_query_multi(q, xp, radii, nss, return_cnt=True, lengths=lengths)])
    for g in got[1:]:
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(g, got[0])), "pad rows influence the lists"
    xp = torch.from_numpy(_fill(x, lengths, "nan")).to(dev)
    nv = torch.tensor(lengths, dtype=torch.int32, device=dev)
    for k, (r, ns) in enumerate(zip(radii, nss)):
        idx, cnt = got[0][k]
        for b, n in enumerate(lengths):
            assert idx[b].max() < n and idx[b].min() >= 0
            want, wcnt = oracle.ball_query(centres[b:b + 1], x[b:b + 1, :n], r, ns, return_cnt=True)
            assert np.array_equal(idx[b], want[0]) and np.array_equal(cnt[b], wcnt[0]), f"radius {r}, cloud {b}"
        s_idx, s_cnt = ops.ball_query(q, xp, r, ns, return_cnt=True, lengths=nv)          # the single-radius ragged kernel agrees
        assert np.array_equal(s_idx.cpu().numpy(), idx) and np.array_equal(s_cnt.cpu().numpy(), cnt)
    t = ops.ball_query_multi(q, xp, radii, nss, return_cnt=True, lengths=nv)
    assert all(np.array_equal(a[0].cpu().numpy(), b[0]) and np.array_equal(a[1].cpu().numpy(), b[1]) for a, b in zip(t, got[0]))
    xd = torch.from_numpy(x).to(dev)
    f = ops.ball_query_multi(q, xd, radii, nss, return_cnt=True, lengths=[N] * B)
    d = ops.ball_query_multi(q, xd, radii, nss, return_cnt=True)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(f, d))


# ----------------------------------------------------------------------------------------------------------------- 3-NN
@pytest.mark.parametrize("which", ["targets", "sources", "both"])
@pytest.mark.parametrize("S", [512, 5000])              # one staged chunk; two chunks (S > 4096)
def test_three_nn_ragged(dev, oracle, which, S):
    from pointcloudlib_amd.misc import ops
    N = 1000                                            # not a multiple of the 32 targets of a workgroup
    l1 = [N, 1, 33, 640, 777, 999] if which != "sources" else None
    l2 = [S, 1, 2, 3, S // 2 + 1, S - 1] if which != "targets" else None
    B = 6
    x1, x2 = _clouds(B, N, 3), _clouds(B, S, 4)
    x2[4, 5] = x2[4, 9]                                 # equal distances: the (distance, index) order decides
    got = []
    for how in FILLS:
        a = torch.from_numpy(_fill(x1, l1, how) if l1 else x1).to(dev)
        b = torch.from_numpy(_fill(x2, l2, how) if l2 else x2).to(dev)
        idx, w = ops.three_nn(a, b, lengths1=l1, lengths2=l2)
        got.append((idx.cpu().numpy(), _bits(w)))
    assert all(np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) for g in got[1:]), "pad rows influence the result"
    idx, w = got[0]
    for b in range(B):
        n1, n2 = (l1[b] if l1 else N), (l2[b] if l2 else S)
        assert idx[b].min() >= 0 and idx[b].max() < n2, f"cloud {b}: a source index beyond its {n2} points"
        w_idx, w_w = oracle.three_nn(x1[b:b + 1, :n1], x2[b:b + 1, :n2])
        assert np.array_equal(idx[b, :n1], w_idx[0]) and np.array_equal(w[b, :n1], w_w[0].view(np.int32)), f"cloud {b} vs the oracle"
        d_idx, d_w = ops.three_nn(torch.from_numpy(x1[b:b + 1, :n1].copy()).to(dev), torch.from_numpy(x2[b:b + 1, :n2].copy()).to(dev))
        assert np.array_equal(idx[b, :n1], d_idx.cpu().numpy()[0]) and np.array_equal(w[b, :n1], _bits(d_w)[0]), f"cloud {b}: dense kernel"
        assert not idx[b, n1:].any() and not w[b, n1:].any(), f"cloud {b}: pad targets must be idx 0, w 0"
    a = torch.from_numpy(_fill(x1, l1, "nan") if l1 else x1).to(dev)
    b = torch.from_numpy(_fill(x2, l2, "nan") if l2 else x2).to(dev)
    as_dev = lambda l: None if l is None else torch.tensor(l, dtype=torch.int32, device=dev)
    t_idx, t_w = ops.three_nn(a, b, lengths1=as_dev(l1), lengths2=as_dev(l2))
    assert np.array_equal(t_idx.cpu().numpy(), idx) and np.array_equal(_bits(t_w), w), "device lengths tensors"
    xa, xb = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    f_idx, f_w = ops.three_nn(xa, xb, lengths1=[N] * B if l1 else None, lengths2=[S] * B if l2 else None)
    d_idx, d_w = ops.three_nn(xa, xb)
    assert torch.equal(f_idx, d_idx) and np.array_equal(_bits(f_w), _bits(d_w)), "full lengths are not the dense entry point's result"


def test_device_lengths_must_be_int32_of_shape_b(dev):
    from pointcloudlib_amd.misc import ops
    x = torch.rand(3, 64, 3, device=dev)
    with pytest.raises(TypeError, match="int32"):
        ops.furthest_point_sample(x, 8, lengths=torch.tensor([64, 64, 64], device=dev))
    with pytest.raises(ValueError, match="shape"):
        ops.ball_query(x[:, :8].contiguous(), x, 0.2, 4, lengths=torch.tensor([64, 64], dtype=torch.int32, device=dev))
