"""Frozen PointNet inference with bf16 matrix operands on the GPU (``FrozenPointNet(net, precision="bf16")``,
pcl_pointnet_stack_infer_bf16_f32; csrc/infer_pointnet.hip).

Exact data (every rounded value a small integer): the bf16 launch must equal fp64, the fp32 launch and a second call bit for bit,
which pins every k, row and column mapping.  Random data: the yardstick of tests/pointnet_bf16_yardstick.py (the contract restated
in fp64 with its roundings, a tight bound T on the last layer's fp32 arithmetic, at most 1 % of the outputs over T and those within
the worst-case bound).  Then the contract of ``FrozenPointNet`` under either precision."""
import ctypes
import functools

import pytest
import torch

import pointnet_bf16_yardstick as y
from test_inference_pointnet_gpu import RAGGED, _clouds, _net

pytestmark = pytest.mark.gpu

BF16, FP32 = "pcl_pointnet_stack_infer_bf16_f32", "pcl_pointnet_stack_infer_f32"
SPEC = y.SPEC
# two clouds of 129 tiles of 128 rows: 258 such tiles, and from 256 on a workgroup takes 128 rows; last tiles of 32 and of 65 rows
BIG = (2, 16416, [16416, 16321])


def _P(t):
    return None if t is None else t.data_ptr()


def _splits(B, N):
    from pointcloudlib_amd import _lib
    return _lib.lib().pcl_pointnet_stack_infer_splits(B, N)


def _call(entry, x, n_valid, Ws, scales, shifts, slope, ldo=1024):
    """``entry`` on x [B,3,N] (a view of any strides), n_valid device int32 [B] or None, Ws[l >= 1] of the entry's element type
    -> out [B, ldo] whose columns beyond 1024 were filled with 7 before the call.  The workspace is pre-filled with NaN."""
    from pointcloudlib_amd import _lib
    B, _, N = x.shape
    L = len(Ws)
    want_dtype = torch.bfloat16 if entry == BF16 else torch.float32
    assert Ws[0].dtype == torch.float32 and all(w.dtype == want_dtype and w.is_contiguous() for w in Ws[1:])
    widths = (ctypes.c_int32 * L)(*[w.shape[0] for w in Ws])
    c_W = (ctypes.c_void_p * L)(*[None if l == 0 else _P(w) for l, w in enumerate(Ws)])      # W[0] is ignored
    c_sc = (ctypes.c_void_p * L)(*[_P(t) for t in scales])
    c_sh = (ctypes.c_void_p * L)(*[_P(t) for t in shifts])
    need = _lib.lib().pcl_pointnet_stack_infer_workspace_bytes(B, N, 1024)
    ws = torch.full((need // 4,), float("nan"), device=x.device)
    out = torch.full((B, ldo), 7.0, device=x.device)
    _lib.call(entry, _P(x), x.stride(0), x.stride(2), x.stride(1), _P(n_valid), B, N, 3, _P(Ws[0]), Ws[0].shape[1], L, widths, c_W, c_sc,
              c_sh, float(slope), _P(ws), need, _P(out), ldo, torch.cuda.current_stream().cuda_stream)
    return out


def _as_fp32(Wl):
    return [Wl[0]] + [w.float().contiguous() for w in Wl[1:]]


# ----------------------------------------------------------------------------------------------------------- exact data
@functools.lru_cache(maxsize=None)
def _exact_params(seed=23):
    """Made once, read only.  Weight rows with 2 / 3 / 3 / 4 / 4 entries of +-1 at random columns; scale 1 (the last layer: -1 on
    about a quarter of its columns, so both signs of the last epilogue are pinned), shift 0."""
    g = torch.Generator().manual_seed(seed)
    Ws, scales, shifts = [], [], []
    for l, (cin, cout) in enumerate(zip(SPEC[:-1], SPEC[1:])):
        nz = (2, 3, 3, 4, 4)[l]
        W = torch.zeros(cout, cin)
        for r in range(cout):
            cols = torch.randperm(cin, generator=g)[:nz]
            W[r, cols] = torch.randint(0, 2, (nz,), generator=g).float() * 2 - 1
        Ws.append(W.cuda())
        sc = torch.ones(cout)
        if l == 4:
            sc[torch.rand(cout, generator=g) < 0.25] = -1.0
        scales.append(sc.cuda())
        shifts.append(torch.zeros(cout).cuda())
    return Ws, scales, shifts


def _exact_ref64(pts, n, Ws, scales, shifts):
    """fp64 restatement at slope 0 with the exactness precondition asserted: every activation an integer, at most 256 where the
    kernel rounds to bf16 (layers 1-4), sums of |products| far below 2^24 in the last layer, and a result that is not all zero."""
    out = []
    for b in range(pts.shape[0]):
        best = None
        for r0 in range(0, n[b], 8192):                                       # in chunks: the big shape has 16 416 rows a cloud
            z = pts[b, r0:min(n[b], r0 + 8192)].double()
            for l, (W, sc, sh) in enumerate(zip(Ws, scales, shifts)):
                W = W.double()
                assert float((z.abs() @ W.abs().t()).max()) < 2 ** 16
                z = (sc.double() * (z @ W.t()) + sh.double()).clamp_(min=0.0)
                assert bool((z == z.round()).all())
                if l < 4:
                    assert float(z.max()) <= 256
            m = z.max(dim=0)[0]
            best = m if best is None else torch.maximum(best, m)
        out.append(best)
    out = torch.stack(out)
    assert int((out != 0).sum()) > 0
    return out


# (B, N, n_valid or None): N around the 64-row tile, the ragged batch, one shape per split count, and the 128-row workgroups
SHAPES = [(3, 1, None), (3, 63, None), (3, 64, None), (3, 65, None), (3, 129, None), (5, 200, RAGGED), (1, 64, None),
          (3, 3200, None), (5, 3840, None), BIG]


def test_shapes_reach_every_variant():
    assert [_splits(1, 64), _splits(3, 3200), _splits(5, 3840), _splits(*BIG[:2])] == [4, 2, 1, 1]
    tiles128 = [B * -(-N // 128) for B, N, _ in SHAPES]              # 64 rows per workgroup below 256 such tiles, 128 from there on
    assert max(tiles128[:-1]) < 256 <= tiles128[-1] and 1 * -(-BIG[2][1] // 128) < 256


def _exact_points(B, N, n_valid, dev):
    g = torch.Generator().manual_seed(B * 10007 + N)
    pts = torch.randint(0, 4, (B, N, 3), generator=g).float().to(dev)               # [B,N,3], a loader's layout
    n = [N] * B if n_valid is None else n_valid
    return pts, n


@pytest.mark.parametrize("B,N,n_valid", SHAPES)
def test_exact_data_bit_for_bit(dev, B, N, n_valid):
    Ws, scales, shifts = _exact_params()
    Wl = y.launch_weights(Ws)
    assert all(torch.equal(a.float(), b) for a, b in zip(Wl, Ws))                    # +-1 and 0: exact in bf16
    pts, n = _exact_points(B, N, n_valid, dev)
    want = _exact_ref64(pts, n, Ws, scales, shifts).float()
    nv = None
    if n_valid is not None:
        nv = torch.tensor(n_valid, dtype=torch.int32, device=dev)
        for b in range(B):
            pts[b, n[b]:] = float("nan")
    cf = pts.transpose(1, 2).contiguous()                                            # [B,3,N] dense, the network's layout
    ldo = 1024 + 8
    got_nl = _call(BF16, pts.transpose(1, 2), nv, Wl, scales, shifts, 0.0, ldo)      # [B,N,3] strides
    got_cf = _call(BF16, cf, nv, Wl, scales, shifts, 0.0, ldo)                       # [B,3,N] strides
    again = _call(BF16, cf, nv, Wl, scales, shifts, 0.0, ldo)
    got_32 = _call(FP32, cf, nv, Ws, scales, shifts, 0.0, ldo)
    torch.cuda.synchronize()
    assert bool((got_cf[:, 1024:] == 7.0).all()) and bool((got_nl[:, 1024:] == 7.0).all()), "wrote beyond column 1024"
    assert torch.equal(got_cf, again), "two calls differ"
    assert torch.equal(got_cf, got_nl), "the two layouts differ"
    assert torch.equal(got_cf[:, :1024], want), f"bf16 vs fp64: max |diff| {(got_cf[:, :1024] - want).abs().max().item():.3e}"
    assert torch.equal(got_cf, got_32), "bf16 and fp32 launches differ"


# ----------------------------------------------------------------------------------------------------------- random data
def _ragged_points(pts, n):
    pts = pts.clone()
    for b in range(pts.shape[0]):
        pts[b, n[b]:] = float("nan")
    return pts


@pytest.mark.parametrize("B,N,n_valid", [(4, 129, None), (5, 200, RAGGED)])
@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("negated", [False, True])
def test_random_data_against_the_yardstick(dev, B, N, n_valid, slope, negated):
    """``negated``: every third scale of the last layer negated (the generator's scales are all positive; the last epilogue has
    one path per sign)."""
    pts, Ws, sc, sh = y.case(100 + int(10 * slope), B, N, dev)
    if negated:
        sc = sc[:-1] + [sc[-1] * torch.where(torch.arange(1024, device=dev) % 3 == 0, -1.0, 1.0)]
    Wl = y.launch_weights(Ws)
    n = [N] * B if n_valid is None else n_valid
    bounds = y.want_and_bounds(pts, n, Wl, sc, sh, slope)
    nv = None
    if n_valid is not None:
        nv = torch.tensor(n_valid, dtype=torch.int32, device=dev)
        pts = _ragged_points(pts, n)
    got = _call(BF16, pts.transpose(1, 2), nv, Wl, sc, sh, slope)
    got_32 = _call(FP32, pts.transpose(1, 2), nv, _as_fp32(Wl), sc, sh, slope)
    torch.cuda.synchronize()
    y.check(got, *bounds, f"B={B} N={N} {'ragged' if n_valid else 'dense'} slope {slope} negated {negated}")
    assert not torch.equal(got, got_32), "the bf16 entry returned the fp32 kernel's bits"


def test_cloud_alone(dev):
    """Every cloud of the ragged batch equals the same cloud in a B = 1 launch (another capacity) and at another position, capacity
    and split count, bit for bit."""
    B, N = 5, 200
    assert (_splits(5, 200), _splits(3, 3200)) == (4, 2)
    pts, Ws, sc, sh = y.case(7, B, N, dev)
    Wl = y.launch_weights(Ws)
    nv = torch.tensor(RAGGED, dtype=torch.int32, device=dev)
    got = _call(BF16, _ragged_points(pts, RAGGED).transpose(1, 2), nv, Wl, sc, sh, 0.2)
    assert not bool(torch.isnan(got).any())
    for b, n in enumerate(RAGGED):
        alone = _call(BF16, pts[b:b + 1, :n].contiguous().transpose(1, 2), None, Wl, sc, sh, 0.2)
        assert torch.equal(alone[0], got[b]), f"cloud {b} alone"
        other = torch.full((3, 3200, 3), float("nan"), device=dev)              # position 2 of 3, capacity 3200: two splits, not four
        other[0, :7] = 1.0
        other[1, :3200] = -2.0
        other[2, :n] = pts[b, :n]
        other[2, n:] = 5.0                                                      # finite pad rows that would win a max
        moved = _call(BF16, other.transpose(1, 2), torch.tensor([7, 3200, n], dtype=torch.int32, device=dev), Wl, sc, sh, 0.2)
        assert torch.equal(moved[2], got[b]), f"cloud {b} at another position, capacity and split count"


def test_cloud_alone_across_rows_per_workgroup(dev):
    """A cloud of the big batch (128 rows per workgroup) equals itself alone (64 rows per workgroup, capacity n), bit for bit."""
    B, N, n = BIG
    pts, Ws, sc, sh = y.case(8, B, N, dev)
    Wl = y.launch_weights(Ws)
    nv = torch.tensor(n, dtype=torch.int32, device=dev)
    got = _call(BF16, _ragged_points(pts, n).transpose(1, 2), nv, Wl, sc, sh, 0.0)
    alone = _call(BF16, pts[1:2, :n[1]].contiguous().transpose(1, 2), None, Wl, sc, sh, 0.0)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(alone[0], got[1])


# ----------------------------------------------------------------------------------------------------------- networks
LENGTHS = [1024, 1, 512, 513, 777, 257, 300, 64]


def _fnet_consts(fnet):
    return [fnet.Ws[0]] + list(fnet.Ws_bf16[1:]), fnet.scales, fnet.shifts, fnet.slope


@pytest.mark.parametrize("lengths", [None, LENGTHS])
def test_frozen_pointnet_bf16_feature_within_the_yardstick(dev, lengths):
    from pointcloudlib_amd.inference import FrozenPointNet
    net = _net(dev)
    pts = _clouds(8)
    B, N, _ = pts.shape
    fnet = FrozenPointNet(net, precision="bf16")
    assert fnet.plan == "fused" and fnet.precision == "bf16"
    Wl, sc, sh, slope = _fnet_consts(fnet)
    n = [N] * B if lengths is None else lengths
    bounds = y.want_and_bounds(pts, n, Wl, sc, sh, slope)
    x = (pts if lengths is None else _ragged_points(pts, n)).transpose(1, 2)
    feat, logits = fnet.run(x, lengths)
    torch.cuda.synchronize()
    assert feat.shape == (B, 1024) and logits.shape == (B, 40) and feat.dtype == logits.dtype == torch.float32
    y.check(feat, *bounds, f"FrozenPointNet bf16 global feature, lengths {lengths}")
    assert bool(torch.isfinite(logits).all())
    if lengths is not None:                                                          # ragged == every cloud alone, logits included
        for b in range(B):
            f1, l1 = fnet.run(pts[b:b + 1, :n[b]].contiguous().transpose(1, 2))
            assert torch.equal(f1[0], feat[b]), f"cloud {b} alone: feature"
            assert torch.equal(l1[0], logits[b]), f"cloud {b} alone: logits"


def test_frozen_pointnet_fp32_is_the_default_bit_for_bit(dev):
    from pointcloudlib_amd.inference import FrozenPointNet
    net = _net(dev)
    x = _clouds(8).transpose(1, 2)
    f_def, l_def = FrozenPointNet(net).run(x, LENGTHS)
    f_32, l_32 = FrozenPointNet(net, precision="fp32").run(x, LENGTHS)
    f_16, l_16 = FrozenPointNet(net, precision="bf16").run(x, LENGTHS)
    assert torch.equal(f_def, f_32) and torch.equal(l_def, l_32)
    assert not torch.equal(f_16, f_32)


def test_frozen_pointnet_bf16_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointNet
    net = _net(dev).train()
    x = _clouds(8).transpose(1, 2)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = FrozenPointNet(net, precision="bf16")
    out = fnet(x)
    torch.cuda.synchronize()
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    with torch.no_grad():
        net.convs.weights[3].mul_(1.25)
    stale = fnet(x)
    fresh = fnet.refresh()(x)
    torch.cuda.synchronize()
    assert torch.equal(stale, out)
    assert not torch.equal(fresh, out)
    assert torch.equal(fresh, FrozenPointNet(net, precision="bf16")(x))


def test_frozen_pointnet_bf16_forward_memory(dev):
    """The bound formula of test_frozen_pointnet_forward_memory: the bf16 forward allocates what the fp32 forward does."""
    from pointcloudlib_amd.inference import FrozenPointNet
    net = _net(dev)
    B, N = 32, 1024
    x = _clouds(B).transpose(1, 2)
    fnet = FrozenPointNet(net, precision="bf16")
    fnet(x)                                       # warm-up: one-time allocations (plans)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fnet(x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    bound = 2 * 4 * (B * N * 3 + B * -(-N // 64) * 1024 + B * (1024 + 512 + 40))
    assert out.shape == (B, 40)
    assert peak <= bound, f"frozen bf16 forward peak +{peak / 2**20:.2f} MiB > bound {bound / 2**20:.2f} MiB"


def test_module_plan_ignores_the_precision(dev):
    from pointcloudlib_amd.inference import FrozenPointNet
    net = _net(dev, seed=4, convs=[3, 64, 64, 96, 1024])
    x = _clouds(8).transpose(1, 2)
    f32, f16 = FrozenPointNet(net), FrozenPointNet(net, precision="bf16")
    assert f32.plan == f16.plan == "module" and f16.precision == "bf16"
    assert torch.equal(f32(x), f16(x))
    assert torch.equal(f32(x, LENGTHS), f16(x, LENGTHS))
