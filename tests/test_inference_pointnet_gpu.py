"""Frozen PointNet inference on the GPU (pointcloudlib_amd/inference.py: FrozenPointNet, csrc/infer_pointnet.hip): the fused conv
stack + max through the C ABI on exactly representable data (bit for bit against fp64), its shapes, strides, ragged batches and
launch variants, random data and whole networks against an fp64 evaluation-mode restatement, the memory a forward needs, and the
contract of ``FrozenPointNet``.

Yardstick (tests/test_inference_gpu.py): the frozen result may be no further from the fp64 restatement than the existing
evaluation path on the same inputs, x 1.25, plus 1e-6."""
import copy
import ctypes
import functools
import os
import subprocess
import sys

import pytest
import torch

from test_inference_gpu import _act, _consts64, _err, _perturb, _ref_head

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = [3, 64, 64, 64, 128, 1024]
RAGGED = [200, 1, 64, 65, 129]


def _P(t):
    return None if t is None else t.data_ptr()


def _splits(B, N):
    from pointcloudlib_amd import _lib
    return _lib.lib().pcl_pointnet_stack_infer_splits(B, N)


def _call(x, n_valid, Ws, scales, shifts, slope, ldo=1024):
    """pcl_pointnet_stack_infer_f32 on x [B,3,N] (a view of any strides), n_valid device int32 [B] or None -> out [B, ldo] whose
    columns beyond 1024 were filled with 7 before the call."""
    from pointcloudlib_amd import _lib
    B, _, N = x.shape
    L = len(Ws)
    widths = (ctypes.c_int32 * L)(*[w.shape[0] for w in Ws])
    c_W = (ctypes.c_void_p * L)(*[_P(w) for w in Ws])
    c_sc = (ctypes.c_void_p * L)(*[_P(t) for t in scales])
    c_sh = (ctypes.c_void_p * L)(*[_P(t) for t in shifts])
    need = _lib.lib().pcl_pointnet_stack_infer_workspace_bytes(B, N, 1024)
    ws = torch.full((need // 4,), float("nan"), device=x.device)          # never cleared, never read where it was not written
    out = torch.full((B, ldo), 7.0, device=x.device)
    _lib.call("pcl_pointnet_stack_infer_f32", _P(x), x.stride(0), x.stride(2), x.stride(1), _P(n_valid), B, N, 3, _P(Ws[0]), Ws[0].shape[1],
              L, widths, c_W, c_sc, c_sh, float(slope), _P(ws), need, _P(out), ldo, torch.cuda.current_stream().cuda_stream)
    return out


def _ref64(x, n, Ws, scales, shifts, slope):
    """fp64 restatement: x [B,N,3], n per-cloud counts -> max over each cloud's first n[b] rows of the stack's output [B, 1024]."""
    z = x.double()
    for W, sc, sh in zip(Ws, scales, shifts):
        z = _act(sc.double() * (z @ W.double().t()) + sh.double(), slope)
    return torch.stack([z[b, :n[b]].max(dim=0)[0] for b in range(x.shape[0])])


# ----------------------------------------------------------------------------------------------------------- exact data
@functools.lru_cache(maxsize=None)
def _exact_params(seed=11):
    """Made once, read only.  Every weight row 4 entries of +-1 (3 in layer 1), scale +-1/2, shift an integer in [-2, 2]."""
    g = torch.Generator().manual_seed(seed)
    Ws, scales, shifts = [], [], []
    for cin, cout in zip(SPEC[:-1], SPEC[1:]):
        W = torch.zeros(cout, cin)
        nz = min(4, cin)
        for r in range(cout):
            cols = torch.randperm(cin, generator=g)[:nz]
            W[r, cols] = torch.randint(0, 2, (nz,), generator=g).float() * 2 - 1
        Ws.append(W.cuda())
        scales.append(((torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1) / 2).cuda())
        shifts.append(torch.randint(-2, 3, (cout,), generator=g).float().cuda())
    return Ws, scales, shifts


def _assert_exact_precondition(x, Ws, scales, shifts, slope):
    """In fp64: at every layer the sum of |products| and the activated value, in units of the layer's quantum, stay below 2^24,
    so every product and partial sum is an exact fp32 number in any order."""
    z, q = x.double(), 1.0
    for W, sc, sh in zip(Ws, scales, shifts):
        assert ((z.abs() @ W.double().abs().t()).max().item() / q) < 2 ** 24
        z = _act(sc.double() * (z @ W.double().t()) + sh.double(), slope)
        q = q / 2 * (slope if slope else 1.0)
        assert z.abs().max().item() / q < 2 ** 24
        assert bool((z / q == (z / q).round()).all())


# (B, N, n_valid or None): dense N around the 64-row tile at B = 3, the ragged batch, and every value of the variant function
SHAPES = [(3, 1, None), (3, 63, None), (3, 64, None), (3, 65, None), (3, 129, None), (5, 200, RAGGED), (1, 64, None),
          (3, 3200, None), (5, 3840, None)]


def test_shapes_reach_every_variant():
    assert sorted({_splits(B, N) for B, N, _ in SHAPES}) == [1, 2, 4]
    assert _splits(1, 64) == 4 and _splits(3, 3200) == 2 and _splits(5, 3840) == 1


@pytest.mark.parametrize("B,N,n_valid", SHAPES)
@pytest.mark.parametrize("slope", [0.0, 0.25])
def test_exact_data_bit_for_bit(dev, B, N, n_valid, slope):
    Ws, scales, shifts = _exact_params()
    g = torch.Generator().manual_seed(B * 10007 + N)
    pts = torch.randint(-4, 5, (B, N, 3), generator=g).float().to(dev)              # [B,N,3], a loader's layout
    n = [N] * B if n_valid is None else n_valid
    _assert_exact_precondition(pts, Ws, scales, shifts, slope)
    want = _ref64(pts, n, Ws, scales, shifts, slope).float()
    nv = None
    if n_valid is not None:
        nv = torch.tensor(n_valid, dtype=torch.int32, device=dev)
        for b in range(B):
            pts[b, n[b]:] = float("nan")
    cf = pts.transpose(1, 2).contiguous()                                            # [B,3,N] dense, the network's layout
    ldo = 1024 + 8
    got_nl = _call(pts.transpose(1, 2), nv, Ws, scales, shifts, slope, ldo)          # [B,N,3] strides
    got_cf = _call(cf, nv, Ws, scales, shifts, slope, ldo)                           # [B,3,N] strides
    again = _call(cf, nv, Ws, scales, shifts, slope, ldo)
    torch.cuda.synchronize()
    assert bool((got_cf[:, 1024:] == 7.0).all()) and bool((got_nl[:, 1024:] == 7.0).all()), "wrote beyond column 1024"
    assert torch.equal(got_cf, again), "two calls differ"
    assert torch.equal(got_cf, got_nl), "the two layouts differ"
    assert torch.equal(got_cf[:, :1024], want), f"max |diff| {(got_cf[:, :1024] - want).abs().max().item():.3e}"


# ----------------------------------------------------------------------------------------------------------- random data
def _mlp(dev, slope, seed, spec=SPEC):
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    torch.manual_seed(seed)
    mlp = PointwiseMLP(spec, bias=False, bn=True, slope=slope).to(dev)
    _perturb(mlp, seed)
    return mlp.eval()


def _consts(mlp):
    from pointcloudlib_amd.inference import _eval_consts
    Ws = [w.detach().contiguous() for w in mlp.weights]
    consts = [_eval_consts(mlp, l) for l in range(mlp.n_layers)]
    return Ws, [c[0] for c in consts], [c[1] for c in consts]


def test_cloud_alone(dev):
    """A cloud's output depends only on its own valid rows: the same bits alone, at another batch position and capacity."""
    mlp = _mlp(dev, 0.2, 3)
    Ws, scales, shifts = _consts(mlp)
    B, N = 5, 200
    torch.manual_seed(1)
    pts = torch.randn(B, N, 3, device=dev)
    for b in range(B):
        pts[b, RAGGED[b]:] = float("nan")
    nv = torch.tensor(RAGGED, dtype=torch.int32, device=dev)
    got = _call(pts.transpose(1, 2), nv, Ws, scales, shifts, 0.2)
    assert not bool(torch.isnan(got).any())
    for b in range(B):
        n = RAGGED[b]
        alone = _call(pts[b:b + 1, :n].contiguous().transpose(1, 2), None, Ws, scales, shifts, 0.2)
        assert torch.equal(alone[0], got[b]), f"cloud {b} alone"
        other = torch.full((3, 333, 3), float("nan"), device=dev)               # position 2 of 3, capacity 333
        other[0, :7] = 1.0
        other[1, :333] = -2.0
        other[2, :n] = pts[b, :n]
        moved = _call(other.transpose(1, 2), torch.tensor([7, 333, n], dtype=torch.int32, device=dev), Ws, scales, shifts, 0.2)
        assert torch.equal(moved[2], got[b]), f"cloud {b} at another position and capacity"


@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_kernel_against_fp64(dev, slope):
    mlp = _mlp(dev, slope, 5 + int(10 * slope))
    Ws, scales, shifts = _consts(mlp)
    B, N = 3, 700
    pts = torch.randn(B, N, 3, device=dev)
    with torch.no_grad():
        got = _call(pts.transpose(1, 2), None, Ws, scales, shifts, slope)
        want_eval = mlp(pts[:, None], group_max=N).reshape(B, -1)
    c64 = [_consts64(mlp, l) for l in range(mlp.n_layers)]
    ref = _ref64(pts, [N] * B, [c[0] for c in c64], [c[1] for c in c64], [c[2] for c in c64], slope)
    e_fused, e_eval = _err(got, ref), _err(want_eval, ref)
    print(f"slope {slope}: fused {e_fused:.3e} eval path {e_eval:.3e}")
    assert e_fused <= 1.25 * e_eval + 1e-6, f"fused {e_fused:.3e} vs eval path {e_eval:.3e} from fp64"


# ----------------------------------------------------------------------------------------------------------- networks
def _net(dev, seed=0, convs=None):
    from pointcloudlib_amd.misc.layers import PointwiseMLP
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    torch.manual_seed(seed)
    net = PointNet()
    if convs is not None:
        net.convs = PointwiseMLP(convs, bias=False)
    return _perturb(net.to(dev), seed + 1)


@functools.lru_cache(maxsize=None)
def _clouds(B, N=1024, seed=0):
    from pointcloudlib_amd import synth
    return torch.from_numpy(synth.gauss_ball(B, N, seed)).cuda()                    # [B,N,3]; read only


def _ref_net(net, pts, n):
    mlp = net.convs
    c64 = [_consts64(mlp, l) for l in range(mlp.n_layers)]
    feat = _ref64(pts, n, [c[0] for c in c64], [c[1] for c in c64], [c[2] for c in c64], mlp.slope)
    return feat, _ref_head([net.linear1, net.bn6, net.relu, net.dp1, net.linear2], feat)


def _check_network(net, dev, lengths=None):
    from pointcloudlib_amd.inference import FrozenPointNet
    pts = _clouds(8)
    B, N, _ = pts.shape
    n = [N] * B if lengths is None else lengths
    ref_feat, ref_logits = _ref_net(net, pts, n)
    if lengths is not None:
        pts = pts.clone()
        for b in range(B):
            pts[b, n[b]:] = float("nan")
    x = pts.transpose(1, 2)                                                          # [B,3,N], strides of [B,N,3]
    fnet = FrozenPointNet(net)
    feat, logits = fnet.run(x, lengths)
    ev = copy.deepcopy(net).eval()
    with torch.no_grad():
        ev_logits = ev(x.contiguous()) if lengths is None else ev(x.contiguous(), lengths=lengths)
    torch.cuda.synchronize()
    assert feat.shape == (B, net.convs.spec[-1]) and logits.shape == ev_logits.shape
    ef, ee = _err(logits, ref_logits), _err(ev_logits, ref_logits)
    print(f"logits: frozen {ef:.3e} eval {ee:.3e}; feature: frozen {_err(feat, ref_feat):.3e}")
    bound = 1.25 * ee + 1e-6
    assert ef <= bound, f"logits: frozen {ef:.3e} vs eval {ee:.3e} from fp64"
    top2 = ref_logits.topk(2, dim=1)[0]
    sure = (top2[:, 0] - top2[:, 1]) > 2 * bound
    assert bool((logits.argmax(1) == ref_logits.argmax(1))[sure].all())
    return fnet


def test_frozen_pointnet_against_fp64(dev):
    assert _check_network(_net(dev), dev).plan == "fused"


def test_frozen_pointnet_ragged_against_fp64(dev):
    assert _check_network(_net(dev), dev, [1024, 1, 512, 513, 777, 257, 300, 64]).plan == "fused"


def test_frozen_pointnet_device_lengths(dev):
    net = _net(dev)
    from pointcloudlib_amd.inference import FrozenPointNet
    lengths = [1024, 1, 512, 513, 777, 257, 300, 64]
    x = _clouds(8).transpose(1, 2)
    fnet = FrozenPointNet(net)
    a = fnet(x, lengths)
    b = fnet(x, torch.tensor(lengths, dtype=torch.int32, device=dev))
    assert torch.equal(a, b)


def test_frozen_pointnet_falls_back_for_other_widths(dev):
    net = _net(dev, seed=4, convs=[3, 64, 64, 96, 1024])
    assert _check_network(net, dev).plan == "module"
    assert _check_network(net, dev, [1024, 1, 512, 513, 777, 257, 300, 64]).plan == "module"


def test_frozen_pointnet_forward_memory(dev):
    from pointcloudlib_amd.inference import FrozenPointNet
    net = _net(dev)
    B, N = 32, 1024
    x = _clouds(B).transpose(1, 2)
    fnet = FrozenPointNet(net)
    fnet(x)                                       # warm-up: one-time allocations (plans)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fnet(x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    bound = 2 * 4 * (B * N * 3 + B * -(-N // 64) * 1024 + B * (1024 + 512 + 40))
    assert out.shape == (B, 40)
    assert peak <= bound, f"frozen forward peak +{peak / 2**20:.2f} MiB > bound {bound / 2**20:.2f} MiB"


def test_frozen_pointnet_contract(dev):
    from pointcloudlib_amd.inference import FrozenPointNet
    net = _net(dev).train()
    x = _clouds(8).transpose(1, 2)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fnet = FrozenPointNet(net)
    out = fnet(x)
    torch.cuda.synchronize()
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    with torch.no_grad():
        net.convs.running_var_2.mul_(3.0)
    stale = fnet(x)
    fresh = fnet.refresh()(x)
    torch.cuda.synchronize()
    assert torch.equal(stale, out)
    assert not torch.equal(fresh, out)
    assert torch.equal(fresh, FrozenPointNet(net)(x))


def test_train_cls_fast_eval_pointnet(dev):
    cmd = [sys.executable, os.path.join(ROOT, "train_cls.py"), "--model", "pointnet", "--fast_eval", "--epochs", "1",
           "--synthetic_items", "64"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "val acc" in r.stdout
