"""The FC head's backward with the dX launches between its layers removed (csrc/head.hip, head_bwd_cols_kernel): a layer's column
workgroups form their dOUT from the dY and W of the layer above in head_bwd_dx_kernel's summation order, and a last Linear without
BatchNorm / activation / dropout shares its launch with the layer below.  Nothing may move by a bit against the per-layer kernels.

Every case runs ``head.fc_head`` forward + backward through the per-layer kernels and through the stack entry points and asserts
  * ``torch.equal`` on the output, ``x.grad``, every parameter gradient and every buffer (all shapes have K < 2048: no atomics);
  * agreement with the fp64 evaluation of the same module sequence within the bound of test_mlp_hip.py's head test
    (2e-5 of max(1, largest reference entry)); the running variance follows the library's rule (biased batch variance);
  * a second stack-path run on the same inputs is ``torch.equal`` to the first.
The per-layer side is ``head.USE_STACK = False``.  With dropout in training mode that path draws torch's masks (``nn.Dropout`` itself),
so there the per-layer side is the chain of ONE-layer heads -- head_bwd_col_kernel + head_bwd_dx_kernel per layer, the launches the
per-layer path makes -- each given the seed under which its dropout hash equals that of layer l of the whole head; the call's seed is
pinned through torch's CUDA generator, where ``head._dropout_seed`` takes it from.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF


def _mods(spec, bn, bias, slope, p, last):
    """last: 'plain' (Linear), 'bn_relu', 'leaky' (Linear + LeakyReLU(0.2)), 'dropout' (Linear + Dropout(0.5))"""
    mods = []
    for i in range(len(spec) - 1):
        end = i == len(spec) - 2
        mods.append(nn.Linear(spec[i], spec[i + 1], bias=bias or end))
        if not end:
            if bn:
                mods.append(nn.BatchNorm1d(spec[i + 1]))
            if slope != 1.0:
                mods.append(nn.ReLU() if slope == 0.0 else nn.LeakyReLU(slope))
            if p:
                mods.append(nn.Dropout(p))
        elif last == "bn_relu":
            mods += [nn.BatchNorm1d(spec[i + 1]), nn.ReLU()]
        elif last == "leaky":
            mods.append(nn.LeakyReLU(0.2))
        elif last == "dropout":
            mods.append(nn.Dropout(0.5))
    seq = nn.Sequential(*mods)
    for m in seq:
        if isinstance(m, nn.BatchNorm1d):
            m.weight.data.uniform_(-1.0, 1.5); m.bias.data.uniform_(-0.5, 0.5)
            m.running_mean.uniform_(-0.3, 0.3); m.running_var.uniform_(0.5, 1.5)
    return seq


def _call_seed(dev, cuda_seed):
    """the 64-bit dropout seed that a head call draws right after torch.cuda.manual_seed(cuda_seed)"""
    from pointcloudlib_amd.misc import head
    torch.cuda.manual_seed(cuda_seed)
    return head._dropout_seed(dev, 4)


def _layer_seed(seed, l):
    """seed' with head_drop(seed', 0) == head_drop(seed, l) (csrc/head.hip): lo = seed_lo ^ c1 (l + 1), hi = seed_hi + c2 (l + 1)"""
    lo = (seed & M32) ^ ((0x9E3779B9 * (l + 1)) & M32) ^ 0x9E3779B9
    hi = ((seed >> 32) + 0x7F4A7C15 * l) & M32
    return (hi << 32) | lo


def _drop_scale(seed, l, R, N, p):
    """drop_scale of csrc/head.hip for layer l's output [R, N]: 0 or 1 / (1 - p), fp32"""
    lo = np.uint64((seed & M32) ^ ((0x9E3779B9 * (l + 1)) & M32))
    hi = np.uint64(((seed >> 32) + 0x7F4A7C15 * (l + 1)) & M32)
    m = np.uint64(M32)
    with np.errstate(over="ignore"):
        h = ((((np.arange(R * N, dtype=np.uint64) + hi) & m) * np.uint64(0x9E3779B1)) & m) ^ lo
        h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & m; h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & m; h ^= h >> np.uint64(16)
        h = (h + hi) & m; h ^= h >> np.uint64(15); h = (h * np.uint64(0x2C1B3C6D)) & m; h ^= h >> np.uint64(12); h = (h * np.uint64(0x297A2D39)) & m
        h ^= h >> np.uint64(15)
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(np.where(u >= np.float32(p), scale, np.float32(0.0)).astype(np.float32).reshape(R, N))


def _result(seq, out, x):
    return (out.detach(), None if x.grad is None else x.grad.detach(), [q.grad.detach() for q in seq.parameters()],
            [b.detach().clone() for b in seq.buffers()])


def _run(seq, x0, gout, stack, cuda_seed, need_dx=True):
    from pointcloudlib_amd.misc import head
    s2 = copy.deepcopy(seq)
    old, head.USE_STACK = head.USE_STACK, stack
    try:
        torch.cuda.manual_seed(cuda_seed)
        x = x0.clone().requires_grad_(need_dx)
        out = head.fc_head(s2, x)
        out.backward(gout)
    finally:
        head.USE_STACK = old
    return _result(s2, out, x)


def _run_one_layer_heads(seq, x0, gout, seed, need_dx=True):
    from pointcloudlib_amd.misc import head
    s2 = copy.deepcopy(seq)
    x = x0.clone().requires_grad_(need_dx)
    cur = x
    for l, (lin, bn, slope, p) in enumerate(head._head_layers(list(s2))):
        plan = head._head_plan([(lin, bn, slope, p)], x0.shape[0], lin.training)
        params = [lin.weight] + ([lin.bias] if lin.bias is not None else []) + ([bn.weight, bn.bias] if bn is not None else [])
        cur = head._HeadStack.apply(cur, (plan, _layer_seed(seed, l)), *params)
    cur.backward(gout)
    return _result(s2, cur, x)


def _run_fp64(seq, x0, gout, seed):
    from pointcloudlib_amd.misc import head
    s2 = copy.deepcopy(seq).double()
    x = x0.double().requires_grad_(True)
    cur = x
    for l, (lin, bn, slope, p) in enumerate(head._head_layers(list(s2))):
        y = F.linear(cur, lin.weight, lin.bias)
        if bn is not None:
            if bn.training:
                mean, var = y.mean(0), y.var(0, unbiased=False)
                with torch.no_grad():                      # the library's rule: the BIASED batch variance into running_var
                    bn.running_mean += (mean - bn.running_mean) * bn.momentum
                    bn.running_var += (var - bn.running_var) * bn.momentum
            else:
                mean, var = bn.running_mean, bn.running_var
            y = (y - mean) / torch.sqrt(var + bn.eps) * bn.weight + bn.bias
        if slope != 1.0:
            y = F.leaky_relu(y, slope)
        if lin.training and p > 0.0:
            y = y * _drop_scale(seed, l, y.shape[0], y.shape[1], p).to(y.device).double()
        cur = y
    cur.backward(gout.double())
    return _result(s2, cur, x)


#        spec                        R   bn     bias   slope p    training last       need_dx
CASES = [
    ([20, 24, 17, 5],                5,  True,  False, 0.0,  0.0, True,  "plain",   True),     # chain tails: N = 5, 17; K = 17 scalar path
    ([20, 24, 17, 5],                5,  True,  True,  0.2,  0.0, True,  "plain",   False),    # no input gradient wanted
    ([64, 40, 33, 10],               32, True,  False, 0.0,  0.0, True,  "plain",   True),     # full rows of the RMAX = 32 form
    ([64, 40, 33, 10],               33, True,  False, 0.0,  0.0, True,  "plain",   True),     # RMAX = 64
    ([64, 40, 33, 10],               64, True,  True,  0.2,  0.0, True,  "plain",   True),
    ([16, 12, 10],                   1,  True,  True,  0.0,  0.0, True,  "plain",   True),     # batch variance 0
    # (R = 2: no Linear bias under BatchNorm.  Its gradient is exactly 0, as the sum of two dy of opposite sign that carry invstd -- of the order
    #  of 1e2 where the column's two values lie close --, so its fp32 rounding, 1e2 x 2^-24 x a few, is not measured by a bound of 2e-5 x max(1, 0))
    ([16, 12, 10],                   2,  True,  False, 0.0,  0.0, True,  "plain",   True),
    ([30, 7],                        5,  True,  True,  0.0,  0.0, True,  "plain",   True),     # one layer: unchanged launches
    ([30, 20, 7],                    5,  True,  True,  0.0,  0.0, True,  "plain",   True),     # two layers: the shared launch alone
    ([30, 20, 7],                    5,  False, True,  1.0,  0.0, True,  "plain",   True),     # Linear -> Linear: a plain layer below a plain layer
    ([48, 96, 96, 24, 10],           33, True,  False, 0.0,  0.0, True,  "plain",   True),     # the dY regions alternate more than once
    ([16, 24, 24, 24, 24, 10],       4,  True,  False, 0.0,  0.0, True,  "plain",   True),     # 5 layers > PCL_HEAD_MAX_LAYERS: per-layer path
    ([20, 24, 17, 5],                5,  True,  False, 0.0,  0.0, True,  "bn_relu", True),     # independence rule off: no shared launch
    ([20, 24, 17, 5],                5,  True,  False, 0.0,  0.0, True,  "leaky",   True),
    ([20, 24, 17, 5],                5,  True,  False, 0.0,  0.0, True,  "dropout", True),
    ([20, 24, 17, 5],                5,  True,  False, 0.0,  0.5, True,  "plain",   True),     # dropout on the middle layers
    ([20, 24, 17, 5],                5,  True,  True,  0.2,  0.5, True,  "plain",   True),
    ([64, 40, 33, 10],               33, True,  False, 0.0,  0.5, True,  "plain",   True),
    ([20, 24, 17, 5],                5,  True,  False, 0.0,  0.5, False, "plain",   True),     # evaluation mode: bn_mode 2, dropout off
    ([64, 40, 33, 10],               32, True,  True,  0.0,  0.0, False, "plain",   True),
    ([16, 8, 1024, 6],               3,  True,  False, 0.0,  0.0, True,  "plain",   True),     # the longest sum a column forms itself
    ([16, 8, 1040, 6],               3,  True,  False, 0.0,  0.0, True,  "plain",   True),     # past it: that seam keeps its dX launch
    ([1024, 512, 256, 40],           32, True,  True,  0.0,  0.0, True,  "plain",   True),     # the headline head
    ([1024, 512, 256, 40],           32, True,  True,  0.0,  0.5, True,  "plain",   True),
]


@pytest.mark.parametrize("spec,R,bn,bias,slope,p,training,last,need_dx", CASES)
def test_merged_head_backward_equals_per_layer_kernels(dev, spec, R, bn, bias, slope, p, training, last, need_dx):
    from pointcloudlib_amd.misc import head
    torch.manual_seed(len(spec) * 1000 + R)
    seq = _mods(spec, bn, bias, slope, p, last)
    x0, gout = torch.randn(R, spec[0]), torch.randn(R, spec[-1])                      # (CPU generator: the same numbers on every machine)
    seq, x0, gout = seq.to(dev).train(training), x0.to(dev), gout.to(dev)
    drops = training and (p > 0.0 or last == "dropout")
    with torch.random.fork_rng(devices=[dev]):
        seed = _call_seed(dev, 77) if drops else 0
        a = _run_one_layer_heads(seq, x0, gout, seed, need_dx) if drops else _run(seq, x0, gout, False, 77, need_dx)
        b = _run(seq, x0, gout, True, 77, need_dx)
        c = _run(seq, x0, gout, True, 77, need_dx)
    if len(spec) - 1 > head._MAXL:
        assert head.head_stack(list(seq), x0) is None
    ref = _run_fp64(seq, x0, gout, seed)
    for name, i in (("out", 0), ("dx", 1)):
        if a[i] is None:
            assert b[i] is None and c[i] is None
            continue
        assert torch.equal(a[i], b[i]), name
        assert torch.equal(b[i], c[i]), (name, "run to run")
    assert len(a[2]) == len(b[2]) == len(ref[2]) and len(a[3]) == len(b[3])
    for k, (u, v, w) in enumerate(zip(a[2], b[2], c[2])):
        assert torch.equal(u, v), ("parameter gradient", k)
        assert torch.equal(v, w), ("parameter gradient", k, "run to run")
    for k, (u, v, w) in enumerate(zip(a[3], b[3], c[3])):
        assert torch.equal(u, v), ("buffer", k)
        assert torch.equal(v, w), ("buffer", k, "run to run")
    pairs = [("out", b[0], ref[0])] + ([("dx", b[1], ref[1])] if need_dx else [])
    pairs += [(f"grad {k}", u, v) for k, (u, v) in enumerate(zip(b[2], ref[2]))]
    pairs += [(f"buffer {k}", u, v) for k, (u, v) in enumerate(zip(b[3], ref[3])) if u.dtype.is_floating_point]
    for name, u, v in pairs:
        err = (u.double() - v).abs().max().item()
        print(f"{name}: max |stack - fp64| = {err:.3e}, largest reference entry {v.abs().max().item():.3e}")
        assert err <= 2e-5 * max(1.0, v.abs().max().item()), name
