"""Training step of PointNet (classification and part segmentation) on a ragged batch: the dense ``forward`` against the packed
rows of DESIGN.md section 16.

One step = forward + loss + backward + SGD (``train_utils.make_sgd``): the classifier at B = 8 and B = 32, N = 1024
(``soft_cross_entropy_loss``), part segmentation at B = 16, N = 2048 (``seg_cross_entropy_loss``).  Three forms alternate window by
window in one process (device events around each window, median over the windows, the estimator of
``tools/bench_partseg_ragged_train.py``):
  (a) ``dense``        the existing ``forward`` at capacity -- unchanged code, the yardstick;
  (b) ``packed_full``  the ragged path with every length = N (the same B * N rows, packed, pooled per segment);
  (c) ``packed``       the ragged path with lengths drawn once (fixed seed) uniformly from [N/2, N], the largest forced to N.
Each form trains its own copy of the network (same initial state).  Lengths are handed over as a device tensor with ``n_rows``, so a
step holds no host synchronisation of its own.  Peak memory is ``torch.cuda.max_memory_allocated`` above the resident set over one
step.  Prints one JSON line and writes it to profiles/pointnet_ragged_bench_line.json.

    python tools/bench_pointnet_ragged.py [--windows 7] [--iters 5] [--warmup 3] [--cases cls8 cls32 seg16]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = {"cls8": ("cls", 8, 1024), "cls32": ("cls", 32, 1024), "seg16": ("seg", 16, 2048)}


def _window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _case(name, a, dev):
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.misc import ops
    from pointcloudlib_amd.networks.cls.pointnet import PointNet
    from pointcloudlib_amd.networks.seg.pointnet_partseg import PointNet_partseg
    from pointcloudlib_amd.train_utils import make_sgd, seg_cross_entropy_loss, soft_cross_entropy_loss
    kind, B, N = CASES[name]
    x = torch.from_numpy(synth.gauss_ball(B, N, 1)).transpose(1, 2).contiguous().to(dev)          # [B,3,N]
    lab = torch.from_numpy(synth.labels(B, 40, 3)).to(dev)
    onehot = torch.zeros(B, 16, device=dev)
    onehot[torch.arange(B), torch.arange(B) % 16] = 1.0
    seg = torch.randint(0, 50, (B, N), generator=torch.Generator().manual_seed(3)).to(dev)
    lengths = np.random.default_rng(12345).integers(N // 2, N + 1, B)
    lengths[int(lengths.argmax())] = N
    drawn = [int(v) for v in lengths]
    make = PointNet if kind == "cls" else PointNet_partseg
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in make().to(dev).state_dict().items()}

    def form(lens):
        net = make().to(dev).train()
        net.load_state_dict(state)
        opt = make_sgd(net.parameters(), lr=1e-3, momentum=0.9)
        if lens is not None:
            R = int(sum(lens))
            lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
        if kind == "cls":
            def loss():
                out = net(x) if lens is None else net(x, lengths=lens_dev, n_rows=R)
                return soft_cross_entropy_loss(out, lab)
        elif lens is None:
            def loss():
                return seg_cross_entropy_loss(net(x, onehot), seg)
        else:
            def loss():
                logits, row_off = net.forward_packed(x, onehot, lengths=lens_dev, n_rows=R)
                return seg_cross_entropy_loss(logits, ops.pack_rows(seg, lens_dev, row_off, R))

        def step():
            opt.zero_grad(set_to_none=True)
            loss().backward()
            opt.step()
        return step

    forms = [("dense", form(None)), ("packed_full", form([N] * B)), ("packed", form(drawn))]
    for _ in range(a.warmup):
        for _, fn in forms:
            fn()
    times = {n: [] for n, _ in forms}
    for w in range(a.windows):
        for n, fn in (forms if w % 2 == 0 else forms[::-1]):
            times[n].append(_window(fn, a.iters))
    case = {"case": name, "net": "PointNet " + kind, "B": B, "N": N, "rows_dense": B * N, "rows_packed": int(lengths.sum()),
            "mean_length": round(float(lengths.mean()), 1), "min_length": int(lengths.min())}
    for n, fn in forms:
        case[f"{n}_ms"] = round(statistics.median(times[n]), 4)
        case[f"{n}_ms_min"] = round(min(times[n]), 4)
        case[f"{n}_ms_max"] = round(max(times[n]), 4)
        case[f"{n}_peak_mib"] = round(_peak(fn) / 2**20, 1)
    case["packed_full_vs_dense"] = round(case["packed_full_ms"] / case["dense_ms"], 4)
    case["packed_vs_dense"] = round(case["packed_ms"] / case["dense_ms"], 4)
    case["packed_full_inside_dense_range"] = bool(case["dense_ms_min"] <= case["packed_full_ms"] <= case["dense_ms_max"])
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--no-write", action="store_true", help="print only, leave profiles/ alone")
    a = ap.parse_args()
    from pointcloudlib_amd import _lib
    _lib.lib()
    dev = torch.device("cuda:0")
    res = {"what": "PointNet training step (forward + loss + backward + SGD), ms per step, median of interleaved windows",
           "device": torch.cuda.get_device_name(0), "windows": a.windows, "iters": a.iters, "warmup": a.warmup,
           "cases": [_case(name, a, dev) for name in a.cases]}
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "pointnet_ragged_bench_line.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
