"""Training step of PointNet++ part segmentation on a ragged batch: dense ``forward`` against ``forward_packed``.

One step = forward + ``seg_cross_entropy_loss`` + backward + SGD (``train_utils.make_sgd``), SSG and MSG at B = 16, N = 2048.  Three
forms alternate window by window in one process (device events around each window, median over the windows, the estimator of
``tools/bench_infer.py --ragged``):
  (a) ``dense``        the existing ``forward`` at capacity -- unchanged code, the yardstick;
  (b) ``packed_full``  ``forward_packed`` with every length = N (the same B * N rows, built and consumed as packed rows);
  (c) ``packed``       ``forward_packed`` with lengths drawn once (fixed seed) uniformly from [N/2, N], the largest forced to N.
Each form trains its own copy of the network (same initial state) with a sampling handle produced once outside the windows, so
a window holds the step alone.  Peak memory is ``torch.cuda.max_memory_allocated`` above the resident set over one step.  Prints
one JSON line and writes it to profiles/partseg_ragged_train_bench_line.json.

    python tools/bench_partseg_ragged_train.py [--windows 7] [--iters 5] [--warmup 3] [--batch 16] [--points 2048] [--nets ssg msg]
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


def _case(kind, B, N, a, dev):
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.misc import ops
    from pointcloudlib_amd.networks.seg import pointnet2_partseg as seg_nets
    from pointcloudlib_amd.train_utils import make_sgd, seg_cross_entropy_loss
    xyz = torch.from_numpy(synth.gauss_ball(B, N, 1)).to(dev)
    nrm = torch.from_numpy(synth.unit_normals(B, N, 2)).to(dev)
    onehot = torch.zeros(B, 16, device=dev)
    onehot[torch.arange(B), torch.arange(B) % 16] = 1.0
    seg = torch.randint(0, 50, (B, N), generator=torch.Generator().manual_seed(3)).to(dev)
    lengths = np.random.default_rng(12345).integers(N // 2, N + 1, B)
    lengths[int(lengths.argmax())] = N
    drawn = [int(v) for v in lengths]

    torch.manual_seed(0)
    proto = (seg_nets.PointNet2_partseg if kind == "ssg" else seg_nets.PointNetMSG)().to(dev)
    state = {k: v.clone() for k, v in proto.state_dict().items()}

    def form(lens):
        net = (seg_nets.PointNet2_partseg if kind == "ssg" else seg_nets.PointNetMSG)().to(dev).train()
        net.load_state_dict(state)
        opt = make_sgd(net.parameters(), lr=1e-3, momentum=0.9)
        handle = net.precompute_sampling(xyz, lengths=lens)
        if lens is None:
            def step():
                opt.zero_grad(set_to_none=True)
                seg_cross_entropy_loss(net(xyz, nrm, onehot, sampling=handle), seg).backward()
                opt.step()
        else:
            def step():
                opt.zero_grad(set_to_none=True)
                logits, row_off = net.forward_packed(xyz, nrm, onehot, sampling=handle)
                seg_cross_entropy_loss(logits, ops.pack_rows(seg, handle["lengths"], row_off, handle["n_rows"])).backward()
                opt.step()
        return step

    forms = [("dense", form(None)), ("packed_full", form([N] * B)), ("packed", form(drawn))]
    for _ in range(a.warmup):
        for _, fn in forms:
            fn()
    times = {name: [] for name, _ in forms}
    for w in range(a.windows):
        for name, fn in (forms if w % 2 == 0 else forms[::-1]):
            times[name].append(_window(fn, a.iters))
    case = {"net": kind, "B": B, "N": N, "rows_dense": B * N, "rows_packed": int(lengths.sum()), "mean_length": round(float(lengths.mean()), 1),
            "min_length": int(lengths.min())}
    for name, fn in forms:
        case[f"{name}_ms"] = round(statistics.median(times[name]), 4)
        case[f"{name}_ms_min"] = round(min(times[name]), 4)
        case[f"{name}_ms_max"] = round(max(times[name]), 4)
        case[f"{name}_peak_mib"] = round(_peak(fn) / 2**20, 1)
    case["packed_full_vs_dense"] = round(case["packed_full_ms"] / case["dense_ms"], 4)
    case["packed_vs_dense"] = round(case["packed_ms"] / case["dense_ms"], 4)
    case["packed_full_inside_dense_range"] = bool(case["dense_ms_min"] <= case["packed_full_ms"] <= case["dense_ms_max"])
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--nets", nargs="+", default=["ssg", "msg"], choices=["ssg", "msg"])
    ap.add_argument("--no-write", action="store_true", help="print only, leave profiles/ alone")
    a = ap.parse_args()
    from pointcloudlib_amd import _lib
    _lib.lib()
    dev = torch.device("cuda:0")
    res = {"what": "PointNet++ part-seg training step (forward + loss + backward + SGD), ms per step, median of interleaved windows",
           "device": torch.cuda.get_device_name(0), "windows": a.windows, "iters": a.iters, "warmup": a.warmup,
           "cases": [_case(kind, a.batch, a.points, a, dev) for kind in a.nets]}
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "partseg_ragged_train_bench_line.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
