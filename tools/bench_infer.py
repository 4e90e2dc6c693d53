"""Evaluation forward of the PointNet++ classifiers: ``net.eval()`` + ``torch.no_grad()`` (the existing path) against
``frozen(net)`` (pointcloudlib_amd/inference.py).  SSG and MSG, B in {32, 256}, N = 1024, synthetic clouds; the two forms
alternate window by window in one process, device events around each window, median over the windows; peak
``torch.cuda.max_memory_allocated`` above the resident set of one forward of each form.  Prints one JSON line.

    python tools/bench_infer.py [--windows 7] [--iters 5] [--warmup 3] [--batch 32 256] [--nets ssg msg]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--nets", nargs="+", default=["ssg", "msg"])
    ap.add_argument("--frozen_only", action="store_true", help="run only the frozen form (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infer.py needs a GPU")
    from pointcloudlib_amd import synth
    from pointcloudlib_amd.inference import frozen
    from pointcloudlib_amd.networks.cls.pointnet2 import PointNet2_cls, PointNetMSG
    dev = torch.device("cuda")
    res = {"N": 1024, "windows": a.windows, "iters": a.iters, "cases": []}
    for kind in a.nets:
        torch.manual_seed(0)
        net = (PointNet2_cls if kind == "ssg" else PointNetMSG)().to(dev).eval()
        fnet = frozen(net)
        for B in a.batch:
            xyz = torch.from_numpy(synth.gauss_ball(B, 1024, 1)).to(dev)
            nrm = torch.from_numpy(synth.unit_normals(B, 1024, 2)).to(dev)

            def eval_fwd():
                with torch.no_grad():
                    return net(xyz, nrm)

            def frozen_fwd():
                return fnet(xyz, nrm)

            forms = [("frozen", frozen_fwd)] if a.frozen_only else [("eval", eval_fwd), ("frozen", frozen_fwd)]
            for _ in range(a.warmup):
                for _, fn in forms:
                    fn()
            times = {name: [] for name, _ in forms}
            for w in range(a.windows):
                for name, fn in (forms if w % 2 == 0 else forms[::-1]):
                    times[name].append(_window(fn, a.iters))
            case = {"net": kind, "B": B}
            for name, fn in forms:
                case[f"{name}_ms"] = round(statistics.median(times[name]), 4)
                case[f"{name}_ms_min"] = round(min(times[name]), 4)
                case[f"{name}_peak_mib"] = round(_peak(fn) / 2**20, 1)
            if not a.frozen_only:
                case["speedup"] = round(case["eval_ms"] / case["frozen_ms"], 3)
                with torch.no_grad():
                    case["max_abs_logit_diff"] = float((eval_fwd() - frozen_fwd()).abs().max())
            res["cases"].append(case)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
