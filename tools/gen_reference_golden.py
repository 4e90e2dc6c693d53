"""Generate tests/golden/reference_index_ops.npz -- what the reference's OWN index kernels return on the cases of
oracle/ref_cases.py.  Needs an MI355X and oracle/_ref/libpcl_ref_off.so (built by __graft_entry__.build() where a reference
checkout is present; it is never read here).

The reference's CUDA text, compiled by hipcc with -ffp-contract=off, runs on the device; its outputs are recorded next to their
inputs.  The file holds recorded data only.  tests/test_reference_golden_cpu.py then holds oracle/pcl_oracle.c and
oracle/np_oracle.py to these arrays on machines with neither a GPU nor the reference.

* indices are stored as int16 (every cloud has at most 300 points); rows of a ball query without a hit, which the reference
  leaves unwritten, are stored as -1;
* the case with 5000 references is left out, and the two widest k-NN feature clouds (C = 64 and C = 130, ~290 KB of random
  floats) are stored as their generator seed and SHA-256: the test regenerates them and checks the digest.

    python tools/gen_reference_golden.py [--out tests/golden/reference_index_ops.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from oracle import ref_cases as rc  # noqa: E402
from oracle import ref_kernels  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STORE_INPUT_UP_TO = 16384            # values; a larger input is stored as seed + digest


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(GOLD, "reference_index_ops.npz"))
    args = ap.parse_args()
    ref = ref_kernels.load("off")
    if ref is None:
        raise SystemExit("oracle/_ref/libpcl_ref_off.so not built: run __graft_entry__.build() next to a reference checkout")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the recorded values are the reference kernels' own output")
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    I16 = lambda t: t.cpu().numpy().astype(np.int16)
    g, differs = {}, []

    for name, (xyz, m) in rc.fps_cases().items():
        g[f"fps.{name}.xyz"], g[f"fps.{name}.m"] = xyz, np.int32(m)
        for S in rc.FPS_BLOCKS:
            idx = ref.fps(T(xyz), m, S).cpu().numpy()
            assert idx.min() >= 0 and idx.max() < xyz.shape[1]
            g[f"fps.{name}.S{S}"] = idx.astype(np.int16)
            if not np.array_equal(idx, oracle.fps(xyz, m, block_size=S)):
                differs.append(f"fps {name} S={S}")

    for name, (q, xyz, radii, n_hitless) in rc.bq_cases(oracle).items():
        g[f"bq.{name}.q"], g[f"bq.{name}.xyz"], g[f"bq.{name}.n_hitless"] = q, xyz, np.int32(n_hitless)
        B = q.shape[0]
        for r in radii:
            for ns in rc.BQ_NSAMPLES:
                idx, cnt = ref.ball_query(T(q), T(xyz), r, ns, oracle.optimal_block(B), fill=-1)
                idx64, cnt64 = ref.ball_query(T(q), T(xyz), r, ns, 64, fill=-1)
                assert torch.equal(idx, idx64) and torch.equal(cnt, cnt64), "the block size changed a ball query"
                g[f"bq.{name}.r{r}_ns{ns}.idx"], g[f"bq.{name}.r{r}_ns{ns}.cnt"] = I16(idx), I16(cnt)
                want, wcnt = oracle.ball_query(q, xyz, r, ns, return_cnt=True)
                hit = cnt.cpu().numpy() > 0
                if not (np.array_equal(wcnt, cnt.cpu().numpy()) and np.array_equal(want[hit], idx.cpu().numpy()[hit])):
                    differs.append(f"ball_query {name} r={r} ns={ns}")

    shapes = {rc.knn_name(s): s for s in rc.KNN_SHAPES}
    for name, (x_q, x_r, k) in rc.knn_cases(with_two_pass=False).items():
        if x_r.size > STORE_INPUT_UP_TO:
            g[f"knn.{name}.seed"] = np.int64(rc.knn_seed(shapes[name]))
            g[f"knn.{name}.shape"] = np.array(shapes[name], np.int32)
            g[f"knn.{name}.sha"] = np.array(rc.sha(x_q) + rc.sha(x_r))
        else:
            g[f"knn.{name}.x_q"], g[f"knn.{name}.x_r"] = x_q, x_r
        g[f"knn.{name}.k"] = np.int32(k)
        idx = ref.knn(T(x_q), T(x_r), k).cpu().numpy()
        assert idx.min() >= 0 and idx.max() < x_r.shape[2]
        g[f"knn.{name}.idx"] = idx.astype(np.int16)
        if not np.array_equal(idx, oracle.knn(x_q, x_r, k)):
            differs.append(f"knn {name}")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **g)
    size, cap = os.path.getsize(args.out), os.path.getsize(os.path.join(GOLD, "sa_level.npz"))
    print(f"wrote {args.out}: {len(g)} arrays, {size} bytes (largest committed fixture: {cap})")
    print("oracle differs from the recorded reference output on:", differs or "nothing")
    if size > cap:
        raise SystemExit("fixture larger than the largest one already committed")


if __name__ == "__main__":
    main()
