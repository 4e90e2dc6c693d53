"""CPU oracle for the point-cloud hot path -- TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import this
package, and only as the checker / the timed CPU baseline.  ``pointcloudlib_amd`` never imports it.

PINNED for the three index kernels (FPS, ball query, k-NN; see ``pcl_oracle.c`` header and DESIGN.md section 0 c): the
oracle restates the reference's CUDA text, and that text itself -- cut out by ``ref_kernels.py``, compiled by hipcc for
gfx950 with ``-ffp-contract=off`` -- returns the same indices on an MI355X (``tests/test_reference_kernels_gpu.py``); its
recorded output holds the oracle and ``np_oracle.py`` to it on every machine (``tests/test_reference_golden_cpu.py``).
STILL UNPINNED: which products nvcc itself contracts, and everything the reference does through Jittor ops (argsort,
matmul, reindex, the 3-NN of misc/ops.py:83-93, PointConv's Python FPS and knn_point) -- so every network restatement
here.  The reference can still not be imported; hand-derived known answers and a second, independent NumPy restatement
remain.
"""
from .oracle import (  # noqa: F401
    lib_path, build, optimal_block, fps, ball_query, group, group_bwd, group_all, knn, three_nn,
    three_interp, num_threads, density, set_contract, get_contract, contract, knn_point_matmul,
)
