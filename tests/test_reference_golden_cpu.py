"""CPU: the oracle and its NumPy restatement reproduce what the reference's OWN kernels returned on an MI355X
(tests/golden/reference_index_ops.npz, recorded by tools/gen_reference_golden.py from the -ffp-contract=off build of
oracle/ref_kernels.py) -- exactly, on a machine with neither a GPU nor the reference.  And the recipe itself: where a reference
checkout is present the reference libraries have been built, so the GPU comparison cannot be skipped there unnoticed."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as npo
from oracle import ref_cases as rc
from oracle import ref_kernels

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_index_ops.npz")


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return {k: g[k] for k in g.files}


def names(gold, op):
    return sorted({k.split(".")[1] for k in gold if k.startswith(op + ".")})


# ------------------------------------------------------------------------------------ the recipe
def test_reference_libraries_are_built_where_the_reference_is_present():
    ref = ref_kernels.reference_dir()
    if not os.path.isdir(ref):
        assert ref_kernels.build(verbose=False) == [ref_kernels.lib_path(c) for c in ref_kernels.CONTRACTS if os.path.exists(ref_kernels.lib_path(c))]
        return                                                      # nothing to extract from: build() left oracle/_ref alone
    found = [k for text in ref_kernels.cut(ref).values() for k in ref_kernels.kernels_in(text)]
    for kernel in ("__update", "furthest_point_sampling_kernel", "query_ball_point_kernel", "compute_distances", "modified_insertion_sort"):
        assert kernel in found, f"{kernel} not in the text cut out of {ref}"
    for c in ("off", "fast"):
        assert os.path.exists(ref_kernels.lib_path(c)), f"{ref} exists but __graft_entry__.build() did not produce {ref_kernels.lib_path(c)}"
        L = ref_kernels.load(c)
        assert L is not None
        # the launcher refuses on the host, before any launch, what the kernels cannot do: a block the reduction tree does not
        # cover (it has no 1024 step), a block that is no power of two, k > Nr
        buf = ctypes.create_string_buffer(64)
        p = ctypes.cast(buf, ctypes.c_void_p)
        for block in (1024, 3, 0):
            assert L._L.ref_fps(p, p, p, 1, 8, 4, block, None) != 0, block
        assert L._L.ref_fps(p, p, p, 1, 8, 9, 4, None) != 0                      # m > N
        assert L._L.ref_knn(p, p, p, p, 1, 3, 8, 8, 9, None) != 0                # k > Nr
        assert L._L.ref_ball_query(p, p, p, p, 1, 8, 4, ctypes.c_float(0.2), 0, 4, None) != 0   # nsample < 1


def _fake_reference(tmp_path, fps_host="int block_size = #block_size;", bq_kernel="query_ball_point_kernel", knn_host="inline static bool knn_cuda_global"):
    """a reference tree of the right outline with empty kernels of our own"""
    src = f'''
class FurthestPointSampler:
    cuda_src = """
        __device__ void __update(int a) {{ }}
        __global__ void furthest_point_sampling_kernel (int b) {{ }}

        {fps_host}
        launch();
    """

class BallQueryGrouper:
    cuda_src = """
        __global__ void {bq_kernel}(int b) {{ }}

        int block_size = #block_size;
    """

class KNN:
    def __init__(self, k):
        self.k = k
        self.cuda_inc = """
        #undef out
        #include "helper_cuda.h"
        __global__ void compute_distances(int a) {{ }}
        __global__ void modified_insertion_sort(int a) {{ }}
           {knn_host}(int b) {{ return true; }}
        """
'''
    os.makedirs(tmp_path / "misc")
    (tmp_path / "misc" / "ops.py").write_text(src)
    return str(tmp_path)


def test_extraction_cuts_at_the_markers_and_names_what_it_misses(tmp_path):
    texts = ref_kernels.cut(_fake_reference(tmp_path / "ok"))
    assert sorted(texts) == sorted(ref_kernels.KERNELS)
    assert "launch" not in texts["fps.inc"] and "#block_size" not in texts["fps.inc"] and "__update" in texts["fps.inc"]
    assert "knn_cuda_global" not in texts["knn.inc"] and "#undef" not in texts["knn.inc"] and "helper_cuda" not in texts["knn.inc"]
    assert ref_kernels.kernels_in(texts["knn.inc"]) == ["compute_distances", "modified_insertion_sort"]
    for kw, word in ((dict(fps_host="int block_size = 4;"), "#block_size"), (dict(bq_kernel="some_other_kernel"), "query_ball_point_kernel"),
                     (dict(knn_host="static bool other_host"), "knn_cuda_global")):
        with pytest.raises(ref_kernels.ExtractError, match=re.escape(word)):
            ref_kernels.cut(_fake_reference(tmp_path / word.strip("#"), **kw))
    with pytest.raises(ref_kernels.ExtractError, match="ops.py"):
        ref_kernels.cut(str(tmp_path / "nowhere"))
    with pytest.raises(ValueError):
        ref_kernels.lib_path("on")


# ------------------------------------------------------------------------------------ the recorded reference output
def test_fixture_is_small_and_records_the_cases_the_gpu_test_runs(oracle, gold):
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(os.path.dirname(GOLD), "sa_level.npz"))
    fps = rc.fps_cases()
    assert names(gold, "fps") == sorted(fps)
    for name, (xyz, m) in fps.items():
        assert np.array_equal(gold[f"fps.{name}.xyz"], xyz) and int(gold[f"fps.{name}.m"]) == m
    bq = rc.bq_cases(oracle)
    assert names(gold, "bq") == sorted(bq)
    for name, (q, xyz, radii, n_hitless) in bq.items():
        assert np.array_equal(gold[f"bq.{name}.q"], q) and np.array_equal(gold[f"bq.{name}.xyz"], xyz)
        assert int(gold[f"bq.{name}.n_hitless"]) == n_hitless
        assert sorted(k for k in gold if k.startswith(f"bq.{name}.r") and k.endswith(".idx")) == \
            sorted(f"bq.{name}.r{r}_ns{ns}.idx" for r in radii for ns in rc.BQ_NSAMPLES)
    assert names(gold, "knn") == sorted(rc.knn_cases(with_two_pass=False))


@pytest.mark.parametrize("name", ["plain300", "plain37", "lattice100", "lattice257", "skips64", "capped128"])
def test_oracle_fps_reproduces_the_reference_kernel(oracle, gold, name):
    xyz, m = gold[f"fps.{name}.xyz"], int(gold[f"fps.{name}.m"])
    for S in rc.FPS_BLOCKS:
        truth = gold[f"fps.{name}.S{S}"].astype(np.int32)
        assert np.array_equal(oracle.fps(xyz, m, block_size=S), truth), f"oracle.fps: {name} block_size={S}"
        assert np.array_equal(npo.fps_np(xyz, m, S), truth), f"np_oracle.fps_np: {name} S={S}"


@pytest.mark.parametrize("name", ["saturation", "exact_radius", "hitless", "rim"])
def test_oracle_ball_query_reproduces_the_reference_kernel(oracle, gold, name):
    q, xyz, n_hitless = gold[f"bq.{name}.q"], gold[f"bq.{name}.xyz"], int(gold[f"bq.{name}.n_hitless"])
    keys = sorted(k for k in gold if k.startswith(f"bq.{name}.r") and k.endswith(".idx"))
    assert keys
    for key in keys:
        r, ns = re.match(r".*\.r([0-9.]+)_ns(\d+)\.idx", key).groups()
        truth, tcnt = gold[key].astype(np.int32), gold[key[:-4] + ".cnt"].astype(np.int32)
        hitless = tcnt == 0                                         # rows the reference left unwritten: recorded as -1
        assert hitless.sum() == n_hitless * q.shape[0] and (truth[hitless] == -1).all() and (truth[~hitless] >= 0).all()
        for who, (idx, cnt) in (("oracle.ball_query", oracle.ball_query(q, xyz, float(r), int(ns), return_cnt=True)),
                                ("np_oracle.ball_query_np", npo.ball_query_np(q, xyz, float(r), int(ns)))):
            assert np.array_equal(cnt, tcnt), f"{who}: {key}"
            assert np.array_equal(idx[~hitless], truth[~hitless]), f"{who}: {key}"
            assert (idx[hitless] == 0).all(), f"{who}: a row without a hit is defined as zeros ({key})"


def knn_inputs(gold, name):
    if f"knn.{name}.x_r" in gold:
        return gold[f"knn.{name}.x_q"], gold[f"knn.{name}.x_r"]
    shape = tuple(int(v) for v in gold[f"knn.{name}.shape"])
    assert rc.knn_seed(shape) == int(gold[f"knn.{name}.seed"])
    x_q, x_r = rc.knn_inputs(shape)
    assert rc.sha(x_q) + rc.sha(x_r) == str(gold[f"knn.{name}.sha"]), "the seeded generator no longer gives the recorded input"
    return x_q, x_r


@pytest.mark.parametrize("name", [rc.knn_name(s) for s in rc.KNN_SHAPES if s[2] <= 4096] + ["lattice", "lattice_kNr", "zeros"])
def test_oracle_knn_reproduces_the_reference_kernels(oracle, gold, name):
    x_q, x_r = knn_inputs(gold, name)
    k = int(gold[f"knn.{name}.k"])
    truth = gold[f"knn.{name}.idx"].astype(np.int32)
    assert np.array_equal(oracle.knn(x_q, x_r, k), truth), f"oracle.knn: {name}"
    assert np.array_equal(npo.knn_np(x_q, x_r, k), truth), f"np_oracle.knn_np: {name}"
