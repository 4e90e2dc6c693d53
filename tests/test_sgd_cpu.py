"""CPU: the optimiser step's yardstick (tests/sgd_ref.py) against an element-by-element scalar loop, and the host-side
validation of ``pcl_sgd_momentum_f32`` (a rejected table launches nothing, so no GPU is needed)."""
import ctypes

import numpy as np
import pytest

import sgd_ref as R

PCL_EINVAL = -1


@pytest.mark.parametrize("lr,mu,wd,damp", R.HYPER)
def test_vectorised_restatement_equals_the_scalar_loop(lr, mu, wd, damp):
    """The fp64 restatement the GPU tests compare with, against the same three statements in Python ``float`` arithmetic with one
    ``np.float32`` round trip per statement: bit for bit on a few hundred random elements, for every hyper-parameter tuple."""
    rng = np.random.default_rng(17)
    n = 300
    p, g, v = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    g[:4] = [np.inf, -np.inf, np.nan, 0.0]                     # the non-finite case of the GPU tests
    g0 = g.copy()
    p1, v1 = R.sgd_ref(p, g, v, lr, mu, wd, damp)
    ps, vs = R.sgd_ref_scalar(p, g, v, lr, mu, wd, damp)
    assert np.array_equal(R.bits(g), R.bits(g0)), "sgd_ref modified g"
    assert p1.dtype == v1.dtype == np.float32
    assert R.same_bits(p1, ps), R.first_difference(p1, ps)
    assert R.same_bits(v1, vs), R.first_difference(v1, vs)
    assert R.all_normal(p1[4:], v1[4:])
    if lr == 0.0:
        assert np.array_equal(R.bits(p1[3:]), R.bits(p[3:]))   # (p - 0 * inf is NaN: the three non-finite elements aside)
    else:
        assert not np.array_equal(p1[4:], p[4:])


def test_helpers_tell_one_ulp_from_equal():
    a = np.array([1.0, -1.0, 0.5, 3.0e38], np.float32)
    b = np.nextafter(a, np.float32(0.0))
    assert list(R.ulp_distance(a, a)) == [0, 0, 0, 0] and list(R.ulp_distance(a, b)) == [1, 1, 1, 1]
    assert R.same_bits(a, a) and not R.same_bits(a, b)
    assert not R.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert R.same_bits(np.array([np.nan, 1.0], np.float32), np.array([-np.nan, 1.0], np.float32))
    assert not R.same_bits(np.array([np.inf], np.float32), np.array([np.nan], np.float32))
    assert not R.all_normal(np.array([1e-39], np.float32)) and not R.all_normal(np.array([0.0], np.float32)) and R.all_normal(a)


@pytest.mark.parametrize("n,bad", [(3, 2), (120, 100)])
@pytest.mark.parametrize("kind", ["null_grad", "null_param", "null_buf", "negative", "two_to_32", "two_to_32_less_a_block"])
def test_bad_entry_anywhere_in_the_table_is_rejected_on_the_host(n, bad, kind):
    """A table with a bad entry returns PCL_EINVAL and names the tensor, whichever chunk of 96 the entry lies in: the whole table
    is validated before the first launch.  Every table here holds a bad entry, the pointers are made up: nothing is launched."""
    from pointcloudlib_amd import _lib
    lib = _lib.lib()
    U64, I64 = ctypes.c_uint64 * n, ctypes.c_int64 * n
    pa, ga, ba = (U64(*[base + 4096 * i for i in range(n)]) for base in (0x10000000, 0x20000000, 0x30000000))
    na = I64(*[1 + i for i in range(n)])
    if kind == "null_grad":
        ga[bad] = 0
    elif kind == "null_param":
        pa[bad] = 0
    elif kind == "null_buf":
        ba[bad] = 0
    else:
        na[bad] = {"negative": -1, "two_to_32": 2 ** 32, "two_to_32_less_a_block": 2 ** 32 - 4096}[kind]
    assert lib.pcl_sgd_momentum_f32(pa, ga, ba, na, n, 0.02, 0.9, 1e-4, 0.0, None) == PCL_EINVAL
    msg = lib.pcl_last_error().decode()
    assert f"tensor {bad}:" in msg, msg
