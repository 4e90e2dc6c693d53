"""The yardstick of the optimiser-step tests (``pcl_sgd_momentum_f32``, csrc/sgd.hip).  TEST INFRASTRUCTURE, no test of its own;
NumPy only, needs no GPU.

The library is built with -ffp-contract=off, so each of the kernel's three statements is IEEE fp64 products and sums of fp32
operands (the hyper-parameters are doubles) followed by ONE rounding to fp32.  That is exactly reproducible on the CPU, so the
comparison is bit for bit and no tolerance has to be measured:

    g1 = g                                  if wd == 0.0 else  f32( f64(g) + wd * f64(p) )
    v1 = f32( mu * f64(v) + (1.0 - damp) * f64(g1) )
    p1 = f32( f64(p) - lr * f64(v1) )

``sgd_ref`` is the vectorised restatement, ``sgd_ref_scalar`` the same three statements element by element in Python ``float``
arithmetic with an ``np.float32`` round trip after each (tests/test_sgd_cpu.py holds the two to each other).
"""
import numpy as np

# (lr, momentum, weight_decay, dampening) of the optimiser-step tests: the drivers' two settings (train_cls.py, train_partseg.py),
# dampening != 0, no momentum, and lr = 0 (p must not move)
HYPER = [(0.02, 0.9, 0.0, 0.0), (0.02, 0.9, 1e-4, 0.0), (0.05, 0.9, 1e-3, 0.1), (0.1, 0.0, 0.0, 0.0), (0.0, 0.9, 1e-4, 0.0)]

F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


def sgd_ref(p, g, v, lr, mu, wd, damp):
    """float32 arrays in (``g`` is not modified), Python-float hyper-parameters -> (p_new, v_new) float32 arrays."""
    p, g, v = (np.asarray(a) for a in (p, g, v))
    assert p.dtype == g.dtype == v.dtype == np.float32
    lr, mu, wd, damp = float(lr), float(mu), float(wd), float(damp)
    one_minus_damp = 1.0 - damp                       # formed once in double, as the host code does
    p64 = p.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        g1 = g if wd == 0.0 else (g.astype(np.float64) + wd * p64).astype(np.float32)
        v1 = (mu * v.astype(np.float64) + one_minus_damp * g1.astype(np.float64)).astype(np.float32)
        p1 = (p64 - lr * v1.astype(np.float64)).astype(np.float32)
    return p1, v1


def sgd_ref_scalar(p, g, v, lr, mu, wd, damp):
    """The same three statements one element at a time: Python ``float`` (IEEE fp64) arithmetic, one ``np.float32`` round trip
    after each statement."""
    lr, mu, wd, damp = float(lr), float(mu), float(wd), float(damp)
    one_minus_damp = 1.0 - damp
    p1, v1 = np.empty(len(p), np.float32), np.empty(len(p), np.float32)
    for i in range(len(p)):
        pi, gi, vi = float(p[i]), float(g[i]), float(v[i])
        if wd != 0.0:
            gi = float(np.float32(gi + wd * pi))
        vi = float(np.float32(mu * vi + one_minus_damp * gi))
        pi = float(np.float32(pi - lr * vi))
        p1[i], v1[i] = pi, vi
    return p1, v1


def bits(a):
    """The int32 view of a float32 array (what "bit for bit" compares)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(got, want):
    """Bit equality of two float32 arrays; where ``want`` is NaN any NaN will do (the payload of a NaN is not part of the contract)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    got, want = got.ravel(), want.ravel()
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def first_difference(got, want):
    """A short description of the first differing element (for assertion messages), or None."""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    if not bad.any():
        return None
    i = int(np.argmax(bad))
    return f"{int(bad.sum())} of {bad.size} elements differ, first at {i}: got {got[i]!r} want {want[i]!r}"


def ulp_distance(a, b):
    """Distance in fp32 units in the last place between two finite float32 arrays (int64 array)."""
    def key(x):                                        # monotone map of the fp32 bit patterns onto the integers
        i = bits(x).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def normal_mask(a):
    """Elementwise: a normal fp32 number (finite, no subnormal and not 0 -- IEEE 754's "normal")."""
    a = np.asarray(a)
    return np.isfinite(a) & (np.abs(a) >= F32_MIN_NORMAL)


def all_normal(*arrays):
    """The precondition of the tests' random inputs and of the restatement's outputs: normal numbers only.  Subnormals are out of
    scope, and so is an exact 0: it comes out of a statement whose two terms cancel exactly, where nothing is left to compare but the
    rounding residue of a product."""
    return all(bool(np.all(normal_mask(a))) for a in arrays)


def abnormal_elements(p, g, v, lr, mu, wd, damp):
    """Mask of the elements with an operand, the intermediate gradient g1 or a result that is no normal number."""
    p1, v1 = sgd_ref(p, g, v, lr, mu, wd, damp)
    g1 = g if float(wd) == 0.0 else (np.asarray(g, np.float64) + float(wd) * np.asarray(p, np.float64)).astype(np.float32)
    ok = normal_mask(p) & normal_mask(g) & normal_mask(v) & normal_mask(g1) & normal_mask(p1) & normal_mask(v1)
    return ~ok
