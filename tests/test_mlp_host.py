"""The numpy twin of the MLP policy (tests/mlp_numpy.py) against libm and exact rational arithmetic: its float32 fused multiply-add, the
forward pass, the heads.  No GPU."""
import ctypes
from fractions import Fraction

import numpy as np

import mlp_numpy as M

_libm = ctypes.CDLL("libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _libm_fmaf(a, b, c):
    return np.array([_libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float32).view(np.int32), np.asarray(y, np.float32).view(np.int32))


def test_fmaf32_on_random_triples():
    rng = np.random.default_rng(0)
    n = 20000
    a, b, c = (rng.standard_normal(n).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, n).astype(np.float32) for _ in range(3))
    assert _same_bits(M.fmaf32(a, b, c), _libm_fmaf(a, b, c))


def test_fmaf32_near_cancellation_at_many_scales():
    rng = np.random.default_rng(1)
    n = 20000
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    c = (-(a.astype(np.float64) * b)).astype(np.float32)                     # c = -a*b rounded: the sum is the product's rounding error
    nudge = rng.integers(-2, 3, n)
    c = np.where(nudge < 0, np.nextafter(c, np.float32(-np.inf)), np.where(nudge > 0, np.nextafter(c, np.float32(np.inf)), c)).astype(np.float32)
    for e in (-60, -30, -8, 0, 8, 30, 60):
        s = np.float32(2.0 ** e)
        assert _same_bits(M.fmaf32(a * s, b, c * s), _libm_fmaf(a * s, b, c * s)), e
    c2 = (c * np.float32(2.0) ** rng.integers(-30, 30, n).astype(np.float32)).astype(np.float32)       # and c far from the product, both ways
    assert _same_bits(M.fmaf32(a, b, c2), _libm_fmaf(a, b, c2))
    tiny = np.float32(2.0 ** -75)                                                                       # results in the subnormal range
    assert _same_bits(M.fmaf32(a * tiny, b * tiny, c * tiny * tiny), _libm_fmaf(a * tiny, b * tiny, c * tiny * tiny))


def test_fmaf32_double_rounding_case():
    """a = b = 1 + 2^-12: a*b = 1 + 2^-11 + 2^-24 lies exactly half way between two float32; c = +-2^-60 decides, and a float64 sum has
    already lost it."""
    a = np.float32(1 + 2.0 ** -12)
    up, down = M.fmaf32(a, a, np.float32(2.0 ** -60)), M.fmaf32(a, a, np.float32(-2.0 ** -60))
    assert float(down) == 1 + 2.0 ** -11 and float(up) == 1 + 2.0 ** -11 + 2.0 ** -23
    for c, want in ((2.0 ** -60, up), (-2.0 ** -60, down)):
        assert _same_bits([want], _libm_fmaf([a], [a], [np.float32(c)]))
    naive = np.float32(np.float64(a) * np.float64(a) + np.float64(np.float32(2.0 ** -60)))
    assert float(naive) != float(up)                                         # the plain float64 sum gets it wrong


def _round_f32(q):
    """The float32 nearest (ties to even) to the Fraction q, exactly."""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    m = q / ulp
    f = m.numerator // m.denominator
    r = m - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2):
        f += 1
    return np.float32(sign * float(f * ulp))


def test_forward_against_exact_fractions():
    rng = np.random.default_rng(2)
    widths = (5, 3, 2)
    p = M.nasty_params(rng, 1, widths)[0]
    x = M.nasty_inputs(rng, 7, 5)
    got = M.raw_forward(p, widths, x)
    ls = M.layers(p, widths)
    for e in range(x.shape[0]):
        h = [np.float32(v) for v in x[e]]
        for l, (W, b) in enumerate(ls):
            out = []
            for j in range(W.shape[1]):
                acc = np.float32(b[j])
                for k in range(W.shape[0]):
                    acc = _round_f32(Fraction(float(h[k])) * Fraction(float(W[k, j])) + Fraction(float(acc)))
                if l == 0:
                    acc = acc if acc > 0 else np.float32(0.0)
                out.append(acc)
            h = out
        assert _same_bits(got[e], np.array(h, np.float32)), e


def test_hidden_activation_maps_nan_and_minus_zero_to_plus_zero():
    widths = (1, 3, 3)
    p = np.zeros(M.param_count(widths), np.float32)
    (W0, b0), (W1, b1) = M.layers(p, widths)
    b0[:] = [np.nan, -0.0, -3.0]
    W1[:] = np.eye(3, dtype=np.float32)
    b1[:] = -0.0
    y = M.raw_forward(p, widths, np.zeros((1, 1), np.float32))
    assert np.array_equal(y, np.zeros((1, 3), np.float32)) and not np.signbit(y).any()


def test_box_head_clip_edges():
    lo, hi = np.array([0.0, -57.3]), np.array([0.5, 57.3])
    y = np.array([[-1.0, 1.0], [-7.0, 7.0], [0.0, -0.0], [np.nan, np.inf], [-np.inf, np.nan], [1 - 2.0 ** -24, -1 + 2.0 ** -24]], np.float32)
    a = M.head_of(y, M.BOX2, lo, hi)
    assert np.array_equal(a[0], [0.0, 57.3]) and np.array_equal(a[1], [0.0, 57.3])
    assert np.array_equal(a[2], [0.25, 0.0])
    assert np.array_equal(a[3], [0.0, 57.3]) and np.array_equal(a[4], [0.0, -57.3])           # NaN -> u = -1 -> lo
    assert (a >= lo).all() and (a <= hi).all()
    u = np.float64(np.float32(1 - 2.0 ** -24))
    assert a[5, 0] == 0.0 + ((u + 1.0) * 0.5) * (0.5 - 0.0)                                    # one rounding per operation, in this order
    t = M.head_of(y[:, 1:], M.TURN, lo[1:], hi[1:])
    assert t.shape == (6,) and np.array_equal(t, a[:, 1])


def test_discrete_head_first_maximum_and_nan():
    nan = np.nan
    y = np.array([[0, 3, 3, 1, 3], [2, 2, 2, 2, 2], [nan, 1, 0, 0, 0], [0, nan, -1, nan, -2], [-1, nan, nan, nan, 5], [nan] * 5,
                  [-np.inf, -np.inf, -1, -np.inf, -1], [0.0, -0.0, 0.0, -0.0, 0.0]], np.float32)
    k = M.discrete_head(y)
    assert k.dtype == np.int32
    assert k.tolist() == [1, 0, 0, 0, 4, 0, 2, 0]
    # (row 2: nothing compares greater than a NaN at index 0, so it keeps the default; a NaN elsewhere never wins)


def test_constructed_rows_depend_on_ties_and_subnormals():
    """The rows the GPU test feeds the kernel (tie_case, subnormal_case): every set's actions change under the arithmetic it is built
    against, and the tie rows are exactly one float32 ulp apart by the sign of the bias."""
    lo, hi = np.array([0.0, -0.57296]), np.array([0.5, 0.57296])
    for case, wrong, other in ((M.tie_case, M.fma_f64sum, M.fma_flush), (M.subnormal_case, M.fma_flush, M.fma_f64sum)):
        widths, p, x = case(180)
        exact = M.population(p, widths, x, M.BOX2, lo, hi, M.ROWS)
        bad = M.population(p, widths, x, M.BOX2, lo, hi, M.ROWS, fma=wrong)
        assert ((exact != bad).any(1).reshape(4, M.ROWS).sum(1) >= M.ROWS - 1).all()
        assert np.array_equal(exact, M.population(p, widths, x, M.BOX2, lo, hi, M.ROWS, fma=other))      # and on nothing else
    widths, p, x = M.tie_case(180)
    y = M.raw_forward(p[0], widths, x[:M.ROWS - 1])
    assert (y[:, 0] == np.float32(0.5 + 2.0 ** -11 + 2.0 ** -23)).all() and (y[:, 1] == np.float32(0.5 + 2.0 ** -11)).all()
    widths, p, x = M.subnormal_case(180)
    y = M.raw_forward(p[0], widths, x[:M.ROWS])
    m = (1 << 19) + 37 * np.arange(M.ROWS) + 1
    assert np.array_equal(y[:, 0].astype(np.float64), m * 2.0 ** -21) and np.array_equal(y[:, 1], -y[:, 0])
    assert (M.raw_forward(p[0], widths, x[:M.ROWS], fma=M.fma_flush) == 0).all()
