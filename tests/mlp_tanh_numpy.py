"""numpy twin of the MLP policy with a choice of hidden activation (include/ftl.h, the ftl_mlp_act block, ``ftl_mlp.activation``): the
layer loop of ``mlp_numpy.raw_forward`` -- the same ``layers`` and ``fmaf32`` -- with ``rnn_numpy.tanh32`` after every hidden chain under
``"tanh"`` and the ReLU select under ``"relu"``; the heads and the population mapping are ``mlp_numpy``'s own.  The device is pinned to this
bit for bit (tests/test_gpu_mlp_tanh.py), and the ReLU branch to ``mlp_numpy.raw_forward`` (tests/test_mlp_tanh_host.py)."""
import numpy as np

import mlp_numpy as M
import rnn_numpy as R


def relu32(v):
    return np.where(v > 0, v, np.float32(0.0)).astype(np.float32)       # NaN and -0 -> +0


def tanh_f64(v):
    """NOT the contract: float64 ``np.tanh`` cast to float32.  Tests re-run the twin with it to show that their probes reach the places
    where ``tanh32`` is its own function (its zero below 2^-25, its exact 1, its last bits)."""
    with np.errstate(all="ignore"):
        return np.tanh(np.asarray(v, np.float32).astype(np.float64)).astype(np.float32)


ACTIVATIONS = {"relu": relu32, "tanh": R.tanh32}


def raw_forward(params, widths, x, activation="tanh", fma=M.fmaf32):
    """float32 [n, widths[-1]]: the head layer's outputs of rows ``x`` [n, widths[0]] under one weight set.  ``activation`` is ``"relu"``,
    ``"tanh"`` or a function float32 array -> float32 array (a wrong one, for the tests that show their inputs matter)."""
    act = ACTIVATIONS[activation] if isinstance(activation, str) else activation
    h = np.asarray(x, np.float32)
    assert h.shape[1] == widths[0]
    ls = M.layers(np.asarray(params, np.float32), widths)
    for l, (W, b) in enumerate(ls):
        acc = np.broadcast_to(b, (h.shape[0], W.shape[1])).astype(np.float32)
        for k in range(W.shape[0]):
            acc = fma(h[:, k:k + 1], W[k][None, :], acc)
        if l + 1 < len(ls):
            with np.errstate(all="ignore"):
                acc = np.asarray(act(acc), np.float32)
        h = acc
    return h


def forward(params, widths, x, head, lo=None, hi=None, activation="tanh", fma=M.fmaf32):
    return M.head_of(raw_forward(params, widths, x, activation, fma), head, lo, hi)


def _per_set(fn, params, x, envs_per_set, env_first):
    sets = (env_first + np.arange(x.shape[0])) // envs_per_set
    out = None
    for s in np.unique(sets):
        r = fn(params[s], x[sets == s])
        if out is None:
            out = np.zeros((x.shape[0],) + r.shape[1:], r.dtype)
        out[sets == s] = r
    return out


def population(params, widths, x, head, lo, hi, envs_per_set, env_first=0, activation="tanh", fma=M.fmaf32):
    """``forward`` of a population: row e of ``x`` under set (env_first + e) // envs_per_set of ``params`` [n_sets, param_count] (the
    mapping of ``mlp_numpy.population``)."""
    return _per_set(lambda p, xs: forward(p, widths, xs, head, lo, hi, activation, fma), params, x, envs_per_set, env_first)


def population_raw(params, widths, x, envs_per_set, env_first=0, activation="tanh", fma=M.fmaf32):
    """The raw heads y [n, widths[-1]] of a population (what ``sample()`` records as ``head``)."""
    return _per_set(lambda p, xs: raw_forward(p, widths, xs, activation, fma), params, x, envs_per_set, env_first)


# ---------------------------------------------------------------- constructed rows: the edges of tanh32 that reach the output
F = np.float32
EDGE_H = 70                                # hidden width of the constructed nets: five neuron blocks, the last one partial
EDGE_UNITS = ((3, 0, 5, 16), (64, 21, 70, 37), (177, 69, 179, 68))     # (input column, hidden unit) of y_0's probe, then of y_1's, by row % 3
EDGE_INF = (100, 40, 101, 55)              # the same for the probes that a large weight makes infinite


def _near(v):
    v = F(v)
    return [np.nextafter(v, F(0)), v, np.nextafter(v, F(np.inf))]


def edge_probes():
    """[(class, |v| float32)]: the arguments of tanh32 whose results the constructed nets carry to the head.
      tiny   0, 2^-149, 1e-8, 2^-24: tanh32 is 0 up to 2^-26 (the accepted cancellation), a correctly rounded tanh is the argument;
      one    both sides of 8.66434, where tanh32 first returns exactly 1, and on to 9.02 (a correctly rounded tanh reaches 1 at 13 ln 2);
      tie    x = -m / 2 for float32 m whose float32 product m * log2(e) is exactly n + 0.5, n = -1 .. -12 -- rintf decides by its
             ties-to-even rule -- and the float32 on either side of each;
      range  1e30, and infinity (1e30 through a weight of 1e30): exactly 1, no NaN from the clamp at -86;
      nan    one NaN."""
    out = [("tiny", F(0.0)), ("tiny", F(2.0 ** -149)), ("tiny", F(1e-8)), ("tiny", F(2.0 ** -24))]
    first_one = F(8.66434)
    assert R.tanh32(first_one) == 1 and R.tanh32(np.nextafter(first_one, F(0))) < 1
    out += [("one", v) for v in _near(first_one)] + [("one", F(v)) for v in (8.5, 8.8, 9.0, 9.02)]
    ties = 0
    for n in range(-1, -13, -1):
        m0 = F((n + 0.5) / np.float64(R.LOG2E))
        for m in _near(m0):
            if F(m * R.LOG2E) == F(n + 0.5):
                out += [("tie", v) for v in _near(F(m / F(-2.0)))]
                ties += 1
                break
    assert ties >= 6, ties
    return out + [("range", F(1e30)), ("range", F(np.inf)), ("nan", F(np.nan))]


def edge_case(w0):
    """(widths, params [2, count], x [2 R, w0], classes [R]): Box(2) nets (w0, EDGE_H, 2), R = len(edge_probes()) rows a set.
    Set 0: zero biases, zero first-layer weights but one-hot 1.0 entries, so that in row r the hidden pre-activation of one unit is exactly
    +v_r and of another exactly -v_r (units and input columns change with r % 3: three neuron blocks, both k-chunks); the head gives each
    of the two a weight of 0.5 into y_0 and y_1: y = (0.5 * tanh32(v), 0.5 * tanh32(-v)), inside (-1, 1), so the float64 Box map keeps
    every bit.  Infinity is 1e30 * 1e30 on units of its own; the NaN row is NaN throughout (NaN * 0).
    Set 1: every first-layer weight and bias is -0 and the inputs are >= 0, so every hidden pre-activation is -0; with head weights 0.5
    and a head bias of -0 the head is -0 exactly where the activation keeps the sign, +0 where it does not."""
    probes = edge_probes()
    rows = len(probes)
    widths = (w0, EDGE_H, 2)
    p = np.zeros((2, M.param_count(widths)), F)
    x = np.zeros((2 * rows, w0), F)
    (W0, b0), (W1, b1) = M.layers(p[0], widths)
    for qa, ja, qb, jb in EDGE_UNITS + (EDGE_INF,):
        big = (qa, ja, qb, jb) == EDGE_INF
        W0[qa, ja] = W0[qb, jb] = F(1e30) if big else F(1.0)
        W1[ja, 0] = W1[jb, 1] = F(0.5)
    for r, (cls, v) in enumerate(probes):
        qa, ja, qb, jb = EDGE_INF if np.isinf(v) else EDGE_UNITS[r % 3]
        x[r, qa], x[r, qb] = (F(1e30), F(-1e30)) if np.isinf(v) else (v, -v)
    (W0, b0), (W1, b1) = M.layers(p[1], widths)
    W0[:], b0[:], W1[:], b1[:] = F(-0.0), F(-0.0), F(0.5), F(-0.0)
    rng = np.random.default_rng(5)
    x[rows:] = rng.random((rows, w0), dtype=F) * (rng.random((rows, w0)) < 0.7)
    return widths, p, x, [cls for cls, _ in probes]


def first_layer(params, widths, x, fma=M.fmaf32):
    """The pre-activations of the first layer (what the constructed rows pin)."""
    W, b = M.layers(np.asarray(params, F), widths)[0]
    acc = np.broadcast_to(b, (x.shape[0], W.shape[1])).astype(F)
    for k in range(W.shape[0]):
        acc = fma(x[:, k:k + 1], W[k][None, :], acc)
    return acc
