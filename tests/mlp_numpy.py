"""numpy twin of the MLP policy (include/ftl.h, the ftl_mlp_act block): the float32 fused multiply-add without math.fma, the forward pass
neuron by neuron in k order, and the three heads.  Everything the device computes is pinned to this bit for bit."""
import numpy as np

BOX2, DISCRETE, TURN = 0, 1, 2


def fmaf32(a, b, c):
    """Correctly rounded float32 ``a * b + c`` (one rounding), elementwise.  The product of two float32 is exact in float64; ``c`` is added
    in float64 with the TwoSum error term; where that error is non-zero and the sum's last mantissa bit is even the sum moves one float64
    towards the error (round to odd), so the cast to float32 cannot round twice."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                          # p + c = s + e exactly (finite s)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def fma_f64sum(a, b, c):
    """NOT the contract: the float64 product and sum cast to float32 -- it rounds twice, and gets a tie the third operand decides wrong.
    Tests re-run the twin with it to show that their rows reach such a tie."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        return (a * b + c).astype(np.float32)


def _flush(v):
    v = np.asarray(v, np.float32)
    return np.where(np.abs(v) < np.float32(2.0 ** -126), np.float32(0.0), v).astype(np.float32)


def fma_flush(a, b, c):
    """NOT the contract: ``fmaf32`` on a machine that flushes float32 subnormal operands and results to zero.  Tests re-run the twin with
    it to show that their rows depend on subnormals being kept."""
    return _flush(fmaf32(_flush(a), _flush(b), _flush(c)))


def param_count(widths):
    return sum((a + 1) * b for a, b in zip(widths[:-1], widths[1:]))


def layers(params, widths):
    """[(W [in, out], b [out])] views of one weight set."""
    out, off = [], 0
    for a, b in zip(widths[:-1], widths[1:]):
        out.append((params[off:off + a * b].reshape(a, b), params[off + a * b:off + a * b + b]))
        off += (a + 1) * b
    return out


def raw_forward(params, widths, x, fma=fmaf32):
    """float32 [n, widths[-1]]: the head layer's outputs y of rows ``x`` [n, widths[0]] under one weight set (``fma``: the contract's
    ``fmaf32``, or one of the wrong arithmetics above)."""
    h = np.asarray(x, np.float32)
    assert h.shape[1] == widths[0]
    ls = layers(np.asarray(params, np.float32), widths)
    for l, (W, b) in enumerate(ls):
        acc = np.broadcast_to(b, (h.shape[0], W.shape[1])).astype(np.float32)
        for k in range(W.shape[0]):
            acc = fma(h[:, k:k + 1], W[k][None, :], acc)
        if l + 1 < len(ls):
            acc = np.where(acc > 0, acc, np.float32(0.0)).astype(np.float32)       # NaN and -0 -> +0
        h = acc
    return h


def box_head(y, lo, hi):
    lo, hi = np.float64(lo), np.float64(hi)
    u = np.fmin(np.fmax(np.asarray(y, np.float32).astype(np.float64), -1.0), 1.0)
    s = (u + 1.0) * 0.5
    a = lo + s * (hi - lo)
    return np.fmin(np.fmax(a, lo), hi)


def discrete_head(y):
    y = np.asarray(y, np.float32)
    k = np.zeros(y.shape[0], np.int32)
    rows = np.arange(y.shape[0])
    with np.errstate(invalid="ignore"):
        for j in range(1, 5):
            k = np.where(y[:, j] > y[rows, k], np.int32(j), k).astype(np.int32)
    return k


def head_of(y, head, lo, hi):
    """The encoded action of head outputs ``y`` [n, w]: ``lo`` / ``hi`` are the config's action_low / action_high."""
    if head == DISCRETE:
        return discrete_head(y)
    if head == BOX2:
        return np.stack([box_head(y[:, 0], lo[0], hi[0]), box_head(y[:, 1], lo[1], hi[1])], 1)
    return box_head(y[:, 0], lo[-1], hi[-1])


def forward(params, widths, x, head, lo=None, hi=None, fma=fmaf32):
    return head_of(raw_forward(params, widths, x, fma), head, lo, hi)


def population(params, widths, x, head, lo, hi, envs_per_set, env_first=0, fma=fmaf32):
    """``forward`` of a population: row e of ``x`` under set (env_first + e) // envs_per_set of ``params`` [n_sets, param_count]."""
    sets = (env_first + np.arange(x.shape[0])) // envs_per_set
    out = None
    for s in np.unique(sets):
        r = forward(params[s], widths, x[sets == s], head, lo, hi, fma)
        if out is None:
            out = np.zeros((x.shape[0],) + r.shape[1:], r.dtype)
        out[sets == s] = r
    return out


def bounds(cfg):
    """(lo, hi) of the head map for a config: action_low / action_high (None for Discrete(5))."""
    if cfg.discrete_action_space:
        return None, None
    return np.array(cfg.action_low, np.float64), np.array(cfg.action_high, np.float64)


def head_kind(cfg):
    return DISCRETE if cfg.discrete_action_space else TURN if cfg.constant_follower_speed else BOX2


def nasty_inputs(rng, n, w):
    """float32 [n, w] rows for the act tests: uniform values, exact 0 and 1, the double-rounding operands, subnormals and negatives."""
    x = rng.random((n, w), dtype=np.float32)
    x[rng.random((n, w)) < 0.15] = 0.0
    x[rng.random((n, w)) < 0.10] = 1.0
    x[rng.random((n, w)) < 0.05] = np.float32(1 + 2.0 ** -12)
    sub = rng.random((n, w)) < 0.03
    x[sub] = (rng.integers(1, 1 << 20, int(sub.sum())).astype(np.float32) * np.float32(2.0 ** -149))
    neg = rng.random((n, w)) < 0.05
    x[neg] = -x[neg]
    return x


def nasty_params(rng, n_sets, widths, scale=1.0):
    """Normal-random float32 [n_sets, param_count] with double-rounding operands, tiny and subnormal values sprinkled in."""
    p = (rng.standard_normal((n_sets, param_count(widths))) * scale).astype(np.float32)
    big = rng.random(p.shape) < 0.01
    p[big] = np.float32(1 + 2.0 ** -12) * np.where(rng.random(int(big.sum())) < 0.5, np.float32(-1), np.float32(1))
    p[rng.random(p.shape) < 0.02] = np.float32(2.0 ** -60)
    p[rng.random(p.shape) < 0.02] = np.float32(-2.0 ** -60)
    p[rng.random(p.shape) < 0.01] = np.float32(2.0 ** -140)
    return p


# ---------------------------------------------------------------- constructed rows: ties and subnormals that reach the output
A_TIE = np.float32(1 + 2.0 ** -12)      # A_TIE * A_TIE = 1 + 2^-11 + 2^-24: exactly half way between two float32
ROWS = 8                                # envs of every set of the constructed cases


def _sub(m):
    """The float32 subnormal m * 2^-149."""
    return (np.asarray(m, np.float64) * 2.0 ** -149).astype(np.float32)


def tie_case(w0):
    """(widths, params [4, count], x [32, w0]): Box(2) nets (w0, 6, 2) whose two head outputs are chains b + A_TIE * A_TIE - 0.5 * 1 with
    b = +2^-60 and b = -2^-60: the product is a float32 tie, the bias decides it, and y = 0.5 + 2^-11 (+ 2^-23) lies inside (-1, 1), so the
    action carries the last bit.  Set 0 (and set 3 with the signs swapped): the tie in the first layer, at k = 0, 2, 5, 62, 64, 120 and
    w0 - 2 in turn (row 7: no tie) -- every lane position of the matrix instruction, both sides of a k-chunk boundary.  Set 1: in the second
    layer at k = 2, 3 (its input is 6 wide: the matrix instruction's part).  Set 2: there at k = 4, 5 (the w_in % 4 rows done by fmaf)."""
    widths = (w0, 6, 2)
    p = np.zeros((4, param_count(widths)), np.float32)
    x = np.zeros((4 * ROWS, w0), np.float32)
    pos = [0, 2, 5, 62, 64, 120, w0 - 2]
    tiny = np.float32(2.0 ** -60)
    for s, sign in ((0, 1), (3, -1)):
        (W0, b0), (W1, b1) = layers(p[s], widths)
        for j, sg in ((0, sign), (1, -sign)):
            b0[j] = sg * tiny
            for q in pos:
                W0[q, j], W0[q + 1, j] = A_TIE, -0.5
            W1[j, j] = 1.0
        for r, q in enumerate(pos):
            x[s * ROWS + r, q], x[s * ROWS + r, q + 1] = A_TIE, 1.0
        x[s * ROWS + 7, 1] = 1.0
    for s, (ka, kb) in ((1, (2, 3)), (2, (4, 5))):
        (W0, b0), (W1, b1) = layers(p[s], widths)
        W0[10, ka], W0[11, kb] = 1.0, 1.0                       # hidden ka = x[10], hidden kb = x[11]
        for j, sg in ((0, 1), (1, -1)):
            b1[j] = sg * tiny
            W1[ka, j], W1[kb, j] = A_TIE, -0.5
        x[s * ROWS:(s + 1) * ROWS, 10] = A_TIE
        x[s * ROWS:(s + 1) * ROWS, 11] = np.where(np.arange(ROWS) % 2 == 0, 1.0, 0.5)
    return widths, p, x


def subnormal_case(w0):
    """(widths, params [4, count], x [32, w0]): Box(2) nets (w0, 6, 6, 2) in which a float32 subnormal appears in the first layer and is
    scaled back by power-of-two weights (2^100 in the second layer, +-2^28 in the head), so that y = +-m * 2^-21 with the subnormal's own
    integer m: a flush anywhere gives 0.  Set 0: subnormal x (second layer through the matrix instruction, k = 1).  Set 1: subnormal W
    (second layer through the w_in % 4 rows, k = 5).  Set 2: a subnormal bias and a running sum that stays subnormal from k = 0 to the
    end, with a subnormal product of two normal operands and a subnormal x added on the way (k = 2).  Set 3: a subnormal result of
    normal operands (k = 4)."""
    widths = (w0, 6, 6, 2)
    p = np.zeros((4, param_count(widths)), np.float32)
    x = np.zeros((4 * ROWS, w0), np.float32)
    r = np.arange(ROWS)
    m = (1 << 19) + 37 * r + 1
    m0 = (1 << 16) + 3

    def wire(s, k):                                             # hidden k -> * 2^100 -> * +-2^28 -> the two head outputs
        (W0, b0), (W1, b1), (W2, b2) = layers(p[s], widths)
        W1[k, 0] = np.float32(2.0 ** 100)
        W2[0, 0], W2[0, 1] = np.float32(2.0 ** 28), np.float32(-2.0 ** 28)
        return W0, b0
    W0, b0 = wire(0, 1)
    W0[3, 1] = 1.0
    x[0 * ROWS + r, 3] = _sub(m)
    W0, b0 = wire(1, 5)
    W0[7, 5] = _sub(m0)
    x[1 * ROWS + r, 7] = (1 + r).astype(np.float32)
    W0, b0 = wire(2, 2)
    b0[2] = _sub(m0)
    W0[20, 2], W0[130, 2] = np.float32(2.0 ** -45), 1.0
    x[2 * ROWS + r, 20] = np.float32(2.0 ** -100)
    x[2 * ROWS + r, 130] = _sub(m)
    W0, b0 = wire(3, 4)
    W0[9, 4] = np.float32(2.0 ** -40)
    x[3 * ROWS + r, 9] = ((8 + r) * 2.0 ** -103).astype(np.float32)
    return widths, p, x
