"""numpy twin of the recurrent policy (include/ftl.h, the ftl_rnn_act block) on top of ``mlp_numpy`` and ``collect_numpy`` (which stay as
they are): ``exp32`` / ``sig32`` / ``tanh32`` line by line in float32, the cell input, the gate chain, the cell lines, the head and the
state row with its zero rule.  Everything the device computes is pinned to this bit for bit."""
import numpy as np

import collect_numpy as CN
import mlp_numpy as M

PREV_ACTION, PREV_REWARD = 1, 2
F = np.float32
LOG2E, LN2_HI, LN2_LO = F(float.fromhex("0x1.715476p+0")), F(float.fromhex("0x1.62e400p-1")), F(float.fromhex("0x1.7f7d1cp-20"))
POLY = tuple(F(1.0 / d) for d in (5040, 720, 120, 24, 6, 2, 1, 1))      # the float32 roundings of 1/7! .. 1/0!
assert LN2_HI.view(np.uint32) == 0x3f317200 and LN2_LO.view(np.uint32) == 0x35bfbe8e


def exp32(a):
    """e^a for a <= 0, float32, every line one float32 operation (a below -86, and a NaN, are read as -86)."""
    with np.errstate(all="ignore"):
        a = np.fmax(np.asarray(a, F), F(-86.0))
        s = a * LOG2E
        n = np.rint(s)
        r = M.fmaf32(n, -LN2_HI, a)
        r = M.fmaf32(n, -LN2_LO, r)
        p = np.full_like(r, POLY[0])
        for c in POLY[1:]:
            p = M.fmaf32(p, r, c)
        return np.ldexp(p, n.astype(np.int32)).astype(F)


def exp_libm(a):
    """NOT the contract: float32 e^a through float64 libm.  Tests re-run the twin with it to show that their values tell the two apart."""
    with np.errstate(all="ignore"):
        return np.exp(np.fmax(np.asarray(a, F), F(-86.0)).astype(np.float64)).astype(F)


def sig32(x, exp=exp32):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        e = exp(-np.abs(x))
        d = F(1.0) + e
        r = np.where(x >= 0, F(1.0) / d, e / d).astype(F)
    return np.where(x != x, x, r).astype(F)


def tanh32(x, exp=exp32):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        m = F(-2.0) * np.abs(x)
        e = exp(m)
        a = F(1.0) - e
        b = F(1.0) + e
        r = np.copysign(a / b, x).astype(F)
    return np.where(x != x, x, r).astype(F)


def dims(widths, cell, flags):
    """(P, R, U, S): ``widths`` = the trunk's widths followed by the head width."""
    A = widths[-1]
    P, R = (A if flags & PREV_ACTION else 0), (1 if flags & PREV_REWARD else 0)
    return P, R, widths[-2] + P + R + cell, 2 * cell + P + 1


def param_count(widths, cell, flags):
    U = dims(widths, cell, flags)[2]
    return M.param_count(widths[:-1]) + (U + 1) * 4 * cell + (cell + 1) * widths[-1]


def split(params, widths, cell, flags):
    """(trunk params, W_g [U, 4C], b_g [4C], W_y [C, A], b_y [A]) views of one weight set."""
    U, A, C = dims(widths, cell, flags)[2], widths[-1], cell
    o = M.param_count(widths[:-1])
    Wg = params[o:o + U * 4 * C].reshape(U, 4 * C); o += U * 4 * C
    bg = params[o:o + 4 * C]; o += 4 * C
    Wy = params[o:o + C * A].reshape(C, A); o += C * A
    return params[:M.param_count(widths[:-1])], Wg, bg, Wy, params[o:o + A]


def chain(x, W, b):
    acc = np.broadcast_to(b, (x.shape[0], W.shape[1])).astype(F)
    for k in range(W.shape[0]):
        acc = M.fmaf32(x[:, k:k + 1], W[k][None, :], acc)
    return acc


def relu_trunk(params, widths, x):
    """The trunk ``widths`` (every layer a hidden one) of one set on rows ``x``."""
    h = np.asarray(x, F)
    for W, b in M.layers(np.asarray(params, F), widths):
        acc = chain(h, W, b)
        h = np.where(acc > 0, acc, F(0.0)).astype(F)
    return h


def decide(params, widths, cell, flags, x, state, reward, done_in, head, lo, hi, before=False, out_done=None, noise=None, sigma=None, exp=exp32):
    """One decision of rows ``x`` [n, w0] under ONE weight set: ``state`` [n, S] float32, ``reward`` float64 [n] (out->reward),
    ``done_in`` bool [n] (done on entry: mode AFTER), ``out_done`` bool [n] (mode BEFORE), ``sigma`` [n, A] the env's own row.
    Returns dict(action, head, read [n, S] -- the row as step 1 read it --, state [n, S] -- the row written)."""
    C, A = cell, widths[-1]
    P, R, U, S = dims(widths, cell, flags)
    trunk, Wg, bg, Wy, by = split(np.asarray(params, F), widths, cell, flags)
    read = np.array(state, F)[:, :S].copy()
    if before:
        read[np.asarray(out_done, bool)] = 0
    h, c, ap, live = read[:, :C], read[:, C:2 * C], read[:, 2 * C:2 * C + P], read[:, 2 * C + P]
    xt = relu_trunk(trunk, widths[:-1], x)
    parts = [xt, ap]
    if R:
        with np.errstate(all="ignore"):
            parts.append(np.where(live != 0, np.asarray(reward, np.float64).astype(F), F(0.0)).astype(F)[:, None])
    u = np.concatenate(parts + [h], 1)
    assert u.shape[1] == U
    z = chain(u, Wg, bg)
    with np.errstate(all="ignore"):
        gi, gf, gg, go = sig32(z[:, :C], exp), sig32(z[:, C:2 * C], exp), tanh32(z[:, 2 * C:3 * C], exp), sig32(z[:, 3 * C:], exp)
        t = (gi * gg).astype(F)
        c1 = M.fmaf32(gf, c, t)
        h1 = (go * tanh32(c1, exp)).astype(F)
    y = chain(h1, Wy, by)
    action = CN.sample_head(y, head, lo, hi, noise, sigma)
    if head == M.DISCRETE:
        ap1 = (np.arange(5)[None, :] == action[:, None]).astype(F)
    else:
        with np.errstate(all="ignore"):
            ap1 = np.asarray(action, np.float64).reshape(x.shape[0], -1).astype(F)
    new = np.concatenate([h1, c1, ap1[:, :P], np.ones((x.shape[0], 1), F)], 1)
    if not before:
        new[np.asarray(done_in, bool)] = 0
    return dict(action=action, head=y, read=read, state=new)


def population(params, widths, cell, flags, x, state, reward, done_in, head, lo, hi, envs_per_set, env_first=0, before=False, out_done=None,
               noise=None, sigma=None, exp=exp32):
    """``decide`` of a population: row e under set (env_first + e) // envs_per_set of ``params`` [n_sets, count], ``sigma`` [n_sets, A]."""
    n = x.shape[0]
    sets = (env_first + np.arange(n)) // envs_per_set
    out = None
    for s in np.unique(sets):
        m = sets == s
        r = decide(params[s], widths, cell, flags, x[m], state[m], np.asarray(reward)[m], np.asarray(done_in, bool)[m], head, lo, hi, before,
                   None if out_done is None else np.asarray(out_done, bool)[m], None if noise is None else noise[m],
                   None if sigma is None else np.broadcast_to(np.asarray(sigma, F)[s], (int(m.sum()), widths[-1])), exp)
        if out is None:
            out = {k: np.zeros((n,) + v.shape[1:], v.dtype) for k, v in r.items()}
        for k, v in r.items():
            out[k][m] = v
    return out


def f64_forward(params, widths, cell, flags, x, state, reward):
    """NOT the contract: the same net in float64 with libm, rows fresh or live as ``state`` says; the head [n, A] and the new (h, c).  The
    measure of what float32 and the fixed transcendentals cost."""
    C = cell
    P, R, U, S = dims(widths, cell, flags)
    trunk, Wg, bg, Wy, by = (np.asarray(v, np.float64) for v in split(np.asarray(params, F), widths, cell, flags))
    h = np.asarray(x, np.float64)
    for W, b in M.layers(trunk, widths[:-1]):
        h = np.maximum(h @ W + b, 0.0)
    st = np.asarray(state, np.float64)
    parts = [h, st[:, 2 * C:2 * C + P]]
    if R:
        parts.append(np.where(st[:, 2 * C + P] != 0, np.asarray(reward, np.float64), 0.0)[:, None])
    z = np.concatenate(parts + [st[:, :C]], 1) @ Wg + bg
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))
    c1 = sg(z[:, C:2 * C]) * st[:, C:2 * C] + sg(z[:, :C]) * np.tanh(z[:, 2 * C:3 * C])
    h1 = sg(z[:, 3 * C:]) * np.tanh(c1)
    return h1 @ Wy + by, h1, c1


def edge_values():
    """float32 values for the transcendentals: +-0, subnormals, +-1e-3, the rintf ties a * log2e = -(m + 0.5), +-43, +-86, +-87, +-1e30,
    +-inf and NaN."""
    v = [0.0, 1e-3, 43.0, 86.0, 87.0, 1e30, np.inf, 2.0 ** -149, 2.0 ** -127, 3 * 2.0 ** -140, 1.0, 0.5, 88.0, 20.0, 2.0 ** -24, 2.0 ** -12]
    ties = []
    for m in range(0, 124):
        t = F(F(m + 0.5) / LOG2E)
        ties += [t, np.nextafter(t, F(0)), np.nextafter(t, F(np.inf)), F(t / F(2.0))]      # sig32 sees a = -x, tanh32 a = -2x
    v = np.concatenate([np.asarray(v, F), np.asarray(ties, F)])
    return np.concatenate([v, -v, np.asarray([np.nan], F)]).astype(F)
