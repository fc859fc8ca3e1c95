"""numpy twin of the backward pass of the recurrent net (include/ftl.h, the ftl_rnn_backward block), built from ``rnn_numpy`` (the
transcendentals, ``split``, ``dims``), ``rnn_seq_numpy`` (the record's encoding, the kinds), ``mlp_numpy.fmaf32`` and the order of
``mlp_backward_numpy``: per weight set, the forward values of ``rnn_seq_numpy.forward_set`` with every intermediate kept, then the blocks
DESCENDING with the contract's lines written out, then the weight gradients summed in the contract's order -- groups of
``max(1, SPAN // B)`` tiles, (tile, block) pairs tile-major with the blocks descending, spans of ``abi.FTL_RNN_BWD_SPAN`` pairs as float32
chains over 32 row slots (+0 in both factors past a cut tile's end), the spans added in float64 and rounded once.  The device is pinned to
this bit for bit (tests/test_gpu_rnn_backward.py).

The switches build deliberately WRONG variants (``no_void_cut``: the carry is not cut at VOID; ``drop_dc_next``: dc_next is dropped;
``two_roundings``: i * (1 - i) in two roundings; ``exp``: libm's exponential), which the tests use to show that their inputs see each
rule.  ``exact=True`` is the same order in float64 with libm: what the contract computes without float32 rounding."""
import numpy as np

import mlp_numpy as M
import rnn_numpy as R
import rnn_seq_numpy as RS
from continiousenvironment_follower_leader_amd import abi

F = np.float32
TILE, SPAN, PASS = abi.FTL_MLP_ENV_TILE, abi.FTL_RNN_BWD_SPAN, abi.FTL_RNN_PASS_CELLS


class _Arith:
    """The contract's operations in float32 (``fmaf32``, ``sig32``, ``tanh32``), or the exact mode's in float64 with libm."""

    def __init__(self, exact, exp):
        self.exact, self.exp, self.T = exact, exp, (np.float64 if exact else F)

    def fma(self, a, b, c):
        with np.errstate(all="ignore"):
            return np.asarray(a, self.T) * np.asarray(b, self.T) + np.asarray(c, self.T) if self.exact else M.fmaf32(a, b, c)

    def mul(self, a, b):
        with np.errstate(all="ignore"):
            return (np.asarray(a, self.T) * np.asarray(b, self.T)).astype(self.T)

    def add(self, a, b):
        with np.errstate(all="ignore"):
            return (np.asarray(a, self.T) + np.asarray(b, self.T)).astype(self.T)

    def sig(self, x):
        with np.errstate(all="ignore"):
            return 1.0 / (1.0 + np.exp(-x)) if self.exact else R.sig32(x, self.exp)

    def tanh(self, x):
        return np.tanh(x) if self.exact else R.tanh32(x, self.exp)

    def chain(self, x, W, b):
        acc = np.broadcast_to(b, (x.shape[0], W.shape[1])).astype(self.T)
        for k in range(W.shape[0]):
            acc = self.fma(x[:, k:k + 1], W[k][None, :], acc)
        return acc


def pass_columns(C):
    """The columns of W_g in the order of the du chain: pass by pass, inside a pass gate by gate, inside a gate the cells ascending."""
    return [q * C + j for j0 in range(0, C, PASS) for q in range(4) for j in range(j0, min(C, j0 + PASS))]


def forward_values(ar, params, widths, cell, flags, obs, state, action, reward, kind, reward0):
    """Per block the values back-propagation needs, under ONE weight set: dict(hs [h_0 .. h_Lt], u, i, f, g, o, c, c1, tc, h1).  In
    float32 they are ``rnn_seq_numpy.forward_set``'s bits (tests/test_rnn_backward_abi.py compares ``h1``)."""
    T, C, A = ar.T, cell, widths[-1]
    P, Rw, U, S = R.dims(widths, cell, flags)
    B, n = obs.shape[:2]
    trunk, Wg, bg, Wy, by = (np.asarray(v, T) for v in R.split(np.asarray(params, F), widths, cell, flags))
    ls = M.layers(trunk, widths[:-1])
    st = np.array(state, F)[:, :S].astype(T)
    out = []
    for b in range(B):
        hs = [np.asarray(obs[b], F).astype(T)]
        for W, bias in ls:
            acc = ar.chain(hs[-1], W, bias)
            hs.append(np.where(acc > 0, acc, T(0.0)).astype(T))
        h, c, ap, live = st[:, :C], st[:, C:2 * C], st[:, 2 * C:2 * C + P], st[:, 2 * C + P]
        parts = [hs[-1], ap]
        if Rw:
            rew = (np.zeros(n) if reward0 is None else reward0) if b == 0 else reward[b - 1]
            with np.errstate(all="ignore"):
                r32 = np.asarray(rew, np.float64).astype(F).astype(T)
            parts.append(np.where(live != 0, r32, T(0.0)).astype(T)[:, None])
        u = np.concatenate(parts + [h], 1)
        assert u.shape[1] == U
        z = ar.chain(u, Wg, bg)
        gi, gf, gg, go = ar.sig(z[:, :C]), ar.sig(z[:, C:2 * C]), ar.tanh(z[:, 2 * C:3 * C]), ar.sig(z[:, 3 * C:])
        c1 = ar.fma(gf, c, ar.mul(gi, gg))
        tc = ar.tanh(c1)
        h1 = ar.mul(go, tc)
        out.append(dict(hs=hs, u=u, i=gi, f=gf, g=gg, o=go, c=c, c1=c1, tc=tc, h1=h1))
        if b + 1 < B:
            st = np.concatenate([h1, c1, RS._a_prev(action[b], A, P, n).astype(T) if P else np.zeros((n, 0), T), np.ones((n, 1), T)], 1)
            st[np.asarray(kind[b]) == RS.VOID] = 0
    return out


def set_grad(params, widths, cell, flags, obs, dhead, state, action=None, reward=None, kind=None, reward0=None, dstate_in=None,
             exact=False, exp=R.exp32, no_void_cut=False, drop_dc_next=False, two_roundings=False):
    """``(grad [param_count], dstate_out [rows, 2C])`` of one weight set whose rows are ``obs`` [B, rows, w0] with head gradients ``dhead``
    [B, rows, A] from ``state`` [rows, S]: float32, or float64 in exact mode."""
    ar = _Arith(exact, exp)
    T, C, A = ar.T, cell, widths[-1]
    P, Rw, U, S = R.dims(widths, cell, flags)
    B, rows = obs.shape[:2]
    wx, Lt = widths[-2], len(widths) - 2
    trunk, Wg, bg, Wy, by = (np.asarray(v, T) for v in R.split(np.asarray(params, F), widths, cell, flags))
    ls = M.layers(trunk, widths[:-1])
    fw = forward_values(ar, params, widths, cell, flags, obs, state, action, reward, kind, reward0)
    cols = pass_columns(C)
    zero = np.zeros((rows, C), T)
    dhn = dcn = zero if dstate_in is None else None
    if dstate_in is not None:
        dhn, dcn = np.asarray(dstate_in, F)[:, :C].astype(T), np.asarray(dstate_in, F)[:, C:].astype(T)
    # per block the (input, delta) pair of every matrix, in the layout's order: the trunk layers, W_g, W_y
    pairs = [None] * B
    for b in range(B - 1, -1, -1):
        v = fw[b]
        dy = np.asarray(dhead[b], F).astype(T)
        dh = np.zeros((rows, C), T)
        for j in range(A):
            dh = ar.fma(Wy[:, j][None, :], dy[:, j:j + 1], dh)
        if b + 1 < B and not no_void_cut:
            void = (np.asarray(kind[b]) == RS.VOID)[:, None]
            dhn, dcn = np.where(void, T(0.0), dhn).astype(T), np.where(void, T(0.0), dcn).astype(T)
        dh = ar.add(dh, dhn)
        one = T(1.0)
        q = ar.mul(dh, v["o"])
        d = ar.fma(-v["tc"], v["tc"], one)
        dc = ar.fma(q, d, zero if drop_dc_next else dcn)
        do = ar.mul(dh, v["tc"])
        di, dg, df, dcn = ar.mul(dc, v["g"]), ar.mul(dc, v["i"]), ar.mul(dc, v["c"]), ar.mul(dc, v["f"])
        ds = (lambda s: ar.mul(s, ar.add(one, -s))) if two_roundings else (lambda s: ar.fma(-s, s, s))
        dz = np.concatenate([ar.mul(di, ds(v["i"])), ar.mul(df, ds(v["f"])), ar.mul(dg, ar.fma(-v["g"], v["g"], one)),
                             ar.mul(do, ds(v["o"]))], 1)
        du = np.zeros((rows, U), T)
        for col in cols:
            du = ar.fma(Wg[:, col][None, :], dz[:, col:col + 1], du)
        dhn = du[:, wx + P + Rw:]
        deltas = [None] * Lt                                   # deltas[l - 1] = delta_l
        deltas[Lt - 1] = np.where(v["hs"][Lt] > 0, du[:, :wx], T(0.0)).astype(T)
        for l in range(Lt, 1, -1):
            W = ls[l - 1][0]
            c = np.zeros((rows, W.shape[0]), T)
            for j in range(W.shape[1]):
                c = ar.fma(W[:, j][None, :], deltas[l - 1][:, j:j + 1], c)
            deltas[l - 2] = np.where(v["hs"][l - 1] > 0, c, T(0.0)).astype(T)
        pairs[b] = [(v["hs"][l], deltas[l]) for l in range(Lt)] + [(v["u"], dz), (v["h1"], dy)]
    # the sums, in the contract's order
    tiles = (rows + TILE - 1) // TILE
    G = max(1, SPAN // B)
    out = []
    for mi in range(Lt + 2):
        K, J = pairs[0][mi][0].shape[1] + 1, pairs[0][mi][1].shape[1]
        total = np.zeros((K, J), np.float64)
        for t0 in range(0, tiles, G):
            order = [(ti, b) for ti in range(t0, min(t0 + G, tiles)) for b in range(B - 1, -1, -1)]
            for s0 in range(0, len(order), SPAN):
                acc = np.zeros((K, J), T)
                for ti, b in order[s0:s0 + SPAN]:
                    a, dl = pairs[b][mi]
                    for r in range(ti * TILE, min((ti + 1) * TILE, rows)):
                        acc = ar.fma(np.concatenate([a[r], [T(1.0)]])[:, None], dl[r][None, :], acc)
                    if (ti + 1) * TILE > rows:
                        acc = ar.add(acc, T(0.0))              # the slots past a cut tile's end, fmaf(+0, +0, acc) each: -0 becomes +0, once is all
                total = total + acc.astype(np.float64)
        out.append(total.astype(T).reshape(-1))
    return np.concatenate(out), np.concatenate([dhn, dcn], 1)


def population_grad(params, widths, cell, flags, obs, dhead, state, action=None, reward=None, kind=None, reward0=None, envs_per_set=None,
                    env_first=0, dstate_in=None, fill=np.nan, **variant):
    """``(grad [n_sets, param_count], dstate_out [n, 2C])``: ``set_grad`` of every set the rows ``obs`` [B, n, w0] touch under the rule
    (env_first + r) // envs_per_set; the rows of untouched sets hold ``fill``."""
    params = np.asarray(params, F)
    B, n = obs.shape[:2]
    sets = (env_first + np.arange(n)) // (envs_per_set or n)
    T = np.float64 if variant.get("exact") else F
    grad, dso = np.full(params.shape, fill, T), np.zeros((n, 2 * cell), T)
    for s in np.unique(sets):
        m = sets == s
        grad[s], dso[m] = set_grad(params[s], widths, cell, flags, obs[:, m], dhead[:, m], state[m], None if action is None else action[:, m],
                                   None if reward is None else reward[:, m], None if kind is None else kind[:, m],
                                   None if reward0 is None else np.asarray(reward0)[m], None if dstate_in is None else dstate_in[m], **variant)
    return grad, dso


def plan(n_blocks, n, envs_per_set, env_first=0):
    """(groups, spans) of ``ftl_rnn_backward`` counted by hand: per touched set the groups of G tiles and, per group, the spans of its
    (tile, block) pairs."""
    sets = (env_first + np.arange(n)) // envs_per_set
    G = max(1, SPAN // n_blocks)
    groups = spans = 0
    for s in np.unique(sets):
        tiles = -(-int((sets == s).sum()) // TILE)
        for t0 in range(0, tiles, G):
            groups += 1
            spans += -(-(min(G, tiles - t0) * n_blocks) // SPAN)
    return groups, spans


def workspace_bytes(widths, cell, flags, n_blocks, n, envs_per_set, env_first=0):
    """``ftl_sizeof_rnn_backward_workspace`` by its formula: the span partials, the record h' | c' of every block, a tile of du per group."""
    groups, spans = plan(n_blocks, n, envs_per_set, env_first)
    U = R.dims(widths, cell, flags)[2]
    return 4 * (spans * R.param_count(widths, cell, flags) + n_blocks * n * 2 * cell + groups * TILE * U)
