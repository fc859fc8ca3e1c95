"""numpy twin of the recurrent net on a recorded sequence (include/ftl.h: ftl_rnn_forward), built from the pieces of ``rnn_numpy`` (which
stays as it is): ``split`` / ``chain`` / ``relu_trunk`` / ``sig32`` / ``tanh32``.  Block b is a decision of ``rnn_numpy.decide`` without a
head map; the row block b + 1 reads comes from the record (``action[b]``, ``reward[b]``) and is all zeros where ``kind[b]`` is VOID.  The
switches build deliberately WRONG variants, which the tests use to show that their inputs can see each rule.  Also the synthetic records
the CPU and GPU tests share, with the assertions that the patterns the zero rule lives on are present in them."""
import numpy as np

import mlp_numpy as M
import rnn_numpy as R

F = np.float32
STEP, TERMINATED, TRUNCATED, VOID = 0, 1, 2, 3


def _a_prev(action, A, P, n):
    """``(float)`` of a block of recorded actions as the cell input has it: Box heads the float64 values, Discrete(5) the one-hot of the
    index (zeros for an index outside 0 .. 4)."""
    if not P:
        return np.zeros((n, 0), F)
    if A == 5:
        return (np.arange(5)[None, :] == np.asarray(action)[:, None]).astype(F)
    with np.errstate(all="ignore"):
        return np.asarray(action, np.float64).reshape(n, -1).astype(F)[:, :P]


def forward_set(params, widths, cell, flags, obs, state, action, reward, kind, reward0, wipe=True, gate_reward=True, exp=R.exp32):
    """The sequence ``obs`` [B, n, w0] under ONE weight set from ``state`` [n, S].  Returns dict(head [B, n, A], h [B, n, C], read
    [B, n, S] -- the row every block read).  ``wipe=False``: no zeros after a VOID row; ``gate_reward=False``: r_prev is fed whatever
    ``live`` is; ``exp``: the exponential of the gates (``rnn_numpy.exp_libm`` is the wrong one)."""
    C, A = cell, widths[-1]
    P, Rw, U, S = R.dims(widths, cell, flags)
    B, n = obs.shape[:2]
    trunk, Wg, bg, Wy, by = R.split(np.asarray(params, F), widths, cell, flags)
    xt = R.relu_trunk(trunk, widths[:-1], np.asarray(obs, F).reshape(B * n, -1)).reshape(B, n, -1)      # (the trunk does not depend on the state)
    st = np.array(state, F)[:, :S].copy()
    out = dict(head=np.zeros((B, n, A), F), h=np.zeros((B, n, C), F), read=np.zeros((B, n, S), F))
    for b in range(B):
        out["read"][b] = st
        h, c, ap, live = st[:, :C], st[:, C:2 * C], st[:, 2 * C:2 * C + P], st[:, 2 * C + P]
        parts = [xt[b], ap]
        if Rw:
            rew = (np.zeros(n) if reward0 is None else reward0) if b == 0 else reward[b - 1]
            with np.errstate(all="ignore"):
                r32 = np.asarray(rew, np.float64).astype(F)
            parts.append((np.where(live != 0, r32, F(0.0)).astype(F) if gate_reward else r32)[:, None])
        u = np.concatenate(parts + [h], 1)
        assert u.shape[1] == U
        z = R.chain(u, Wg, bg)
        with np.errstate(all="ignore"):
            gi, gf, gg, go = R.sig32(z[:, :C], exp), R.sig32(z[:, C:2 * C], exp), R.tanh32(z[:, 2 * C:3 * C], exp), R.sig32(z[:, 3 * C:], exp)
            t = (gi * gg).astype(F)
            c1 = M.fmaf32(gf, c, t)
            h1 = (go * R.tanh32(c1, exp)).astype(F)
        out["head"][b], out["h"][b] = R.chain(h1, Wy, by), h1
        if b + 1 < B:
            st = np.concatenate([h1, c1, _a_prev(action[b], A, P, n) if P else np.zeros((n, 0), F), np.ones((n, 1), F)], 1)
            if wipe:
                st[np.asarray(kind[b]) == VOID] = 0
    return out


def forward(params, widths, cell, flags, obs, state, action=None, reward=None, kind=None, reward0=None, envs_per_set=None, env_first=0, **variant):
    """``forward_set`` of a population: row r under set (env_first + r) // envs_per_set of ``params`` [n_sets, count]."""
    B, n = obs.shape[:2]
    sets = (env_first + np.arange(n)) // (envs_per_set or n)
    out = None
    for s in np.unique(sets):
        m = sets == s
        r = forward_set(params[s], widths, cell, flags, obs[:, m], state[m], None if action is None else action[:, m],
                        None if reward is None else reward[:, m], None if kind is None else kind[:, m],
                        None if reward0 is None else np.asarray(reward0)[m], **variant)
        if out is None:
            out = {k: np.zeros(v.shape[:1] + (n,) + v.shape[2:], v.dtype) for k, v in r.items()}
        for k, v in r.items():
            out[k][:, m] = v
    return out


def params(seed, n_sets, widths, cell, flags, scale=0.1, nasty=True):
    """The weights of tests/test_gpu_rnn.py: normal draws with the sprinkles of ``mlp_numpy.nasty_params``."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((n_sets, R.param_count(widths, cell, flags))) * scale).astype(F)
    if nasty:
        big = rng.random(p.shape) < 0.01
        p[big] = F(1 + 2.0 ** -12) * np.where(rng.random(int(big.sum())) < 0.5, F(-1), F(1))
        p[rng.random(p.shape) < 0.02] = F(2.0 ** -60)
        p[rng.random(p.shape) < 0.01] = F(2.0 ** -140)
    return p


def random_state(seed, n, S):
    """The state rows of tests/test_gpu_rnn.py (``_random_state``): live 0 and 1, so a non-zero row with live 0 feeds no reward."""
    rng = np.random.default_rng(seed)
    st = (rng.standard_normal((n, S)) * 0.5).astype(F)
    st[:, -1] = (rng.random(n) < 0.5).astype(F)
    return st


def record(seed, B, n, w0, A):
    """A synthetic record of B blocks of n rows, no env behind it: dict(obs [B, n, w0], action [B-1, n(, 2)] in the head's encoding -- on
    Discrete(5) a few indices lie outside 0 .. 4 --, reward f64 [B-1, n], kind u8 [B-1, n] random over the four kinds, reward0 f64 [n])."""
    rng = np.random.default_rng(seed)
    T = max(B - 1, 1)
    obs = np.stack([M.nasty_inputs(rng, n, w0) for _ in range(B)])
    if A == 5:
        action = rng.integers(0, 5, (T, n)).astype(np.int32)
        action[rng.random((T, n)) < 0.1] = 7
        action[rng.random((T, n)) < 0.05] = -1
    else:
        action = rng.standard_normal((T, n, 2) if A == 2 else (T, n)) * 0.7
    reward = rng.standard_normal((T, n)) * 3
    kind = rng.choice(np.array([STEP, TERMINATED, TRUNCATED, VOID], np.uint8), (T, n), p=[0.45, 0.1, 0.1, 0.35])
    return dict(obs=obs, action=action[:B - 1], reward=reward[:B - 1], kind=kind[:B - 1], reward0=rng.standard_normal(n) * 3)


def assert_patterns(rec, state):
    """What a record must hold for the zero rule and the reward gate to show: a VOID at block 0, two VOIDs in a row, a VOID followed by a
    non-VOID (records of at least three blocks), and a non-zero state row with live 0."""
    void = rec["kind"] == VOID
    assert state[(state[:, -1] == 0)].any() and (state[:, -1] == 1).any() and (state[:, -1] == 0).any()
    if void.shape[0] >= 1:
        assert void[0].any() and not void[0].all()
    if void.shape[0] >= 2:
        assert (void[:-1] & void[1:]).any(), "two VOIDs in a row"
        assert (void[:-1] & ~void[1:]).any(), "a VOID followed by a non-VOID"


SYNTHETIC_B = 5


def synthetic(trunk, cell, A, w0, n, n_sets, flags):
    """The inputs of a GPU case of tests/test_gpu_rnn_forward.py, a pure function of its parameters: dict(widths, params [n_sets, count],
    state [n, S] from ``random_state``, rec = ``record`` of SYNTHETIC_B blocks).  The seeds were chosen on the CPU so that
    ``assert_patterns`` holds for every case."""
    widths = (w0,) + tuple(trunk) + (A,)
    S = R.dims(widths, cell, flags)[3]
    seed = 2 + 1000 * cell + 100 * A + 10 * flags + n + w0
    return dict(widths=widths, params=params(seed, n_sets, widths, cell, flags), state=random_state(seed + 1, n, S),
                rec=record(seed + 2, SYNTHETIC_B, n, w0, A))
