"""GPU tests of the recurrent policy (include/ftl.h: ftl_rnn_act, ftl_rollout_rnn, ftl_collect_rnn; ``rnn.RecurrentPolicy``,
``batch.rollout_rnn`` / ``collect_rnn``): one decision against the numpy twin (tests/rnn_numpy.py) bit for bit on both sides of a gate
pass, the transcendentals at their edges, the one-call loops against the loops they replace through episode boundaries with the state's
zero rule, mode BEFORE under same-step reset, the parts of a pipelined batch and the two-stream handle, and the refusals."""
import numpy as np
import pytest
import torch

import mlp_numpy as M
import rnn_numpy as R
from continiousenvironment_follower_leader_amd import abi
from test_gpu_baseline import _fold
from test_gpu_collect import SHORT, TRAJ, _noise, _same_batches, _sigma
from test_gpu_mlp import DEV, EPW, TILE, _in_width, _vec

pytestmark = pytest.mark.gpu

BOTH = R.PREV_ACTION | R.PREV_REWARD
RTRAJ = TRAJ + ("state",)


def _params(seed, n_sets, widths, cell, flags, scale=0.1, nasty=True):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((n_sets, R.param_count(widths, cell, flags))) * scale).astype(np.float32)
    if nasty:                                                      # the sprinkles of mlp_numpy.nasty_params
        big = rng.random(p.shape) < 0.01
        p[big] = np.float32(1 + 2.0 ** -12) * np.where(rng.random(int(big.sum())) < 0.5, np.float32(-1), np.float32(1))
        p[rng.random(p.shape) < 0.02] = np.float32(2.0 ** -60)
        p[rng.random(p.shape) < 0.01] = np.float32(2.0 ** -140)
    return p


def _rnn(env, widths, cell, n_sets=1, seed=0, flags=BOTH, p=None, **kw):
    from continiousenvironment_follower_leader_amd.rnn import RecurrentPolicy
    if p is None:
        p = _params(seed, n_sets, widths, cell, flags, nasty=kw.pop("nasty", True))
    pol = RecurrentPolicy(env, widths, cell, n_sets=n_sets, params=torch.from_numpy(p).to(DEV), prev_action=bool(flags & R.PREV_ACTION),
                          prev_reward=bool(flags & R.PREV_REWARD), **kw)
    return pol, p


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _eq(got, want, nan_aware=False):
    """Bit for bit (a -0 is not a +0); ``nan_aware``: a NaN equals a NaN whatever its payload."""
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want
    got, want = got.detach().cpu(), want.detach().cpu()
    if tuple(got.shape) != tuple(want.shape) or got.dtype != want.dtype:
        return False
    if nan_aware and got.is_floating_point():
        gn, wn = torch.isnan(got), torch.isnan(want)
        return bool(torch.equal(gn, wn)) and bool(torch.equal(_bits(got)[~gn], _bits(want)[~wn]))
    return bool(torch.equal(_bits(got), _bits(want)))


def _random_state(seed, n, S):
    rng = np.random.default_rng(seed)
    st = (rng.standard_normal((n, S)) * 0.5).astype(np.float32)
    st[:, -1] = (rng.random(n) < 0.5).astype(np.float32)           # live 0 and 1: a non-zero row with live 0 feeds no reward
    return st


# ---------------------------------------------------------------- 1. one decision equals the twin
NETS = [((70, 33), 65), ((20,), 128), ((64,), 1), ((33,), 63),     # both sides of a 64-cell pass, the limit, U no multiple of 4
        ((20,), 32), ((20,), 33)]                                 # both sides of the staged width of a pass (128 / 256 columns)


@pytest.mark.parametrize("trunk, cell", NETS, ids=["c65", "c128", "c1", "c63", "c32", "c33"])
@pytest.mark.parametrize("n", [TILE + 1, EPW - 1])
@pytest.mark.parametrize("name, over, A", [("B_s1_chase", None, 2), ("Bcfs_s2_chase", None, 1), ("B_s1_chase", dict(discrete_action_space=True), 5)],
                         ids=["box2", "turn", "discrete"])
def test_decision_equals_the_twin(name, over, A, n, trunk, cell):
    n_sets = 3
    env = _vec(name, n, over=over)
    w0 = _in_width(env)
    widths = (w0,) + trunk + (A,)
    rng = np.random.default_rng(1000 + A + cell)
    x = M.nasty_inputs(rng, n, w0)
    env.policy_obs.copy_(torch.from_numpy(x).to(DEV).view_as(env.policy_obs))
    reward = rng.standard_normal(n) * 3
    env.reward.copy_(torch.from_numpy(reward).to(DEV))
    done_in = np.arange(n) % 4 == 1
    env.state_field("env_int")[:, abi.EI_DONE] = torch.from_numpy(done_in.astype(np.int32)).to(DEV)
    out_done = np.arange(n) % 3 == 2
    env.done.copy_(torch.from_numpy(out_done.astype(np.uint8)).to(DEV))
    lo, hi = M.bounds(env.cfg)
    kind = M.head_kind(env.cfg)
    sg = _sigma(300 + A, n_sets, A)
    sigma = torch.from_numpy(sg).to(DEV)
    nz = _noise(400 + A + cell, (n, A), nan_column=1 if A == 5 else None)
    for flags in (BOTH, 0, R.PREV_ACTION, R.PREV_REWARD):
        pol, p = _rnn(env, widths, cell, n_sets, 100 + A + flags, flags)
        assert (pol.P, pol.R, pol.U, pol.S) == R.dims(widths, cell, flags) and tuple(pol.state.shape) == (n, pol.S)
        st0 = _random_state(500 + cell + flags, n, pol.S)
        rec = torch.empty(n, pol.S, dtype=torch.float32, device=DEV)
        modes = ((None, "next_step"), (nz, "next_step"), (nz, False), (nz, "same_step"), (None, "queue")) if flags == BOTH else ((nz, "next_step"), (None, "sample"))
        for noise, mode in modes:
            before = mode in ("same_step", "queue", "sample")
            pol.auto_reset = mode
            pol.state.copy_(torch.from_numpy(st0).to(DEV))
            rec.fill_(7.0), pol.head.fill_(7.0), pol.obs.fill_(7.0), pol.action.fill_(3)
            got = pol.sample(None if noise is None else torch.from_numpy(noise).to(DEV), None if (noise is None or A == 5) else sigma, state_rec=rec)
            want = R.population(p, widths, cell, flags, x, st0, reward, done_in, kind, lo, hi, n // n_sets, before=before, out_done=out_done,
                                noise=noise, sigma=sg)
            what = (flags, mode, noise is not None)
            assert got is pol.action and _eq(got, want["action"]), what
            assert _eq(pol.head, want["head"]), what
            assert _eq(pol.obs, x), what
            assert _eq(rec, want["read"]), what
            assert _eq(pol.state, want["state"]), what
            if before:
                assert (want["read"][out_done] == 0).all() and (want["state"][:, -1] == 1).all()
            else:
                assert (want["state"][done_in] == 0).all() and (want["state"][~done_in, -1] == 1).all() and _eq(rec, st0)
        # act() is sample() without noise
        pol.auto_reset = "next_step"
        pol.state.copy_(torch.from_numpy(st0).to(DEV))
        a = pol.act().clone()
        s1 = pol.state.clone()
        pol.state.copy_(torch.from_numpy(st0).to(DEV))
        assert torch.equal(pol(None), a) and torch.equal(pol.state, s1)
    env.close()


def test_decision_at_the_limits():
    """Three trunk layers of FTL_MLP_MAX_WIDTH, FTL_RNN_MAX_CELL units and the widest head and a_prev: the most LDS a workgroup asks for
    (125.25 KiB of 160, above the 64 KiB a launch gets without asking), two full gate passes, a 16-row weight chunk."""
    n, cell = TILE + 1, abi.FTL_RNN_MAX_CELL
    env = _vec("B_s1_chase", n, over=dict(discrete_action_space=True))
    W = abi.FTL_MLP_MAX_WIDTH
    widths = (_in_width(env), W, W, W, 5)
    pol, p = _rnn(env, widths, cell, 1, 77, BOTH, nasty=False)
    rng = np.random.default_rng(78)
    x = M.nasty_inputs(rng, n, widths[0])
    env.policy_obs.copy_(torch.from_numpy(x).to(DEV).view_as(env.policy_obs))
    st0 = _random_state(79, n, pol.S)
    pol.state.copy_(torch.from_numpy(st0).to(DEV))
    nz = _noise(80, (n, 5))
    rec = torch.empty(n, pol.S, dtype=torch.float32, device=DEV)
    got = pol.sample(torch.from_numpy(nz).to(DEV), state_rec=rec)
    want = R.population(p, widths, cell, BOTH, x, st0, env.reward.cpu().numpy(), np.zeros(n, bool), M.DISCRETE, None, None, n, noise=nz)
    assert _eq(got, want["action"]) and _eq(pol.head, want["head"]) and _eq(pol.state, want["state"]) and _eq(rec, st0)
    assert len(np.unique(want["action"])) > 1
    env.close()


# ---------------------------------------------------------------- 2. the gates at the edges of exp32 / sig32 / tanh32
def test_gate_edges():
    """Zero gate weights and a chosen b_g make z the edge values of the CPU list (tests/rnn_numpy.py: edge_values), every one of them
    through each of the four gates' places.  The twin re-run with libm's exp must differ; the device must equal the exact twin."""
    cell, per = 128, 2
    edges = R.edge_values()
    n_sets = 4 * -(-edges.size // (4 * cell))                      # each set holds 4 * cell values; 4 rotations put every value in every gate
    n = n_sets * per
    env = _vec("B_s1_chase", n)
    widths = (_in_width(env), 8, 2)
    pol, p = _rnn(env, widths, cell, n_sets, 7, BOTH, nasty=False)
    Wg, bg = pol.cell_weights()
    Wg.zero_()
    pad = np.concatenate([edges, np.resize(edges[::-1], n_sets // 4 * 4 * cell - edges.size)])
    for s in range(n_sets):
        block = pad.reshape(n_sets // 4, 4 * cell)[s // 4]
        bg[s].copy_(torch.from_numpy(np.roll(block, (s % 4) * cell)).to(DEV))
    p = pol.params.cpu().numpy()
    x = np.random.default_rng(8).random((n, widths[0]), dtype=np.float32)
    env.policy_obs.copy_(torch.from_numpy(x).to(DEV).view_as(env.policy_obs))
    st0 = _random_state(9, n, pol.S)
    st0[:, -1] = 1
    pol.state.copy_(torch.from_numpy(st0).to(DEV))
    reward = env.reward.cpu().numpy()
    lo, hi = M.bounds(env.cfg)
    args = (p, widths, cell, BOTH, x, st0, reward, np.zeros(n, bool), M.BOX2, lo, hi, per)
    exact, libm = R.population(*args), R.population(*args, exp=R.exp_libm)
    z_nan = np.isnan(exact["state"])
    differ = (exact["state"].view(np.uint32) != libm["state"].view(np.uint32)) & ~z_nan
    assert differ[:, :2 * cell].reshape(n_sets, -1).any(1).all(), "the state of every set depends on exp32 being exp32"
    assert z_nan.any() and not z_nan.all(1).any()                  # the NaN bias reaches the state, in its own cells only
    a = pol.act()
    got = pol.state.cpu().numpy()
    print("device vs exact twin: %d of %d state words differ; vs libm's exp: %d" % (
        (got.view(np.uint32) != exact["state"].view(np.uint32))[~z_nan].sum(), got.size, (got.view(np.uint32) != libm["state"].view(np.uint32))[~z_nan].sum()))
    assert _eq(pol.state, exact["state"], nan_aware=True)
    assert _eq(a, exact["action"], nan_aware=True) and _eq(pol.head, exact["head"], nan_aware=True)
    env.close()


# ---------------------------------------------------------------- 3. collect_rnn = the loop it replaces, and the twin replayed on the record
def _loop(env, pol, T, noise, sigma, auto_reset):
    """The loop ``collect_rnn`` replaces: ``sample`` + ``step`` + the record, with the stand-alone calls."""
    rec = {k: [] for k in RTRAJ}
    alive = env.state_field("env_int")[:, abi.EI_DONE].eq(0)
    for t in range(T):
        srec = torch.empty(env.n, pol.S, dtype=torch.float32, device=DEV)
        a = pol.sample(None if noise is None else noise[t], sigma, state_rec=srec)
        rec["obs"].append(pol.obs.clone()), rec["head"].append(pol.head.clone()), rec["action"].append(a.clone()), rec["state"].append(srec)
        env.step(a, auto_reset=auto_reset)
        done = env.done.bool()
        ended = torch.where(env.status[:, 0] == abi.MISSION.index("finished_by_time"), abi.FTL_TR_TRUNCATED, abi.FTL_TR_TERMINATED)
        kind = torch.where(~alive, abi.FTL_TR_VOID, torch.where(done, ended, abi.FTL_TR_STEP)).to(torch.uint8)
        rec["reward"].append(env.reward.clone()), rec["kind"].append(kind)
        alive = ~done
    rec["obs"].append(env.policy_obs.reshape(env.n, -1).clone())
    return {k: torch.stack(v) for k, v in rec.items()}


def test_collect_is_the_loop_and_the_twin():
    from continiousenvironment_follower_leader_amd import mlp
    n, T, sets, widths, cell = 2 * TILE + 2, 12, 2, (180, 70, 33, 2), 65
    env, ref = _vec("B_s1_chase", n, over=SHORT), _vec("B_s1_chase", n, over=SHORT)
    pol, p = _rnn(env, widths, cell, sets, 500, nasty=False)
    pref, _ = _rnn(ref, widths, cell, sets, p=p)
    noise = torch.from_numpy(np.random.default_rng(501).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    sg = _sigma(502, sets, 2)
    sigma = torch.from_numpy(sg).to(DEV)
    for b, q in ((env, pol), (ref, pref)):
        b.step(q.act())                                            # envs under way, states live
    r_in = env.reward.cpu().numpy().copy()
    assert bool((pol.state[:, -1] == 1).all()) and torch.equal(pol.state, pref.state)

    tr = env.collect_rnn(pol, T, noise, sigma, record_state=True)
    assert isinstance(tr, mlp.Trajectory) and tuple(tr.state.shape) == (T, n, pol.S) and tr.state.dtype == torch.float32
    want = _loop(ref, pref, T, noise, sigma, "next_step")
    for k in RTRAJ:
        assert _eq(getattr(tr, k), want[k]), k
    _same_batches(env, ref, "collect vs loop")
    assert _eq(pol.state, pref.state)

    kind = tr.kind.cpu().numpy()
    for k in (abi.FTL_TR_STEP, abi.FTL_TR_TRUNCATED, abi.FTL_TR_VOID):
        assert (kind == k).any(), k
    state = tr.state.cpu().numpy()
    void = kind == abi.FTL_TR_VOID
    assert void[:-1].any() and (state[1:][void[:-1]] == 0).all()   # every row read after a VOID row is all zeros
    assert (state[void] != 0).any()                                # ... and the VOID decision itself still read the finished episode's memory
    assert (pol.state.cpu().numpy()[void[-1]] == 0).all()
    first = np.zeros_like(void)
    first[1:] = void[:-1]
    assert (state[~first][:, -1] == 1).all()                       # every other row is live

    # the twin replayed on the record: obs, reward, kind and noise in; head, action and the state chain out
    obs, rew, nz = tr.obs.cpu().numpy(), tr.reward.cpu().numpy(), noise.cpu().numpy()
    lo, hi = M.bounds(env.cfg)
    st = state[0]
    for t in range(T):
        r = R.population(p, widths, cell, BOTH, obs[t], st, r_in if t == 0 else rew[t - 1], void[t], M.BOX2, lo, hi, n // sets, noise=nz[t], sigma=sg)
        assert _eq(tr.head[t], r["head"]) and _eq(tr.action[t], r["action"]) and _eq(tr.state[t], r["read"]), t
        st = r["state"]
    assert _eq(pol.state, st)

    # gae works on the result unchanged; record_state=False keeps block 0; out= reuses the buffers
    values = torch.zeros(T + 1, n, dtype=torch.float32, device=DEV)
    adv, ret = mlp.gae(tr, values, 0.99, 0.95)
    assert tuple(adv.shape) == (T, n) and bool((adv[tr.kind == abi.FTL_TR_VOID] == 0).all())
    s_in = pol.state.clone()
    tr1 = env.collect_rnn(pol, 3, noise[:3], sigma)
    assert tuple(tr1.state.shape) == (1, n, pol.S) and torch.equal(tr1.state[0], s_in)
    ptr = tr1.state.data_ptr()
    assert env.collect_rnn(pol, 3, noise[:3], sigma, out=tr1) is tr1 and tr1.state.data_ptr() == ptr
    env.close(), ref.close()


# ---------------------------------------------------------------- 4. further identities
def test_rollout_is_the_loop_and_collect_without_reset():
    n, T, gamma, widths, cell = TILE + 3, 6, 0.97, (180, 70, 33, 2), 65
    envs = [_vec("B_s1_chase", n, over=SHORT) for _ in range(3)]
    pols = [_rnn(e, widths, cell, 1, 700, nasty=False)[0] for e in envs]
    for e, q in zip(envs, pols):
        e.step(q.act())
    a, b, c = envs
    r = a.rollout_rnn(pols[0], T, gamma=gamma, record=True)
    assert len(r) == 4 and r[0] is a.rollout_ret and tuple(r[3].shape) == (T, n, 2)
    played = []

    def step(t):
        played.append(pols[1].act().clone())
        b.step(played[-1])
    ro = _fold(b, T, gamma, step)
    for x, y in zip(r[:3], ro):
        assert torch.equal(x, y)
    assert torch.equal(torch.stack(played), r[3])
    _same_batches(a, b, "rollout vs loop")
    assert _eq(pols[0].state, pols[1].state)
    steps = r[1]
    assert 0 < int((steps < T).sum())                               # episodes end inside the window: their rows are wiped
    assert bool((pols[0].state[steps < T] == 0).all()) and bool((pols[0].state[steps == T, -1] == 1).all())
    tr = c.collect_rnn(pols[2], T, auto_reset=False)
    assert torch.equal(tr.action, r[3]) and _eq(pols[2].state, pols[0].state)
    _same_batches(a, c, "rollout vs collect(flags 0)")
    assert torch.equal(steps.cpu(), (tr.kind != abi.FTL_TR_VOID).sum(0).to(torch.int32).cpu())
    fit = pols[0].fitness()
    assert tuple(fit.shape) == (1,) and len(a.rollout_rnn(pols[0], 2)) == 3
    for e in envs:
        e.close()


def test_a_terminated_episode():
    """Scenario 8 of config B ends in the first step with mission status FAIL under the constant action (max_speed, +max_rotation_speed)
    (tests/test_gpu_collect.py).  A net with zero weights and a head bias of (10, 10) plays it whatever it observes and remembers."""
    n, T = 40, 3
    env = _vec("B_s1_chase", n)
    pol, _ = _rnn(env, (180, 8, 2), 8, 1, 0, nasty=False)
    pol.params.zero_()
    pol.head_weights()[1][:] = 10.0
    tr = env.collect_rnn(pol, T, record_state=True)
    hi = torch.tensor(env.cfg.action_high, dtype=torch.float64, device=DEV)
    assert bool((tr.action == hi).all())
    kind = tr.kind.cpu()
    assert kind[:, 8].tolist() == [abi.FTL_TR_TERMINATED, abi.FTL_TR_VOID, abi.FTL_TR_STEP]
    live = tr.state[:, 8, -1].tolist()
    assert live == [0.0, 1.0, 0.0] and float(pol.state[8, -1]) == 1.0          # fresh, the void decision, fresh again
    assert tr.state[1, 8, -3:-1].tolist() == [float(np.float32(hi[0].item())), float(np.float32(hi[1].item()))]       # a_prev = (float)action
    env.close()


# ---------------------------------------------------------------- 5. mode BEFORE under same-step reset
def test_mode_before_under_same_step_reset():
    n, T, sets, widths, cell = TILE + 3, 8, 1, (180, 33, 2), 63
    env = _vec("B_s1_chase", n, over=SHORT, final_obs=True)
    pol, p = _rnn(env, widths, cell, sets, 900, nasty=False, auto_reset="same_step")
    lo, hi = M.bounds(env.cfg)
    st = np.zeros((n, pol.S), np.float32)
    resets = 0
    for t in range(T):
        x, rew, done = env.policy_obs.reshape(n, -1).cpu().numpy(), env.reward.cpu().numpy(), env.done.cpu().numpy().astype(bool)
        a = pol()
        r = R.population(p, widths, cell, BOTH, x, st, rew, np.zeros(n, bool), M.BOX2, lo, hi, n, before=True, out_done=done)
        assert _eq(a, r["action"]) and _eq(pol.state, r["state"]), t
        if t and done.any():
            resets += int(done.sum())
            assert (st[done] != 0).any() and (r["read"][done] == 0).all()        # a live memory was there, and was not read
        st = r["state"]
        env.step(a, auto_reset="same_step")
    assert resets >= n
    env.close()


# ---------------------------------------------------------------- 6. pipelined parts and the two-stream handle
def test_pipelined_matches_vec_game():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    n, sets, T, widths, cell = 1045, 5, 6, (180, 33, 2), 65
    a, q = _vec("B_s1_chase", n, over=SHORT), _vec("B_s1_chase", n, cls=PipelinedVecGame, over=SHORT, parts=2)
    lo1 = q.shards[1].lo
    assert lo1 % (n // sets) != 0 and (lo1 - 1) // (n // sets) == lo1 // (n // sets)           # set 2 lies in both parts
    pa, p = _rnn(a, widths, cell, sets, 800, nasty=False)
    pq, _ = _rnn(q, widths, cell, sets, p=p)
    noise = torch.from_numpy(np.random.default_rng(801).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    sigma = torch.from_numpy(_sigma(802, sets, 2)).to(DEV)
    for b, pol in ((a, pa), (q, pq)):
        b.step(pol.act())
    q.join()
    ta, tq = a.collect_rnn(pa, T, noise, sigma, record_state=True), q.collect_rnn(pq, T, noise, sigma, record_state=True)
    q.join()
    for k in RTRAJ:
        assert _eq(getattr(ta, k), getattr(tq, k)), k
    assert bool((ta.kind == abi.FTL_TR_VOID).any()) and bool((ta.kind == abi.FTL_TR_TRUNCATED).any())
    ra, rq = a.rollout_rnn(pa, 4, gamma=0.9, record=True), q.rollout_rnn(pq, 4, gamma=0.9, record=True)
    q.join()
    for x, y in zip(ra, rq):
        assert torch.equal(x, y)
    assert _eq(pa.state, pq.state) and torch.equal(pa.fitness(), pq.fitness())
    _same_batches(a, q, "pipelined")
    a.close(), q.close()


def test_collect_on_a_two_stream_handle(monkeypatch):
    """Config F from 8,192 envs on steps on two streams (tests/test_gpu_collect.py): the decision of step t waits for both halves of step
    t - 1."""
    n, T, widths, cell = 8192 + 37, 5, (360, 32, 2), 32
    trajs, envs, pols = [], [], []
    noise = torch.from_numpy(np.random.default_rng(901).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    sigma = torch.from_numpy(_sigma(902, 1, 2)).to(DEV)
    for split in ("1", "0"):
        monkeypatch.setenv("FTL_SPLIT", split)
        env = _vec("F_s1_chase", n, over=dict(max_steps=100))
        pol, _ = _rnn(env, widths, cell, 1, 900, nasty=False)
        env.step(pol.act())
        trajs.append(env.collect_rnn(pol, T, noise, sigma, record_state=True))
        envs.append(env), pols.append(pol)
    for k in RTRAJ:
        assert _eq(getattr(trajs[0], k), getattr(trajs[1], k)), k
    assert bool((trajs[0].kind == abi.FTL_TR_VOID).any()) and bool((trajs[0].kind == abi.FTL_TR_STEP).any())
    assert _eq(pols[0].state, pols[1].state)
    _same_batches(envs[0], envs[1], "two streams")
    envs[0].close(), envs[1].close()


# ---------------------------------------------------------------- 7. refusals through Python
def test_refusals():
    from continiousenvironment_follower_leader_amd import mlp
    from continiousenvironment_follower_leader_amd.rnn import RecurrentPolicy
    n, T = 6, 2
    env, other = _vec("B_s1_chase", n), _vec("B_s1_chase", n)
    pol, _ = _rnn(env, (180, 8, 2), 8, 2, 1100, nasty=False)
    mpol = mlp.MlpPolicy(env, (180, 8, 2))
    noise, sigma = torch.zeros(T, n, 2, dtype=torch.float32, device=DEV), torch.ones(2, 2, dtype=torch.float32, device=DEV)
    for name in ("collect_rnn", "rollout_rnn"):
        with pytest.raises(ValueError, match="RecurrentPolicy of this batch"):
            getattr(other, name)(pol, T)
        with pytest.raises(ValueError, match="RecurrentPolicy of this batch"):
            getattr(env, name)(mpol, T)
    for bad in (noise[:, :, :1], noise[:1], noise.double(), noise.cpu(), noise.transpose(0, 1)):
        with pytest.raises(ValueError, match="noise"):
            env.collect_rnn(pol, T, bad, sigma)
    for bad in (sigma[:1], sigma.double(), sigma.cpu()):
        with pytest.raises(ValueError, match="sigma"):
            env.collect_rnn(pol, T, noise, bad)
    with pytest.raises(ValueError, match="sigma"):
        env.collect_rnn(pol, T, noise)
    with pytest.raises(ValueError, match="sigma"):
        pol.sample(noise[0])
    with pytest.raises(ValueError, match="state_rec"):
        pol.sample(state_rec=torch.zeros(n, pol.S + 1, dtype=torch.float32, device=DEV))
    for mode in (True, "same_step", "queue", "sample", "never"):
        with pytest.raises(ValueError, match="auto_reset"):
            env.collect_rnn(pol, T, noise, sigma, auto_reset=mode)
    with pytest.raises(ValueError, match="T >= 1"):
        env.collect_rnn(pol, 0)
    with pytest.raises(ValueError, match="T >= 1"):
        env.rollout_rnn(pol, 0)
    tr = env.collect_rnn(pol, T, noise, sigma)
    with pytest.raises(ValueError, match="out.obs"):
        env.collect_rnn(pol, T + 1, out=tr)
    with pytest.raises(ValueError, match="out.state"):
        env.collect_rnn(pol, T, out=tr, record_state=True)
    with pytest.raises(ValueError, match="n_sets"):
        RecurrentPolicy(env, (180, 8, 2), 8, n_sets=4)
    with pytest.raises(ValueError, match="params"):
        RecurrentPolicy(env, (180, 8, 2), 8, params=torch.zeros(1, 5, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="H \\* W"):
        RecurrentPolicy(env, (181, 8, 2), 8)
    lstm = torch.nn.LSTMCell(8 + 2 + 1, 8)
    pol.load_lstm_cell(1, lstm)
    W, b = pol.cell_weights()
    assert torch.equal(W[1, :11].cpu(), lstm.weight_ih.detach().t()) and torch.equal(W[1, 11:].cpu(), lstm.weight_hh.detach().t())
    assert torch.equal(b[1].cpu(), (lstm.bias_ih + lstm.bias_hh).detach())
    with pytest.raises(ValueError, match="inputs"):
        pol.load_lstm_cell(0, torch.nn.LSTMCell(8, 8))
    pol.state.fill_(1.0)
    pol.reset_state([1, 4])
    assert pol.state[[1, 4]].eq(0).all() and pol.state[[0, 2, 3, 5]].eq(1).all()
    pol.reset_state()
    assert bool(pol.state.eq(0).all())
    env.close(), other.close()
