"""GPU tests of the trajectory collection (include/ftl.h: ftl_mlp_sample, ftl_collect_mlp, ftl_gae; ``MlpPolicy.sample`` / ``collect``,
``batch.collect_mlp``, ``mlp.gae``): the sampling heads against the numpy twin (tests/collect_numpy.py) bit for bit, the one-call
collection against the loop it replaces through episode boundaries, a terminated episode, the mode without auto-reset against
``rollout_mlp``, the parts of a pipelined batch and the two-stream handle, the advantage kernel against the twin, and the refusals."""
import numpy as np
import pytest
import torch

import collect_numpy as CN
import mlp_numpy as M
from continiousenvironment_follower_leader_amd import abi
from test_gpu_baseline import FIELDS
from test_gpu_mlp import DEV, EPW, OUTP, TILE, _in_width, _policy, _vec

pytestmark = pytest.mark.gpu

SHORT = dict(max_steps=20)        # config B steps 10 frames a call: done is raised by the third step of an episode, the fourth call restarts
TRAJ = ("obs", "head", "action", "reward", "kind")


def _noise(seed, shape, nan_column=None):
    """float32 draws for the sampling tests: normals with zeros, +-large values and (Discrete) a column of NaN mixed in."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(shape).astype(np.float32)
    z[rng.random(shape) < 0.2] = 0.0
    z[rng.random(shape) < 0.05] = np.float32(1e30)
    z[rng.random(shape) < 0.05] = np.float32(-1e30)
    z[rng.random(shape) < 0.03] = np.float32(-0.0)
    if nan_column is not None:
        z[..., ::3, nan_column] = np.nan
    return z


def _sigma(seed, n_sets, A):
    return (np.random.default_rng(seed).random((n_sets, A)) * 0.5 + 0.05).astype(np.float32)


# ---------------------------------------------------------------- 1. sampling equals the twin
@pytest.mark.parametrize("name, over, A", [("B_s1_chase", None, 2), ("Bcfs_s2_chase", None, 1), ("B_s1_chase", dict(discrete_action_space=True), 5)],
                         ids=["box2", "turn", "discrete"])
@pytest.mark.parametrize("n", [TILE + 1, EPW - 1])
def test_sample_equals_the_twin(name, over, A, n):
    n_sets = 3
    env = _vec(name, n, over=over)
    w0 = _in_width(env)
    widths = (w0, 70, 33, A)
    pol, p = _policy(env, widths, n_sets, 100 + A, scale=0.1)
    x = M.nasty_inputs(np.random.default_rng(200 + A), n, w0)
    env.policy_obs.copy_(torch.from_numpy(x).to(DEV).view_as(env.policy_obs))
    lo, hi = M.bounds(env.cfg)
    kind = M.head_kind(env.cfg)
    act = pol.act().clone()
    want_act, want_y = CN.sample_population(p, widths, x, kind, lo, hi, n // n_sets)
    assert torch.equal(act.cpu(), torch.from_numpy(want_act))
    sg = _sigma(300 + A, n_sets, A)
    sigma = torch.from_numpy(sg).to(DEV)
    # NULL noise and a noise of zeros: the bits of ftl_mlp_act; the records are there either way
    pol.sample()
    for noise in (None, torch.zeros(n, A, dtype=torch.float32, device=DEV)):
        pol.head.fill_(7.0), pol.obs.fill_(7.0), pol.action.fill_(3)
        got = pol.sample(noise, sigma)
        assert got is pol.action and torch.equal(got, act)
        assert torch.equal(pol.head.cpu(), torch.from_numpy(want_y))
        assert torch.equal(pol.obs.cpu(), torch.from_numpy(x))                                  # what the kernel read, tile remainder included
    nz = _noise(400 + A, (n, A), nan_column=1 if A == 5 else None)
    got = pol.sample(torch.from_numpy(nz).to(DEV), None if A == 5 else sigma).clone()
    want, _ = CN.sample_population(p, widths, x, kind, lo, hi, n // n_sets, noise=nz, sigma=sg)
    assert got.dtype == act.dtype and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want)), int((got.cpu() != torch.from_numpy(want)).sum())
    assert not torch.equal(got, act)                                                            # the noise reaches the action
    assert torch.equal(pol.head.cpu(), torch.from_numpy(want_y))
    if A == 5:                                                                                  # sigma is ignored on Discrete(5)
        assert torch.equal(pol.sample(torch.from_numpy(nz).to(DEV), torch.from_numpy(_sigma(9, n_sets, A)).to(DEV)), got)
    env.close()


# ---------------------------------------------------------------- 2. one call = the loop it replaces
def _loop(env, pol, T, noise, sigma, auto_reset):
    """The loop ``collect`` replaces: ``sample`` + ``step`` + the record, with today's calls."""
    rec = {k: [] for k in TRAJ}
    alive = env.state_field("env_int")[:, abi.EI_DONE].eq(0)
    for t in range(T):
        a = pol.sample(None if noise is None else noise[t], sigma)
        rec["obs"].append(pol.obs.clone()), rec["head"].append(pol.head.clone()), rec["action"].append(a.clone())
        env.step(a, auto_reset=auto_reset)
        done = env.done.bool()
        ended = torch.where(env.status[:, 0] == abi.MISSION.index("finished_by_time"), abi.FTL_TR_TRUNCATED, abi.FTL_TR_TERMINATED)
        kind = torch.where(~alive, abi.FTL_TR_VOID, torch.where(done, ended, abi.FTL_TR_STEP)).to(torch.uint8)
        rec["reward"].append(env.reward.clone()), rec["kind"].append(kind)
        alive = ~done
    rec["obs"].append(env.policy_obs.reshape(env.n, -1).clone())
    return {k: torch.stack(v) for k, v in rec.items()}


def _same_batches(a, b, what):
    for k in OUTP:
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)
    for k in FIELDS:
        assert torch.equal(a.state_field(k), b.state_field(k)), (what, k)


def test_collect_is_the_loop():
    from continiousenvironment_follower_leader_amd import mlp
    n, T, sets, widths = 2 * TILE + 2, 12, 2, (180, 70, 33, 2)
    env, ref = _vec("B_s1_chase", n, over=SHORT), _vec("B_s1_chase", n, over=SHORT)
    pol, p = _policy(env, widths, sets, 500, scale=0.1, nasty=False)
    pref = mlp.MlpPolicy(ref, widths, params=torch.from_numpy(p).to(DEV), n_sets=sets)
    noise = torch.from_numpy(np.random.default_rng(501).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    sigma = torch.from_numpy(_sigma(502, sets, 2)).to(DEV)
    for b, q in ((env, pol), (ref, pref)):
        b.step(q.act())                                            # envs under way: the first episode of the window is one step short

    tr = env.collect_mlp(pol, T, noise, sigma)
    assert isinstance(tr, mlp.Trajectory) and tr.noise is noise and tr.sigma is sigma
    assert tuple(tr.obs.shape) == (T + 1, n, 180) and tuple(tr.head.shape) == (T, n, 2) and tuple(tr.action.shape) == (T, n, 2)
    assert tr.reward.dtype == torch.float64 and tr.kind.dtype == torch.uint8 and tuple(tr.kind.shape) == (T, n)
    want = _loop(ref, pref, T, noise, sigma, "next_step")
    for k in TRAJ:
        assert torch.equal(getattr(tr, k), want[k]), k
    _same_batches(env, ref, "collect vs loop")

    # the population of transitions this test is about: it fails, it does not skip, if one is missing
    kind = tr.kind.cpu().numpy()
    for k in (abi.FTL_TR_STEP, abi.FTL_TR_TRUNCATED, abi.FTL_TR_VOID):
        assert (kind == k).any(), k
    ends = (kind == abi.FTL_TR_TRUNCATED) | (kind == abi.FTL_TR_TERMINATED)
    assert (ends.sum(0) >= 2).all(), "every env passes at least two episode boundaries"
    assert ((kind == abi.FTL_TR_VOID).sum(0) >= 2).all()
    assert (kind[1:][ends[:-1]] == abi.FTL_TR_VOID).all()          # the call after an ending is the restart
    assert torch.equal(tr.valid, tr.kind != 3) and torch.equal(tr.truncated, tr.kind == 2) and torch.equal(tr.terminated, tr.kind == 1)
    assert bool((tr.reward[tr.kind == abi.FTL_TR_VOID] == 0).all())
    # the restart step's successor is the new episode's first observation: a fresh reset into the scenario the reset window walks to
    t0 = (kind == abi.FTL_TR_VOID).argmax(0)
    nxt = (torch.arange(n) % env.pool.n + n) % env.pool.n
    fresh = _vec("B_s1_chase", n, over=SHORT, scen=nxt)
    got = tr.obs[torch.from_numpy(t0 + 1).to(DEV), torch.arange(n, device=DEV)]
    assert torch.equal(got, fresh.policy_obs.reshape(n, -1))
    assert not torch.equal(got, tr.obs[torch.from_numpy(t0).to(DEV), torch.arange(n, device=DEV)])      # ... and not the terminal one before it
    fresh.close()

    # the advantages of this trajectory, and out= reuses the buffers
    values = torch.from_numpy(np.random.default_rng(503).standard_normal((T + 1, n)).astype(np.float32)).to(DEV)
    adv, ret = mlp.gae(tr, values, 0.99, 0.95)
    wa, wr = CN.gae(tr.reward.cpu().numpy(), kind, values.cpu().numpy(), 0.99, 0.95)
    assert torch.equal(adv.cpu(), torch.from_numpy(wa)) and torch.equal(ret.cpu(), torch.from_numpy(wr))
    ptrs = [getattr(tr, k).data_ptr() for k in TRAJ]
    tr2 = env.collect_mlp(pol, T, noise, sigma, out=tr)
    assert tr2 is tr and ptrs == [getattr(tr, k).data_ptr() for k in TRAJ]
    want2 = _loop(ref, pref, T, noise, sigma, "next_step")
    for k in TRAJ:
        assert torch.equal(getattr(tr, k), want2[k]), ("second window", k)
    env.close(), ref.close()


# ---------------------------------------------------------------- 3. a terminated episode
def test_a_terminated_episode():
    """Found on the CPU with the oracle (oracle_batch.OracleBatch on the pool of seeds 0 .. 63 of config B, env e on scenario e): under the
    constant action (max_speed, +max_rotation_speed) scenario 8 ends in the first step with mission status FAIL, no other scenario ends
    within 12 steps.  A linear net with zero weights and a head bias of (10, 10) plays that action whatever it observes."""
    n, T = 40, 3
    env = _vec("B_s1_chase", n)
    pol, _ = _policy(env, (180, 2), 1, 0, nasty=False)
    pol.params.zero_()
    pol.layer(0)[1][:] = 10.0
    noise = torch.from_numpy(np.random.default_rng(600).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    tr = env.collect_mlp(pol, T, noise, torch.ones(1, 2, dtype=torch.float32, device=DEV))
    hi = torch.tensor(env.cfg.action_high, dtype=torch.float64, device=DEV)
    assert bool((tr.action == hi).all())
    kind = tr.kind.cpu()
    assert kind[:, 8].tolist() == [abi.FTL_TR_TERMINATED, abi.FTL_TR_VOID, abi.FTL_TR_STEP]
    assert int((kind == abi.FTL_TR_TERMINATED).sum()) == 1 and bool(tr.terminated[0, 8]) and not bool(tr.truncated.any())
    env.close()


# ---------------------------------------------------------------- 4. without auto-reset: rollout_mlp with a record
def test_collect_without_auto_reset_is_rollout_mlp():
    n, T = TILE + 3, 6
    env = _vec("B_s1_chase", n, over=SHORT)
    pol, _ = _policy(env, (180, 70, 33, 2), 1, 700, scale=0.1, nasty=False)
    snap = env.snapshot()
    r = env.rollout_mlp(pol, T, record=True)
    acts, steps = r[3].clone(), r[1].clone()
    out = {k: getattr(env, k).clone() for k in OUTP}
    state = {k: env.state_field(k).clone() for k in FIELDS}
    env.restore(snap, slot_stats=True)
    tr = env.collect_mlp(pol, T, auto_reset=False)
    assert tr.noise is None and tr.sigma is None
    assert torch.equal(tr.action, acts)
    for k in OUTP:
        assert torch.equal(getattr(env, k), out[k]), k
    for k in FIELDS:
        assert torch.equal(env.state_field(k), state[k]), k
    kind = tr.kind.cpu().numpy()
    end = (kind != abi.FTL_TR_STEP).argmax(0)                      # the row that ended the env's episode
    rows = np.arange(T)[:, None]
    assert (kind[end, np.arange(n)] == abi.FTL_TR_TRUNCATED).sum() > n // 2 and (end < T - 1).all()
    assert np.isin(kind[end, np.arange(n)], (abi.FTL_TR_TRUNCATED, abi.FTL_TR_TERMINATED)).all()
    assert (kind[rows < end[None]] == abi.FTL_TR_STEP).all() and (kind[rows > end[None]] == abi.FTL_TR_VOID).all()      # every later row is VOID
    assert torch.equal(steps.cpu(), torch.from_numpy((kind != abi.FTL_TR_VOID).sum(0).astype(np.int32)))
    env.close()


# ---------------------------------------------------------------- 5. pipelined parts and the two-stream handle
def _collect_all(env, pol, T, noise, sigma):
    tr = env.collect_mlp(pol, T, noise, sigma)
    if hasattr(env, "join"):
        env.join()
    return tr


def test_pipelined_matches_vec_game():
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    n, sets, T, widths = 1045, 5, 6, (180, 70, 33, 2)
    a, p = _vec("B_s1_chase", n, over=SHORT), _vec("B_s1_chase", n, cls=PipelinedVecGame, over=SHORT, parts=2)
    lo1 = p.shards[1].lo
    assert lo1 % (n // sets) != 0 and (lo1 - 1) // (n // sets) == lo1 // (n // sets)           # set 2 lies in both parts
    pa, params = _policy(a, widths, sets, 800, scale=0.1, nasty=False)
    pp = MlpPolicy(p, widths, params=torch.from_numpy(params).to(DEV), n_sets=sets)
    noise = torch.from_numpy(np.random.default_rng(801).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    sigma = torch.from_numpy(_sigma(802, sets, 2)).to(DEV)
    ta, tp = _collect_all(a, pa, T, noise, sigma), _collect_all(p, pp, T, noise, sigma)
    for k in TRAJ:
        assert torch.equal(getattr(ta, k), getattr(tp, k)), k
    assert bool((ta.kind == abi.FTL_TR_VOID).any()) and bool((ta.kind == abi.FTL_TR_TRUNCATED).any())
    _same_batches(a, p, "pipelined")
    a.close(), p.close()


def test_collect_on_a_two_stream_handle(monkeypatch):
    """Config F from 8,192 envs on steps on two streams: the sample kernel of step t waits for the sensor kernels of both halves of step
    t - 1, the record kernel and the last copy for both halves of their step."""
    n, T, widths = 8192 + 37, 5, (360, 32, 2)                      # 30 .. 70 frames a step: with max_steps = 100 an episode lasts 2 to 4 steps
    trajs, envs = [], []
    noise = torch.from_numpy(np.random.default_rng(901).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    sigma = torch.from_numpy(_sigma(902, 1, 2)).to(DEV)
    for split in ("1", "0"):
        monkeypatch.setenv("FTL_SPLIT", split)
        env = _vec("F_s1_chase", n, over=dict(max_steps=100))
        pol, _ = _policy(env, widths, 1, 900, scale=0.1, nasty=False)
        env.step(pol.act())
        trajs.append(env.collect_mlp(pol, T, noise, sigma))
        envs.append(env)
    for k in TRAJ:
        assert torch.equal(getattr(trajs[0], k), getattr(trajs[1], k)), k
    assert bool((trajs[0].kind == abi.FTL_TR_VOID).any()) and bool((trajs[0].kind == abi.FTL_TR_STEP).any())
    _same_batches(envs[0], envs[1], "two streams")
    envs[0].close(), envs[1].close()


# ---------------------------------------------------------------- 6. the advantage kernel equals the twin
def _gae_case(seed, T, n):
    rng = np.random.default_rng(seed)
    reward = rng.standard_normal((T, n)) * rng.choice([1e-6, 1e-2, 1.0, 300.0], (T, n))
    values = (rng.standard_normal((T + 1, n)) * rng.choice([1e-4, 1.0, 50.0], (T + 1, n))).astype(np.float32)
    kind = rng.integers(0, 4, (T, n)).astype(np.uint8)
    if n >= 24:
        for k in range(4):
            kind[0, 16 + k] = k                                    # a first and a last row of each kind
            kind[T - 1, 20 + k] = k
        if T >= 2:
            for pair in range(16):                                 # every ordered pair of neighbours
                kind[0, pair], kind[1, pair] = pair // 4, pair % 4
            assert {(int(x), int(y)) for x, y in zip(kind[:-1].ravel(), kind[1:].ravel())} == {(x, y) for x in range(4) for y in range(4)}
        assert set(kind[0].tolist()) == set(kind[T - 1].tolist()) == {0, 1, 2, 3}
    return reward, kind, values


@pytest.mark.parametrize("gamma, lam", [(1.0, 1.0), (0.99, 0.95), (0.0, 0.5)])
def test_gae_equals_the_twin(gamma, lam):
    from continiousenvironment_follower_leader_amd import mlp
    for T in (1, 2, 9):
        for n in (1, 255, 257):
            reward, kind, values = _gae_case(1000 + 10 * T + n, T, n)
            r, k, v = (torch.from_numpy(x).to(DEV) for x in (reward, kind, values))
            adv, ret = mlp.gae((r, k), v, gamma, lam)
            wa, wr = CN.gae(reward, kind, values, gamma, lam)
            assert adv.dtype == ret.dtype == torch.float32 and tuple(adv.shape) == tuple(ret.shape) == (T, n)
            assert torch.equal(adv.cpu(), torch.from_numpy(wa)), (T, n, "adv")
            assert torch.equal(ret.cpu(), torch.from_numpy(wr)), (T, n, "ret")
            a2, r2 = mlp.gae((r, k), v[:, :, None], gamma, lam, out=(adv, ret))                 # a critic's [T+1, N, 1], into the same pair
            assert a2 is adv and r2 is ret and torch.equal(adv.cpu(), torch.from_numpy(wa))


# ---------------------------------------------------------------- 7. refusals through Python
def test_refusals():
    from continiousenvironment_follower_leader_amd import mlp
    n, T = 6, 2
    env, other = _vec("B_s1_chase", n), _vec("B_s1_chase", n)
    pol, _ = _policy(env, (180, 8, 2), 2, 1100, nasty=False)
    noise, sigma = torch.zeros(T, n, 2, dtype=torch.float32, device=DEV), torch.ones(2, 2, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="MlpPolicy of this batch"):
        other.collect_mlp(pol, T)
    for bad in (noise[:, :, :1], noise[:1], noise.double(), noise.cpu(), noise.transpose(0, 1)):
        with pytest.raises(ValueError, match="noise"):
            env.collect_mlp(pol, T, bad, sigma)
    for bad in (sigma[:1], sigma.double(), sigma.cpu(), torch.ones(2, 3, dtype=torch.float32, device=DEV)):
        with pytest.raises(ValueError, match="sigma"):
            env.collect_mlp(pol, T, noise, bad)
    with pytest.raises(ValueError, match="sigma"):
        env.collect_mlp(pol, T, noise)                             # a Box head with noise but no sigma
    with pytest.raises(ValueError, match="sigma"):
        pol.sample(noise[0])
    with pytest.raises(ValueError, match="noise"):
        pol.sample(noise, sigma)                                   # [T, N, A] where [N, A] belongs
    for mode in (True, "same_step", "queue", "sample", "never"):
        with pytest.raises(ValueError, match="auto_reset"):
            env.collect_mlp(pol, T, noise, sigma, auto_reset=mode)
    with pytest.raises(ValueError, match="T >= 1"):
        env.collect_mlp(pol, 0)
    tr = env.collect_mlp(pol, T, noise, sigma)
    with pytest.raises(ValueError, match="out.obs"):
        env.collect_mlp(pol, T + 1, out=tr)
    values = torch.zeros(T + 1, n, dtype=torch.float32, device=DEV)
    for bad in (values[:T], values.double(), values.cpu(), values.clone().requires_grad_(True)):
        with pytest.raises(ValueError, match="values"):
            mlp.gae(tr, bad, 0.99, 0.95)
    with pytest.raises(ValueError, match="kind"):
        mlp.gae((tr.reward, tr.kind.to(torch.int32)), values, 0.99, 0.95)
    with pytest.raises(ValueError, match="adv"):
        mlp.gae(tr, values, 0.99, 0.95, out=(torch.zeros(T, n, device=DEV, dtype=torch.float64), torch.zeros(T, n, device=DEV)))
    env.close(), other.close()
