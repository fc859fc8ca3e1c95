"""GPU tests of the on-demand sensor scans (include/ftl.h: FTL_STEP_NO_SENSORS, ftl_scan, ftl_rollout; ``VecGame.step(sensors=False)``,
``scan()``, ``rollout()`` and their ``PipelinedVecGame`` twins).

The oracle is the library's own ordinary step: batch A is stepped as before, batch B -- same config, same pool, same reset, same actions --
takes the new path.  Every comparison is exact equality ("state" = every field ``ftl_state_field`` knows).  Batches have 83 envs (prime,
above one wavefront, an idle tail group at 16 and at 8 envs per wavefront) and runs at most 12 steps; where episodes must end, ``max_steps``
is three steps' worth of frames."""
import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import config_for, load_episode

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 83
FIELDS = ("rb_pos", "rb_dbl", "rb_int", "env_int", "env_dbl", "fol_cs", "snap_rects", "snap_win", "traj", "traj_bb", "hist", "corr",
          "corr32", "ep_stats", "hist1")
STEP_OUT = ("obs_num", "target", "reward", "done", "status")          # what the frame half of a step writes
SENSOR_OUT = ("lasers", "policy_obs")                                 # what the sensor half writes

_POOLS = {}


def _cfg_pool(name, short):
    """(cfg, pool of the usable scenarios among seeds 0..63) of a golden episode's config; ``short``: episodes of three steps."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    if (name, short) not in _POOLS:
        _, meta = load_episode(name)
        over = {}
        if short:
            c = config_for(meta).c
            over = dict(max_steps=3 * (c.rand_fps_hi - 1 if c.rand_fps_hi > 0 else c.frames_per_step), warm_start=min(c.warm_start, 10))
        cfg = config_for(meta, scen_route_len=256, **over)
        _POOLS[(name, short)] = (cfg, ScenarioPool.generate(cfg, np.arange(64), DEV))
    return _POOLS[(name, short)]


def _vec(name, short, n=N, cls=None, **kw):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg, pool = _cfg_pool(name, short)
    env = (cls or VecGame)(n, device=DEV, config=cfg, **kw)
    env.load_scenarios(pool)
    env.reset()
    return env


def _actions(cfg, n, t, seed=0):
    """Seeded like tests/test_gpu_configs.py::_actions; Discrete(5) configs draw indices."""
    rng = np.random.default_rng(seed * 7919 + t)
    if cfg.discrete_action_space:
        return torch.from_numpy(rng.integers(0, 5, n)).to(DEV)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    v = rng.uniform(0.5, 1.0, n) * ms
    w = np.clip(rng.normal(0, 0.2 * mr, n), -mr, mr)
    return torch.from_numpy(np.stack([v, w], 1)).to(DEV).contiguous()


def _same(a, b, names, what, rows=None):
    for k in names:
        x, y = getattr(a, k, None), getattr(b, k, None)
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            if rows is not None:
                x, y = x[rows], y[rows]
            assert torch.equal(x, y), (what, k)


def _same_state(a, b, what):
    for f in FIELDS:
        assert torch.equal(a.state_field(f), b.state_field(f)), (what, f)


def _sensor_rows(env):
    return {k: getattr(env, k).clone() for k in SENSOR_OUT if getattr(env, k, None) is not None}


def _episodes(env):
    return int(env.state_field("env_int")[:, abi.EI_EPISODES].sum())


def _staggered(name, **kw):
    """A batch in every phase of its episodes.  With ``max_steps`` of three steps' worth of frames an episode ends in its fourth step (the
    first frame past the limit), so after four steps, env e re-initialised after step (e mod 4) + 1 for e mod 4 < 3, the envs are 1, 2 and 3
    steps away from their end and every fourth one (3 mod 4) is done."""
    env = _vec(name, True, **kw)
    for t in range(4):
        env.step(_actions(env.cfg, N, 100 + t, seed=3))
        if t < 3:
            env.reset(mask=(torch.arange(N) % 4 == t).to(torch.uint8).to(DEV))
    return env


# ---------------------------------------------------------------- 1. blind step + scan = step
CASES_1 = [("B_s1_chase", {}, {}), ("B_s1_chase", {"FTL_DEBUG_G8": "0"}, {}), ("B_s1_chase", {"FTL_DEBUG_G8": "1"}, {}),
           ("L_s2_chase", {}, {}), ("T_s3_chase", {}, {}), ("C_s1_chase", {}, dict(policy_obs=True)), ("F_s1_chase", {"FTL_SPLIT": "1"}, {}),
           # the handle's two-stream mode starts at 8,192 envs (tests/test_gpu_configs.py): the same case at the smallest size that runs it
           ("F_s1_chase", {"FTL_SPLIT": "1"}, dict(n=8192 + 37))]


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("name, switches, kw", CASES_1, ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % i for i in v.items()) or "-")
def test_blind_step_then_scan_is_a_step(monkeypatch, name, switches, kw, auto_reset):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    a, b = _vec(name, True, **kw), _vec(name, True, **kw)
    if kw.get("policy_obs"):
        assert b.policy_obs is not None
    ended = 0
    for t in range(6):
        act = _actions(a.cfg, a.n, t)
        before = _sensor_rows(b)
        a.step(act, auto_reset=auto_reset)
        b.step(act, auto_reset=auto_reset, sensors=False)
        _same(a, b, STEP_OUT, "blind step %d" % t)
        for k, v in before.items():
            assert torch.equal(getattr(b, k), v), ("a blind step wrote", k, t)
        if t < 3:                                                     # (the first episodes are still running: the world has moved)
            assert not torch.equal(a.lasers, b.lasers), "step %d: the readings did not change, the test shows nothing" % t
        assert b.scan() is b.lasers
        _same(a, b, SENSOR_OUT, "scan after blind step %d" % t)
        ended += int(a.done.sum())
    _same_state(a, b, "after the last step")
    assert ended > 0, "no episode ended"
    if auto_reset:
        assert _episodes(b) > 0, "no env restarted"


# ---------------------------------------------------------------- 2. k blind steps, then one full step
@pytest.mark.parametrize("auto_reset", [False, True, "same_step", "next_step"])
@pytest.mark.parametrize("name", ["B_s1_chase", "L_s2_chase"])
def test_blind_steps_then_one_full_step(name, auto_reset):
    a, b = _staggered(name, final_obs=True), _staggered(name, final_obs=True)
    masks = ("ended", "restarted") if auto_reset is not True else ()          # (auto_reset=True passes no final buffers)
    finals = ("final_obs_num", "final_target") if auto_reset == "same_step" else ()
    ended = restarted = 0
    for t in range(6):
        act = _actions(a.cfg, N, t, seed=1)
        a.step(act, auto_reset=auto_reset)
        b.step(act, auto_reset=auto_reset, sensors=t == 5)
        _same(a, b, STEP_OUT + masks + finals, "step %d" % t)
        ended += int(a.done.sum())
        restarted += int(a.restarted.sum()) if masks else 0
    _same(a, b, STEP_OUT + SENSOR_OUT + masks + finals, "after the full step")
    if auto_reset == "same_step":          # rows of the envs that ended in the full step (earlier rows hold copies of stale readings)
        rows = a.ended.bool()
        assert bool(rows.any())
        _same(a, b, ("final_lasers",), "terminal readings of the full step", rows)
    _same_state(a, b, "after the full step")
    assert ended > 0, "no episode ended"
    if auto_reset:
        assert _episodes(b) > 0, "no env restarted"
        assert auto_reset is True or restarted > 0


# ---------------------------------------------------------------- 3. scan after restore
@pytest.mark.parametrize("name, kw", [("B_s1_chase", {}), ("C_s1_chase", dict(policy_obs=True)), ("L_s2_chase", {})], ids=lambda v: v if isinstance(v, str) else "")
def test_scan_after_restore(name, kw):
    env = _vec(name, False, **kw)
    ids = torch.tensor([0, 5, 16, 17, 40, 63, 64, 81, 82])
    for t in range(4):
        env.step(_actions(env.cfg, N, t, seed=2))
    kept = {k: v[ids.to(DEV)] for k, v in _sensor_rows(env).items()}
    snap = env.snapshot(ids)
    for t in range(4, 7):
        env.step(_actions(env.cfg, N, t, seed=2))
    later = _sensor_rows(env)
    env.restore(snap, ids)
    for k in later:                        # (restore() copies the snapshot's output rows as well: wipe them, the scan must bring them back)
        getattr(env, k).fill_(-1.0)
    env.scan()
    others = torch.ones(N, dtype=torch.bool)
    others[ids] = False
    for k in later:
        got = getattr(env, k)
        assert torch.equal(got[ids.to(DEV)], kept[k]), ("restored envs", k)
        assert torch.equal(got[others.to(DEV)], later[k][others.to(DEV)]), ("other envs", k)
        assert not torch.equal(kept[k], later[k][ids.to(DEV)]), "the readings did not change, the test shows nothing"


# ---------------------------------------------------------------- 4. rollout = steps
def _recompute(rewards, dones, statuses, done0, gamma):
    """(ret, steps, status) of ftl_rollout from per-step outputs, float64 on the CPU, one rounding per operation."""
    alive = ~done0
    ret, steps, status = torch.zeros(len(done0), dtype=torch.float64), torch.zeros(len(done0), dtype=torch.int32), torch.zeros(len(done0), 3, dtype=torch.uint8)
    disc = 1.0
    for r, d, s in zip(rewards, dones, statuses):
        term = disc * r
        ret = torch.where(alive, ret + term, ret)
        steps += alive.to(torch.int32)
        end = alive & d.bool()
        status[end] = s[end]
        alive = alive & ~d.bool()
        disc = disc * gamma
    return ret, steps, status


@pytest.mark.parametrize("sensors", [True, False])
@pytest.mark.parametrize("gamma", [1.0, 0.97])
def test_rollout_is_a_loop_of_steps(gamma, sensors):
    a, b = _staggered("B_s1_chase"), _staggered("B_s1_chase")
    _same_state(a, b, "before the rollout")
    done0 = a.state_field("env_int")[:, abi.EI_DONE].ne(0).cpu()
    assert bool(done0.any()) and not bool(done0.all())
    acts = torch.stack([_actions(a.cfg, N, t, seed=4) for t in range(5)])
    rewards, dones, statuses = [], [], []
    for t in range(5):
        a.step(acts[t])
        rewards.append(a.reward.cpu()), dones.append(a.done.cpu()), statuses.append(a.status.cpu())
    before = b.lasers.clone()
    ret, steps, status = b.rollout(acts, gamma=gamma, sensors=sensors)
    assert ret is b.rollout_ret and ret.dtype == torch.float64 and steps.dtype == torch.int32 and status.dtype == torch.uint8
    want = _recompute(rewards, dones, statuses, done0, gamma)
    assert torch.equal(ret.cpu(), want[0]) and torch.equal(steps.cpu(), want[1]) and torch.equal(status.cpu(), want[2])
    assert not bool(ret.cpu()[done0].ne(0).any()) and not bool(steps.cpu()[done0].ne(0).any()) and not bool(status.cpu()[done0].ne(0).any())
    assert sorted(set(steps.cpu().tolist())) == [0, 1, 2, 3]                        # the stagger of _staggered
    assert bool(status.cpu()[~done0].ne(0).any(1).all())                            # every running episode ended inside the rollout
    assert bool(ret.cpu()[~done0].ne(0).any())
    _same(a, b, STEP_OUT, "after the rollout")
    if sensors:
        _same(a, b, SENSOR_OUT, "after the rollout")
    else:
        assert torch.equal(b.lasers, before) and not torch.equal(b.lasers, a.lasers)
    _same_state(a, b, "after the rollout")
    b.rollout(acts[:2], gamma=gamma, sensors=sensors)                                # the persistent tensors are reused and rewritten
    assert b.rollout_ret is ret and not bool(b.rollout_steps.ne(0).any())              # (every env is done by now)


def test_rollout_discrete_actions():
    a, b = _vec("N_s3_chase", False), _vec("N_s3_chase", False)
    assert a.cfg.discrete_action_space
    acts = torch.stack([_actions(a.cfg, N, t, seed=5) for t in range(5)])
    rewards, dones, statuses = [], [], []
    for t in range(5):
        a.step(acts[t])
        rewards.append(a.reward.cpu()), dones.append(a.done.cpu()), statuses.append(a.status.cpu())
    ret, steps, status = b.rollout(acts, gamma=0.97)
    want = _recompute(rewards, dones, statuses, torch.zeros(N, dtype=torch.bool), 0.97)
    assert torch.equal(ret.cpu(), want[0]) and torch.equal(steps.cpu(), want[1]) and torch.equal(status.cpu(), want[2])
    assert bool(steps.eq(5).any()), "no episode outlived the rollout"
    _same(a, b, STEP_OUT + SENSOR_OUT, "after the rollout")
    _same_state(a, b, "after the rollout")
    with pytest.raises(ValueError):
        b.rollout(acts.double())                                                    # the checks of _encode_action
    with pytest.raises(ValueError):
        b.rollout(acts[:, :N - 1])


# ---------------------------------------------------------------- 5. queue and sampler
def test_queue_played_blind_gives_the_same_records():
    recs = []
    for sensors in (True, False):
        env = _vec("B_s1_chase", True, n=19)
        q = env.set_episode_queue(torch.arange(40) % env.pool.n)
        env.reset_from_queue()
        before = env.lasers.clone()
        for t in range(12):
            env.step(_actions(env.cfg, 19, t, seed=6), auto_reset="queue", sensors=sensors)
        assert torch.equal(env.lasers, before) != sensors
        recs.append((q.records(), {f: env.state_field(f).clone() for f in FIELDS}, env.ticket.clone()))
    (r0, s0, t0), (r1, s1, t1) = recs
    assert int((r0["state"] == 2).sum()) >= 20, "hardly an episode was recorded"
    assert r0.tobytes() == r1.tobytes()
    assert torch.equal(t0, t1)
    for f in FIELDS:
        assert torch.equal(s0[f], s1[f]), f


def test_sampler_played_blind_gives_the_same_table():
    from continiousenvironment_follower_leader_amd import ScenarioSampler
    runs = []
    for sensors in (True, False):
        env = _vec("B_s1_chase", True)
        s = ScenarioSampler(env.pool.n - 9, base=5, device=DEV)
        s.set_raw_weights(torch.arange(1, env.pool.n - 8))
        env.set_scenario_sampler(s)
        env.reset_from_sampler()
        for t in range(10):
            env.step(_actions(env.cfg, N, t, seed=7), auto_reset="sample", sensors=sensors)
        runs.append((s._table.clone(), {f: env.state_field(f).clone() for f in FIELDS}, {k: getattr(env, k).clone() for k in STEP_OUT}))
    (t0, s0, o0), (t1, s1, o1) = runs
    assert int(t0[:, abi.SS_EPISODES].sum()) >= N, "hardly an episode was recorded"
    assert torch.equal(t0, t1)
    for f in FIELDS:
        assert torch.equal(s0[f], s1[f]), f
    for k in STEP_OUT:
        assert torch.equal(o0[k], o1[k]), k


# ---------------------------------------------------------------- 6. pipelined
def test_pipelined_matches_vec_game():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    a, p = _staggered("C_s1_chase", policy_obs=True), _staggered("C_s1_chase", cls=PipelinedVecGame, parts=2, policy_obs=True)
    acts = [_actions(a.cfg, N, t, seed=8) for t in range(7)]
    for env in (a, p):
        env.step(acts[0], sensors=False)
        env.step(acts[1], auto_reset=True, sensors=False)
    p.join()
    _same(a, p, STEP_OUT + SENSOR_OUT, "after two blind steps")
    for env in (a, p):
        env.scan()
    p.join()
    _same(a, p, STEP_OUT + SENSOR_OUT, "after the scan")
    lo, hi = p.rows(1)
    a.step(acts[2], auto_reset=True)
    p.step_part(0, acts[2][:lo], auto_reset=True, sensors=False)
    p.step_part(1, acts[2][lo:hi], auto_reset=True)
    p.join()
    _same(a, p, STEP_OUT, "after step_part")
    _same(a, p, SENSOR_OUT, "after step_part", rows=slice(lo, hi))
    seq = torch.stack(acts[3:7])
    ra, rp = a.rollout(seq, gamma=0.9), p.rollout(seq, gamma=0.9)
    p.join()
    for x, y in zip(ra, rp):
        assert torch.equal(x, y)
    assert int(ra[1].min()) >= 1 and bool(ra[2].ne(0).any()), "no env was running, or no episode ended inside the rollout"
    _same(a, p, STEP_OUT + SENSOR_OUT, "after the rollout")
    for f in FIELDS:
        assert torch.equal(a.state_field(f), p.state_field(f)), f
    ra, rp = a.rollout(seq[:2], sensors=False), p.rollout(seq[:2], sensors=False)
    p.join()
    for x, y in zip(ra, rp):
        assert torch.equal(x, y)
    _same(a, p, STEP_OUT + SENSOR_OUT, "after the blind rollout")
