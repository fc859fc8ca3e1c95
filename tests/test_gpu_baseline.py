"""GPU tests of the baseline follower (include/ftl.h: ftl_baseline_act, ftl_rollout_baseline; ``baseline.BaselineFollower``,
``rollout_baseline``): the device controller against the table and the four episodes recorded from the UNMODIFIED reference's controller
(tests/golden/gen/make_golden_baseline.py), and the one-call closed-loop rollout against the loop it replaces, bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import GOLDEN, close, config_for, load_episode, scenario_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("rb_pos", "rb_dbl", "rb_int", "env_int", "env_dbl", "fol_cs", "snap_rects", "snap_win", "traj", "traj_bb", "hist", "corr",
          "corr32", "ep_stats", "hist1")
OUT = ("obs_num", "target", "reward", "done", "status", "lasers")
EPISODES = ("A_s0", "B_s1", "Bastar_s1", "E_s3")
V_CAP = 8          # as tests/test_baseline_host.py: rows of the table whose v may sit one ulp from the reference's

_POOLS = {}


def _cfg_pool(name):
    """(cfg, pool of the usable scenarios among seeds 0..63) of a golden episode's config."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    if name not in _POOLS:
        _, meta = load_episode(name)
        cfg = config_for(meta, scen_route_len=256)
        _POOLS[name] = (cfg, ScenarioPool.generate(cfg, np.arange(64), DEV))
    return _POOLS[name]


def _vec(name, n, cls=None, **kw):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg, pool = _cfg_pool(name)
    env = (cls or VecGame)(n, device=DEV, config=cfg, **kw)
    env.load_scenarios(pool)
    env.reset()
    return env


def _follower(env, cap=64):
    from continiousenvironment_follower_leader_amd.baseline import BaselineFollower
    return BaselineFollower(env, cap=cap)


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def _step_count(env):
    return env.state_field("env_int")[:, abi.EI_STEP_COUNT]


# ---------------------------------------------------------------- 1. the table of the reference's move_to_the_point
def test_table():
    with np.load(os.path.join(GOLDEN, "baseline_table.npz")) as f:
        z = {k: f[k] for k in f.files}
    n = len(z["v"])
    assert n == 4096
    env = _vec("A_s0_chase", n)
    assert int(_step_count(env).ne(0).sum()) == 0                  # after reset(): every row re-seeds its FIFO with the target
    env.obs_num[:, 5:7] = torch.from_numpy(z["pos"]).to(DEV)
    env.obs_num[:, 8] = torch.from_numpy(z["direction"]).to(DEV)
    env.target.copy_(torch.from_numpy(z["target"]).to(DEV))
    f = _follower(env)
    a = f.act()
    assert a is f.action and a.dtype == torch.float64 and tuple(a.shape) == (n, 2)
    got = a.cpu().numpy()
    assert np.array_equal(got[:, 1], z["w"])
    d = _ulps(got[:, 0], z["v"])
    print("baseline table on the device: %d of %d rows of v not bit-identical to the reference (max %d ulp)" % (int((d != 0).sum()), n, int(d.max())))
    assert d.max() <= 1
    assert int((d != 0).sum()) <= V_CAP
    assert bool(f.stack_len().eq(1).all()) and bool(f.flags().eq(0).all())
    assert torch.equal(f.front(), env.target)
    assert f.flags().dtype == torch.int32 and f.stack_len().dtype == torch.int32
    assert f.state.dtype == torch.uint8 and tuple(f.state.shape) == (n, 16 + 16 * 64)
    env.close()


# ---------------------------------------------------------------- 2. the closed loop of run_2d.py --mode base, episode by episode
def _episode_env(name):
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool, VecGame
    with np.load(os.path.join(GOLDEN, "baseline_%s.npz" % name)) as f:
        z = {k: f[k] for k in f.files}               # (an NpzFile unpacks an array again at every access)
    meta = json.loads(str(z["meta"]))
    cfg = config_for(meta, scen_route_len=len(z["scen:route"]))
    s = scenario_arrays(z)
    env = VecGame(1, device=DEV, config=cfg)
    env.load_scenarios(ScenarioPool(cfg, s["static_rects"][None], s["robot_pos"][None], s["robot_dir"][None], s["robot_rect"][None],
                                    [s["route"]], [s["init_traj"]], DEV))
    env.reset(torch.zeros(1, dtype=torch.int32))
    return z, env


@pytest.mark.parametrize("name", EPISODES)
def test_episode(name):
    z, env = _episode_env(name)
    f = _follower(env)
    assert close(env.obs_num.cpu().numpy()[0], z["reset:num"]).all()
    acts, lens, nums, dones, stats, rews = [], [], [], [], [], []
    T = len(z["actions"])
    for t in range(T):                                             # (nothing is read back inside the loop)
        a = f.act()
        acts.append(a.clone()), lens.append(f.stack_len().clone())
        env.step(a)
        nums.append(env.obs_num.clone()), dones.append(env.done.clone()), stats.append(env.status.clone()), rews.append(env.reward.clone())
    acts, nums = torch.cat(acts).cpu().numpy(), torch.cat(nums).cpu().numpy()
    lens, dones, stats, rews = torch.cat(lens).cpu().numpy(), torch.cat(dones).cpu().numpy(), torch.cat(stats).cpu().numpy(), torch.cat(rews).cpu().numpy()
    for t in range(T):
        assert acts[t, 1] == z["actions"][t, 1], (name, t, "w", acts[t, 1], z["actions"][t, 1])
        assert _ulps(acts[t, 0], z["actions"][t, 0]) <= 1, (name, t, "v", acts[t, 0], z["actions"][t, 0])
        assert lens[t] == z["bl:fifo_len"][t], (name, t, "FIFO length", lens[t], z["bl:fifo_len"][t])
        assert bool(dones[t]) == bool(z["done"][t]), (name, t, "done")
        assert tuple(stats[t]) == tuple(z["info"][t]), (name, t, stats[t], z["info"][t])
        assert close(nums[t], z["obs:num"][t]).all(), (name, t, "num", nums[t] - z["obs:num"][t])
        assert abs(rews[t] - z["reward"][t]) <= 1e-5, (name, t, rews[t], z["reward"][t])
    assert int(f.flags()[0]) == 0                                  # cap = 64: neither rule was needed
    assert int(env.state_field("env_int")[0, abi.EI_ERROR]) == 0
    env.close()


# ---------------------------------------------------------------- 3. one call = the loop it replaces
def _fold(env, T, gamma, step):
    """(ret, steps, status) of ftl_rollout over ``T`` calls of ``step(t)``, folded on the device as ftl_rollout_fold_kernel folds: float64,
    one rounding per operation."""
    alive = env.state_field("env_int")[:, abi.EI_DONE].eq(0)
    ret = torch.zeros(env.n, dtype=torch.float64, device=DEV)
    steps, status = torch.zeros(env.n, dtype=torch.int32, device=DEV), torch.zeros(env.n, 3, dtype=torch.uint8, device=DEV)
    disc = 1.0
    for t in range(T):
        step(t)
        term = disc * env.reward
        ret = torch.where(alive, ret + term, ret)
        steps = steps + alive.to(torch.int32)
        end = alive & env.done.bool()
        status = torch.where(end[:, None], env.status, status)
        alive = alive & ~env.done.bool()
        disc = disc * gamma
    return ret, steps, status


@pytest.mark.parametrize("sensors", [True, False])
def test_rollout_is_the_loop(sensors):
    n, T, gamma = 67, 12, 0.97
    env = _vec("B_s1_chase", n)
    f = _follower(env)
    for t in range(5):                                             # followers under way, FIFOs of several lengths ...
        env.step(f.act(), sensors=False)
    env.reset(mask=(torch.arange(n) % 5 == 0).to(torch.uint8).to(DEV))      # ... and every fifth env at step count 0: it restarts inside the rollout
    env.scan()
    assert 0 < int(_step_count(env).eq(0).sum()) < n
    snap, fstate = env.snapshot(), f.state.clone()
    before = env.lasers.clone()

    r = env.rollout_baseline(f, T, gamma=gamma, sensors=sensors, record=True)
    assert len(r) == 4 and r[0] is env.rollout_ret and tuple(r[3].shape) == (T, n, 2) and r[3].dtype == torch.float64
    one = dict(out={k: getattr(env, k).clone() for k in OUT}, ro=[x.clone() for x in r[:3]], state={k: env.state_field(k).clone() for k in FIELDS},
               fol=f.state.clone(), acts=r[3].clone())
    assert bool(one["ro"][1].eq(T).any()) and bool(one["ro"][0].ne(0).any())
    assert not torch.equal(one["fol"], fstate)
    assert torch.equal(env.lasers, before) != sensors

    env.restore(snap, slot_stats=True)
    f.state.copy_(fstate)
    played = []

    def step(t):
        played.append(f.act().clone())
        env.step(played[-1], sensors=sensors and t == T - 1)
    ro = _fold(env, T, gamma, step)
    for k in OUT:
        assert torch.equal(getattr(env, k), one["out"][k]), ("loop", k)
    for x, y, k in zip(ro, one["ro"], ("ret", "steps", "status")):
        assert torch.equal(x, y), ("loop", k)
    for k in FIELDS:
        assert torch.equal(env.state_field(k), one["state"][k]), ("loop", k)
    assert torch.equal(f.state, one["fol"])
    assert torch.equal(torch.stack(played), one["acts"])

    env.restore(snap, slot_stats=True)                             # the open-loop rollout of what was recorded
    r2 = env.rollout(one["acts"], gamma=gamma, sensors=sensors)
    for x, y, k in zip(r2, one["ro"], ("ret", "steps", "status")):
        assert torch.equal(x, y), ("rollout", k)
    for k in FIELDS:
        assert torch.equal(env.state_field(k), one["state"][k]), ("rollout", k)

    env.restore(snap, slot_stats=True)                             # without a record: the handle's scratch, the same result
    f.state.copy_(fstate)
    r3 = env.rollout_baseline(f, T, gamma=gamma, sensors=sensors)
    assert len(r3) == 3
    for x, y in zip(r3, one["ro"]):
        assert torch.equal(x, y)
    assert torch.equal(f.state, one["fol"])
    with pytest.raises(ValueError):
        env.rollout_baseline(f, 0)
    with pytest.raises(ValueError):
        env.rollout_baseline(object(), 3)
    env.close()


def test_rollout_on_a_two_stream_handle(monkeypatch):
    """The handle's own two-stream mode (config F, from 8,192 envs on: tests/test_gpu_scan_on_demand.py) at the smallest size that runs
    it: the act kernel of step t has to wait for both halves of step t - 1."""
    monkeypatch.setenv("FTL_SPLIT", "1")
    n, T, gamma = 8192 + 37, 4, 0.9
    env = _vec("F_s1_chase", n)
    f = _follower(env)
    env.step(f.act(), sensors=False)
    snap, fstate = env.snapshot(), f.state.clone()
    r = env.rollout_baseline(f, T, gamma=gamma, record=True)
    one = dict(out={k: getattr(env, k).clone() for k in OUT}, ro=[x.clone() for x in r[:3]], state={k: env.state_field(k).clone() for k in FIELDS},
               fol=f.state.clone(), acts=r[3].clone())
    env.restore(snap, slot_stats=True)
    f.state.copy_(fstate)
    played = []

    def step(t):
        played.append(f.act().clone())
        env.step(played[-1], sensors=t == T - 1)
    ro = _fold(env, T, gamma, step)
    for k in OUT:
        assert torch.equal(getattr(env, k), one["out"][k]), k
    for x, y, k in zip(ro, one["ro"], ("ret", "steps", "status")):
        assert torch.equal(x, y), k
    for k in FIELDS:
        assert torch.equal(env.state_field(k), one["state"][k]), k
    assert torch.equal(f.state, one["fol"]) and torch.equal(torch.stack(played), one["acts"])
    assert bool(one["ro"][1].eq(T).any())
    env.restore(snap, slot_stats=True)                             # ftl_rollout on the same handle: the open-loop rollout of the record
    r2 = env.rollout(one["acts"], gamma=gamma)
    for k in OUT:
        assert torch.equal(getattr(env, k), one["out"][k]), ("rollout", k)
    for x, y, k in zip(r2, one["ro"], ("ret", "steps", "status")):
        assert torch.equal(x, y), ("rollout", k)
    for k in FIELDS:
        assert torch.equal(env.state_field(k), one["state"][k]), ("rollout", k)
    env.close()


# ---------------------------------------------------------------- 4. an env at step count 0 starts afresh, under every reset discipline
@pytest.mark.parametrize("auto_reset", [True, "next_step"])
def test_restarts(auto_reset):
    n = 64
    env = _vec("Bshort_s4_chase", n)
    f = _follower(env)
    restarts = running = 0
    for t in range(61):                                            # the decision after reset() and after each of 60 steps
        a = f.act()
        fresh = _step_count(env).eq(0)
        assert t > 0 or bool(fresh.all())
        assert bool(f.stack_len()[fresh].eq(1).all()), t
        assert torch.equal(f.front()[fresh], env.target[fresh]), t
        if t:
            restarts += int(fresh.sum())
        running += int(f.stack_len()[~fresh].gt(1).sum())
        if t < 60:
            env.step(a, auto_reset=auto_reset, sensors=False)
    assert restarts > 0, "no env restarted"
    assert running > 0, "no follower ever held more than one point"
    env.close()


# ---------------------------------------------------------------- 5. the two rules the reference has no counterpart for
def test_overflow_flag():
    z, env = _episode_env("B_s1")
    assert z["bl:fifo_len"].max() > 2
    f = _follower(env, cap=2)
    for t in range(len(z["actions"])):
        env.step(f.act(), sensors=False)
    assert int(f.flags()[0]) & abi.FTL_BL_OVERFLOW
    assert int(f.stack_len().max()) <= 2
    env.close()


def test_empty_flag():
    """A fresh follower on envs under way (at step count 0 the second act() would simply start afresh) whose target is where they stand:
    the first act() seeds the FIFO with that point and asks for its pop, the second cannot make it."""
    n = 70
    env = _vec("B_s1_chase", n)
    env.step(torch.zeros(n, 2, dtype=torch.float64, device=DEV), sensors=False)
    assert bool(_step_count(env).gt(0).all())
    point = torch.tensor([321.0, 123.5], dtype=torch.float64, device=DEV)
    env.target.copy_(point.expand(n, 2))
    env.obs_num[:, 5:7] = point.float()
    f = _follower(env)
    f.act()
    assert bool(f.flags().eq(0).all()) and bool(f.stack_len().eq(1).all())
    a = f.act()
    assert bool(f.flags().eq(abi.FTL_BL_EMPTY).all()) and bool(f.stack_len().eq(1).all())
    assert torch.equal(f.front(), env.target) and bool(a[:, 0].eq(0).all())
    env.close()


# ---------------------------------------------------------------- 6. pipelined
def test_pipelined_matches_vec_game():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    n = 1045
    a, p = _vec("B_s1_chase", n), _vec("B_s1_chase", n, cls=PipelinedVecGame, parts=2)
    fa, fp = _follower(a), _follower(p)
    for env, f in ((a, fa), (p, fp)):
        env.step(f.act(), sensors=False)                           # the policy form on both, once
    ra, rp = a.rollout_baseline(fa, 8, gamma=0.9, record=True), p.rollout_baseline(fp, 8, gamma=0.9, record=True)
    p.join()
    for x, y in zip(ra, rp):
        assert torch.equal(x, y)
    assert bool(ra[1].eq(8).any())
    for k in OUT:
        assert torch.equal(getattr(a, k), getattr(p, k)), k
    assert torch.equal(fa.state, fp.state)
    assert bool(fa.stack_len().gt(1).any())
    for k in FIELDS:
        assert torch.equal(a.state_field(k), p.state_field(k)), k
    a.close(), p.close()


# ---------------------------------------------------------------- 7. the baseline's score per scenario, whatever the batch size
def test_evaluate_is_independent_of_the_batch_size():
    recs = []
    for n in (32, 96):
        env = _vec("B_s1_chase", n)
        scen = torch.arange(96) % env.pool.n
        recs.append(env.evaluate(_follower(env), scen, sensors=False))
        env.close()
    r0, r1 = recs
    assert len(r0) == len(r1) == 96 and (r0["state"] == 2).all() and (r1["state"] == 2).all()
    for col in ("scenario", "frames", "calls", "status", "errors", "flags", "ret", "stream"):
        assert np.array_equal(r0[col], r1[col]), col
    assert len(set(r0["ret"].tolist())) > 1 and len(set(r0["frames"].tolist())) > 1, "every episode went the same way"
    assert (r0["errors"] == 0).all()
