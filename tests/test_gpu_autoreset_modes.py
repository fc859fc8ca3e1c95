"""GPU tests of the two auto-reset contracts that return terminal observations (include/ftl.h: FTL_STEP_NEXT_RESET, ftl_step_final):

- same-step (``auto_reset="same_step"``, ``final_obs=True``): the outputs and the state of ``auto_reset=True``, plus the terminal rows
  of the envs that ended -- what a step without auto-reset returns for them -- in the final buffers;
- next-step (``auto_reset="next_step"``): the call that ends an episode returns its terminal observation; the env's next call ignores
  its action and returns the first observation of a new episode (reward 0, done 0, status 0), as ``ftl_reset`` would.

Configs: B (the headline world), F (random frame counts, leader regimes, the handle's two-stream mode), T (v1 tracker kernel), L (aux
sensors), in both lane forms of the frame kernel."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import GOLDEN, close, config_for, load_episode, scenario_arrays

pytestmark = pytest.mark.gpu

OUT = ("obs_num", "lasers", "target", "reward", "done", "status")
FINAL = ("obs_num", "lasers", "target")


@pytest.fixture(autouse=True, params=["4 lanes per env", "8 lanes per env"])
def lanes_per_env(request, monkeypatch):
    """Both forms of the frame kernel (FTL_DEBUG_G8 at ftl_create, as tests/test_gpu_parity.py)."""
    monkeypatch.setenv("FTL_DEBUG_G8", "0" if request.param.startswith("4") else "1")


_POOLS = {}


def _cfg_pool(name):
    """(cfg, pool, n_envs) of a config with episodes short enough for every env to finish at least twice in the steps below."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    if name not in _POOLS:
        if name == "B":
            z = np.load(GOLDEN + "/pool_B.npz")
            meta = json.loads(str(z["meta"]))
            cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()), max_steps=60, warm_start=10)
            pool, n = ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0"), 96
        else:
            ep = {"F": "F_s7_chase", "T": "T_s3_chase", "L": "L_s2_chase"}[name]
            _, meta = load_episode(ep)
            over = dict(max_steps=100, warm_start=10, rng_seed=4) if name == "F" else dict(max_steps=60, warm_start=10)
            cfg = config_for(meta, scen_route_len=256, **over)
            # F: 8,192 envs, the smallest batch that runs the handle's two-stream mode (FTL_SPLIT=1 below); a pool size coprime to it
            n = 8192 if name == "F" else 96
            pool = ScenarioPool.generate(cfg, np.arange(257 if name == "F" else 131), "cuda:0")
        _POOLS[name] = (cfg, pool, n)
    return _POOLS[name]


def _vec(cfg, pool, n, **kw):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    env = VecGame(n, device="cuda:0", config=cfg, **kw)
    env.load_scenarios(pool)
    return env


def _action_table(cfg, rows, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    v = (0.5 + 0.5 * torch.rand(rows, generator=g, dtype=torch.float64)) * ms
    w = torch.clamp(torch.randn(rows, generator=g, dtype=torch.float64) * 0.3 * mr, -mr, mr)
    return torch.stack([v, w], 1).contiguous().cuda()


def _steps(name):
    return 12 if name == "F" else 16


@pytest.mark.parametrize("name", ["B", "F", "T", "L"])
def test_same_step_twins(name, monkeypatch):
    """A "same_step" = B True (outputs, state, metrics bit for bit); A's final rows = C's outputs (no auto-reset) before C's reset."""
    if name == "F":
        monkeypatch.setenv("FTL_SPLIT", "1")
    cfg, pool, n = _cfg_pool(name)
    a, b, c = _vec(cfg, pool, n, final_obs=True), _vec(cfg, pool, n), _vec(cfg, pool, n)
    idx = torch.arange(n, dtype=torch.int32) % pool.n
    for e in (a, b, c):
        e.reset(idx)
    scen_c = idx.clone()
    P, stride = pool.n, n % pool.n
    ends = torch.zeros(n, dtype=torch.int64)
    tbl = _action_table(cfg, 4096, seed=11)
    for t in range(_steps(name)):
        act = tbl[(torch.arange(n, device="cuda:0") * 7 + t * 131) % tbl.shape[0]].contiguous()
        a.step(act, auto_reset="same_step")
        b.step(act, auto_reset=True)
        c.step(act, auto_reset=False)
        for k in OUT:
            assert torch.equal(getattr(a, k), getattr(b, k)), (name, t, k)
        d = c.done.bool()
        assert torch.equal(a.ended.bool(), d), (name, t)
        assert torch.equal(a.restarted, a.ended), (name, t)
        assert torch.equal(b.done.bool(), d)
        for k in FINAL:
            assert torch.equal(getattr(a, "final_" + k)[d], getattr(c, k)[d]), (name, t, k)
        term, trunc = a.terminated_truncated()
        assert torch.equal(term | trunc, d) and not bool((term & trunc).any())
        assert torch.equal(trunc, d & (c.status[:, 0] == abi.MISSION.index("finished_by_time")))
        for f in ("rb_pos", "rb_dbl", "rb_int", "env_dbl", "env_int", "ep_stats"):
            assert torch.equal(a.state_field(f), b.state_field(f)), (name, t, f)
        dc = d.cpu()
        if dc.any():
            ends += dc.long()
            scen_c = torch.where(dc, (scen_c % P + stride) % P, scen_c)
            c.reset(scen_c, mask=dc.to(torch.uint8))
        for k in ("obs_num", "lasers", "target"):
            assert torch.equal(getattr(a, k), getattr(c, k)), (name, t, k)
    assert int(ends.min()) >= 2, "every env should finish at least twice"
    assert torch.equal(a.episode_metrics(), b.episode_metrics())
    assert a.error_report() == b.error_report()
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("name", ["B", "F", "T", "L"])
def test_next_step_equivalence(name, monkeypatch):
    """Every episode of a "next_step" batch N sees the action sequence it sees in an auto_reset=True batch A (actions keyed by the env's
    episode and step within the episode): its outputs are A's, step by step, with the terminal observation that the same-step batch S
    keeps in its final buffers, and the restart call returns what A's terminal step returned as the new episode's first observation
    (reward 0, done 0, status 0)."""
    if name == "F":
        monkeypatch.setenv("FTL_SPLIT", "1")
    cfg, pool, n = _cfg_pool(name)
    A, S, N = _vec(cfg, pool, n), _vec(cfg, pool, n, final_obs=True), _vec(cfg, pool, n, final_obs=True)
    idx = torch.arange(n, dtype=torch.int32) % pool.n
    for e in (A, S, N):
        e.reset(idx)
    tbl = _action_table(cfg, 4093, seed=5)
    dev = torch.device("cuda:0")
    env_ids = torch.arange(n, device=dev)
    ja, ia = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    jn, i_n = ja.clone(), ia.clone()

    def act(j, i):
        return tbl[(env_ids * 31 + j * 977 + i * 13) % tbl.shape[0]].contiguous()

    rec_a, rec_n, restarts = {}, {}, {}          # (env, episode, step) -> outputs; (env, episode) -> first observation
    n_rec = min(n, 384)                           # envs whose episodes are compared (all of them step)
    done_entry = torch.zeros(n, dtype=torch.bool, device=dev)
    steps = _steps(name) + 6
    for t in range(steps):
        x = act(ja, ia)
        A.step(x, auto_reset=True)
        S.step(x, auto_reset="same_step")
        N.step(act(jn, i_n), auto_reset="next_step")
        # restarted marks exactly the envs that were done on entry; a restart returns ftl_reset's outputs
        assert torch.equal(N.restarted.bool(), done_entry), (name, t)
        r = done_entry
        assert not bool(N.ended.bool()[r].any())
        assert bool((N.reward[r] == 0).all()) and bool((N.done[r] == 0).all()) and bool((N.status[r] == 0).all()), (name, t)
        a_out = {k: getattr(A, k).cpu() for k in OUT}
        a_fin = {k: getattr(S, "final_" + k).cpu() for k in FINAL}
        n_out = {k: getattr(N, k).cpu() for k in OUT}
        da, rc = A.done.bool().cpu(), r.cpu()
        jac, iac, jnc, inc = ja.cpu(), ia.cpu(), jn.cpu(), i_n.cpu()
        for e in range(n_rec):
            if bool(rc[e]):
                restarts[("N", e, int(jnc[e]) + 1)] = tuple(n_out[k][e] for k in ("obs_num", "lasers", "target"))
            else:
                rec_n[(e, int(jnc[e]), int(inc[e]))] = tuple(n_out[k][e] for k in OUT)
            if bool(da[e]):          # A returned the new episode's first observation; the terminal one is S's final row
                rec_a[(e, int(jac[e]), int(iac[e]))] = tuple(a_fin[k][e] for k in FINAL) + tuple(a_out[k][e] for k in ("reward", "done", "status"))
                restarts.setdefault(("A", e, int(jac[e]) + 1), tuple(a_out[k][e] for k in ("obs_num", "lasers", "target")))
            else:
                rec_a[(e, int(jac[e]), int(iac[e]))] = tuple(a_out[k][e] for k in OUT)
        assert torch.equal(S.ended, A.done)
        # episode / step counters of the next call
        ia = torch.where(A.done.bool(), 0, ia + 1); ja = ja + A.done.long()
        stepped = ~r
        i_n = torch.where(r, 0, i_n + stepped.long()); jn = jn + r.long()
        assert torch.equal(N.ended.bool(), stepped & N.done.bool())
        done_entry = N.done.bool().clone()
    common = set(rec_a) & set(rec_n)
    assert len(common) > n_rec * 4
    for key in common:
        for k, u, v in zip(OUT, rec_a[key], rec_n[key]):
            assert torch.equal(u, v), (name, key, k)
    n_restarts = 0
    for (who, e, j), first in restarts.items():
        ref = restarts.get(("A", e, j))
        if who != "N" or ref is None:
            continue
        n_restarts += 1
        for u, v in zip(first, ref):
            assert torch.equal(u, v), (name, e, j)
    assert n_restarts >= n_rec
    for e in (A, S, N):
        e.close()


def _ending(z):
    """Index of the step that ends the golden episode (the reference keeps recording after done)."""
    d = np.flatnonzero(np.asarray(z["done"]).astype(bool))
    assert len(d), "the fixture's episode does not end"
    return int(d[0])


@pytest.mark.parametrize("ep", ["B_s5_random", "L_s7_random", "B_s1_chase", "Bshort_s4_chase", "Bes_s2_random", "F_s1_chase", "Btraj_s6_random",
                                "B3fps17_s8_random", "Lfps40_s2_chase"])       # (the last two: 17 and 40 frames per step, every frame resolving its own searches)
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_reference_episode_terminal_observation(ep, mode):
    """A golden episode replayed to its end in a pool where another entry follows it: the terminal observation (final buffers under
    same-step, the regular outputs under next-step) is the reference's last observation, terminated_truncated() its mission status;
    the restart is the reference's reset() of the next entry (the same world here, so the fixture's reset observation)."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    z, meta = load_episode(ep)
    cfg = config_for(meta, scen_route_len=len(z["scen:route"]))
    s = scenario_arrays(z)
    pool = ScenarioPool(cfg, np.stack([s["static_rects"]] * 2), np.stack([s["robot_pos"]] * 2), np.stack([s["robot_dir"]] * 2),
                        np.stack([s["robot_rect"]] * 2), [s["route"]] * 2, [s["init_traj"]] * 2, "cuda:0")
    env = _vec(cfg, pool, 1, final_obs=True)
    env.reset(torch.zeros(1, dtype=torch.int32))
    lnames = meta["laser_names"]
    t_end = _ending(z)
    acts, raw = z["actions"], (z["actions_raw"] if "actions_raw" in z else None)

    def action(t):
        if raw is None:
            return torch.tensor(np.asarray(acts[t])[None], dtype=torch.float64, device="cuda:0")
        return torch.full((1,), raw[t].item(), dtype=torch.int32 if raw.dtype == np.int32 else torch.float64, device="cuda:0")

    def check(num, views, tag, t):
        ref = z[tag + ":num"] if t is None else z[tag + ":num"][t]
        assert close(num, ref).all(), (ep, mode, tag, t, num - ref)
        for ln in lnames:
            r = z[tag + ":laser:" + ln] if t is None else z[tag + ":laser:" + ln][t]
            assert close(views[ln], r).all(), (ep, mode, tag, t, ln)
        for a in cfg.aux:
            r = z[tag + ":aux:" + a.name] if t is None else z[tag + ":aux:" + a.name][t]
            assert close(views[a.name], r).all(), (ep, mode, tag, t, a.name)

    def views(lasers):
        out = {}
        for l in cfg.lasers:
            out[l.name] = lasers[l.out_offset:l.out_offset + l.history * l.width].reshape(l.history, l.width)
        for a in cfg.aux:
            out[a.name] = lasers[a.out_offset:a.out_offset + a.out_len].reshape(*a.shape)
        return out

    for t in range(t_end + 1):
        env.step(action(t), auto_reset=mode)
        assert bool(env.ended[0]) == (t == t_end), (ep, mode, t)
    assert tuple(env.status[0].tolist()) == tuple(z["info"][t_end])
    term, trunc = env.terminated_truncated()
    timeout = int(z["info"][t_end][0]) == abi.MISSION.index("finished_by_time")
    assert bool(trunc[0]) == timeout and bool(term[0]) == (not timeout)
    if mode == "same_step":
        check(env.final_obs_num[0].cpu().numpy(), views(env.final_lasers[0].cpu().numpy()), "obs", t_end)
        assert np.array_equal(env.final_target[0].cpu().numpy(), z["obs:target"][t_end])
        assert int(env.restarted[0]) == 1
        restart = (env.obs_num[0].cpu().numpy(), env.lasers[0].cpu().numpy(), env.target[0].cpu().numpy())
    else:
        check(env.obs_num[0].cpu().numpy(), views(env.lasers[0].cpu().numpy()), "obs", t_end)
        assert np.array_equal(env.target[0].cpu().numpy(), z["obs:target"][t_end])
        env.step(action(min(t_end + 1, len(acts) - 1)), auto_reset=mode)        # ignored: the env restarts
        assert int(env.restarted[0]) == 1 and int(env.ended[0]) == 0
        assert float(env.reward[0]) == 0.0 and int(env.done[0]) == 0 and env.status[0].tolist() == [0, 0, 0]
        restart = (env.obs_num[0].cpu().numpy(), env.lasers[0].cpu().numpy(), env.target[0].cpu().numpy())
    check(restart[0], views(restart[1]), "reset", None)
    assert np.array_equal(restart[2], z["reset:target"])
    ei = env.state_field("env_int")[0].cpu().numpy()
    assert ei[abi.EI_EPISODES] == 1 and ei[abi.EI_SCEN] == 1 and ei[abi.EI_STEP_COUNT] == 0
    m = env.episode_metrics().cpu().numpy()
    assert m[abi.M_EPISODES] == 1 and m[abi.M_TIMEOUT] == (1 if timeout else 0)
    env.close()


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_pipelined_parts_match_one_batch(mode):
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    cfg, pool, n = _cfg_pool("B")
    one = _vec(cfg, pool, n, final_obs=True)
    pipe = PipelinedVecGame(n, parts=2, device="cuda:0", config=cfg, final_obs=True)
    pipe.load_scenarios(pool)
    idx = torch.arange(n, dtype=torch.int32) % pool.n
    one.reset(idx)
    pipe.reset(idx)
    tbl = _action_table(cfg, 1024, seed=3)
    n_end = 0
    for t in range(16):
        act = tbl[(torch.arange(n, device="cuda:0") * 5 + t * 17) % tbl.shape[0]].contiguous()
        one.step(act, auto_reset=mode)
        pipe.step(act, auto_reset=mode)
        pipe.join()
        for k in OUT + ("ended", "restarted") + tuple("final_" + f for f in FINAL):
            u, v = getattr(one, k), getattr(pipe, k)
            if k.startswith("final_"):
                m = one.ended.bool()
                u, v = u[m], v[m]
            assert torch.equal(u, v), (mode, t, k)
        tt1, tt2 = one.terminated_truncated(), pipe.terminated_truncated()
        assert torch.equal(tt1[0], tt2[0]) and torch.equal(tt1[1], tt2[1])
        n_end += int(one.ended.sum())
    assert n_end >= n
    assert torch.equal(one.episode_metrics(), pipe.episode_metrics())
    one.close(); pipe.close()


def test_rejections():
    cfg, pool, n = _cfg_pool("B")
    env = _vec(cfg, pool, n, final_obs=True)
    env.reset()
    act = _action_table(cfg, n)
    rc = env.lib.ftl_step_final(env.h, act.data_ptr(), abi.FTL_ACTION_BOX2, C.byref(env._out), C.byref(env._fin),
                                abi.FTL_STEP_AUTO_RESET | abi.FTL_STEP_NEXT_RESET, env._stream())
    assert rc == abi.FTL_E_INVALID
    rc = env.lib.ftl_step_encoded(env.h, act.data_ptr(), abi.FTL_ACTION_BOX2, C.byref(env._out),
                                  abi.FTL_STEP_AUTO_RESET | abi.FTL_STEP_NEXT_RESET, env._stream())
    assert rc == abi.FTL_E_INVALID
    with pytest.raises(ValueError):
        env.step(act, auto_reset="final")
    plain = _vec(cfg, pool, n)
    plain.reset()
    with pytest.raises(ValueError):
        plain.step(act, auto_reset="same_step")
    with pytest.raises(ValueError):
        plain.terminated_truncated()
    env.close(); plain.close()
