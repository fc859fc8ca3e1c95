"""GPU tests of snapshot / clone / restore (include/ftl.h: ftl_pack_envs, ftl_unpack_envs; VecGame.snapshot / restore / clone /
state_dict / load_state_dict, PipelinedVecGame, Game.clone_state / restore_state).

The yardstick is replay: an env copied into another slot (or brought back later) and stepped with the same actions returns the same
outputs and reaches the same state, bit for bit, as its source -- through random draws (configs E and F: leader speed regimes, random
frame counts), auto-resets and other slots' histories."""
import dataclasses
import io
import json

import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import GOLDEN, config_for, load_episode

pytestmark = pytest.mark.gpu

OUT = ("obs_num", "lasers", "target", "reward", "done", "status")
FIELDS = ("rb_pos", "rb_dbl", "rb_int", "env_int", "env_dbl", "traj", "hist", "corr", "snap_rects", "snap_win", "traj_bb", "ep_stats",
          "hist1", "fol_cs", "corr32")
EPISODE_FIELDS = tuple(f for f in FIELDS if f != "ep_stats")          # ep_stats belongs to the slot
SLOT_WORDS = (abi.EI_EPISODES, abi.EI_ERROR_STICKY, abi.EI_STREAM)      # env_int words of the slot (the stream word: relative to it)
EPISODES = {"B": "B_s1_chase", "D": "D_s2_chase", "E": "E_s3_chase", "F": "F_s1_chase", "L": "L_s2_chase", "T": "T_s3_chase"}

_POOLS = {}


def _cfg_pool(name, long=False):
    """(cfg, pool) with episodes short enough for several auto-resets in the steps below (max_steps in frames); ``long``: episodes of
    about 80 steps, which only early endings cut short."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    if (name, long) not in _POOLS:
        if name == "B":
            z = np.load(GOLDEN + "/pool_B.npz")
            meta = json.loads(str(z["meta"]))
            cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()), max_steps=800 if long else 150,
                             warm_start=10)
            pool = ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0")
        else:
            _, meta = load_episode(EPISODES[name])
            over = {"E": dict(max_steps=400 if long else 100, warm_start=5, rng_seed=3),
                    "F": dict(max_steps=2500 if long else 400, warm_start=10, rng_seed=4)}.get(name, dict(max_steps=800 if long else 150, warm_start=10))
            cfg = config_for(meta, scen_route_len=256, **over)
            pool = ScenarioPool.generate(cfg, np.arange(131), "cuda:0", n_threads=8)
        _POOLS[(name, long)] = (cfg, pool)
    return _POOLS[(name, long)]


def _vec(cfg, pool, n, **kw):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    try:
        env = VecGame(n, device="cuda:0", config=cfg, policy_obs=True, **kw)
    except ValueError:                  # sensors without a common history: no fused policy output
        env = VecGame(n, device="cuda:0", config=cfg, **kw)
    env.load_scenarios(pool)
    env.reset(torch.arange(n, dtype=torch.int32) % pool.n)
    return env


def _actions(cfg, n, t, seed=0):
    """Actions of step t for n envs in the config's action space (deterministic)."""
    g = torch.Generator(device="cpu").manual_seed(seed * 100003 + t)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    if cfg.discrete_action_space:
        return torch.randint(0, 5, (n,), generator=g, dtype=torch.int32).cuda()
    w = torch.clamp(torch.randn(n, generator=g, dtype=torch.float64) * 0.4 * mr, -mr, mr)
    if cfg.constant_follower_speed:
        return w.cuda()
    v = (0.3 + 0.7 * torch.rand(n, generator=g, dtype=torch.float64)) * ms
    return torch.stack([v, w], 1).contiguous().cuda()


def _outs(env):
    names = OUT + (("policy_obs",) if env.policy_obs is not None else ())
    return {k: getattr(env, k) for k in names}


def _assert_rows_equal(env, a, b, tag, fields=EPISODE_FIELDS):
    """Outputs and episode state of envs a equal those of envs b (bit for bit; slot words excluded)."""
    for k, t in _outs(env).items():
        assert torch.equal(t[a], t[b]), (tag, k)
    keep = torch.ones(abi.EI_COUNT, dtype=torch.bool, device="cuda:0")
    keep[list(SLOT_WORDS)] = False
    for f in fields:
        x = env.state_field(f)
        if f == "env_int":
            assert torch.equal(x[a][:, keep], x[b][:, keep]), (tag, f)
        else:
            assert torch.equal(x[a], x[b]), (tag, f)


def _pairs(env, rng, want):
    """Disjoint (src, dst) pairs of live envs where dst's trajectory is longer and its slot was reset more often than src's: sources in
    random order, each matched with the least dominating free destination (keeps the dominant ones for the sources that need them)."""
    ei = env.state_field("env_int").cpu().numpy()
    live = np.nonzero(ei[:, abi.EI_DONE] == 0)[0]
    tl, rs = ei[:, abi.EI_TRAJ_LEN].astype(np.int64), ei[:, abi.EI_RESETS].astype(np.int64)
    free = set(int(e) for e in live)
    src, dst = [], []
    for s in sorted(live, key=lambda e: (-rs[e], -tl[e], rng.random())):      # the hardest sources first
        s = int(s)
        if len(src) == want or s not in free:
            continue
        cand = [d for d in free if tl[d] > tl[s] and rs[d] > rs[s]]
        if cand:
            d = min(cand, key=lambda e: (rs[e], tl[e]))
            free.discard(s); free.discard(d)
            src.append(s); dst.append(d)
    order = rng.permutation(len(src))
    return np.array(src)[order], np.array(dst)[order]


@pytest.mark.parametrize("name", sorted(EPISODES))
@pytest.mark.parametrize("mode", ["4 lanes", "8 lanes", "no regroup", "regroup"])
def test_clone_replay(name, mode, monkeypatch):
    if mode in ("4 lanes", "8 lanes"):
        monkeypatch.setenv("FTL_DEBUG_G8", "0" if mode == "4 lanes" else "1")
    else:
        monkeypatch.setenv("FTL_NO_REGROUP", "1" if mode == "no regroup" else "0")
    cfg, pool = _cfg_pool(name, long=True)
    n = 512
    env = _vec(cfg, pool, n)
    for t in range(30):
        env.step(_actions(cfg, n, t), auto_reset=True)
        if t == 0:                  # half of the slots start over once more: destinations with more resets and longer trajectories
            env.reset((torch.arange(n, dtype=torch.int32) * 7 + 3) % pool.n, mask=(torch.arange(n) >= n // 2).to(torch.uint8))
    rng = np.random.default_rng(7)
    src, dst = _pairs(env, rng, 48)
    assert len(src) >= 16, "too few (src, dst) pairs with a longer trajectory and more resets at dst"
    ei0 = env.state_field("env_int").clone()
    own = name in ("E", "F")
    if own:                             # half of the pairs keep the destination's own stream: those must diverge
        h = len(src) // 2
        env.clone(src[:h], dst[:h])
        env.clone(src[h:], dst[h:], own_stream=True)
        src_o, dst_o, src, dst = src[h:], dst[h:], src[:h], dst[:h]
    else:
        env.clone(src, dst)
    ei = env.state_field("env_int")
    assert torch.equal(ei[dst][:, abi.EI_EPISODES], ei0[dst][:, abi.EI_EPISODES])     # slot words stay
    assert torch.equal(ei[dst][:, abi.EI_ERROR_STICKY], ei0[dst][:, abi.EI_ERROR_STICKY])
    _assert_rows_equal(env, src, dst, (name, mode, "after clone"))
    s_t, d_t = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    resets0 = ei[dst][:, abi.EI_RESETS].clone()
    diverged = False
    for t in range(30, 110):
        a = _actions(cfg, n, t)
        a[d_t] = a[s_t]
        if own:
            a[torch.from_numpy(dst_o).cuda()] = a[torch.from_numpy(src_o).cuda()]
        env.step(a, auto_reset=True)
        _assert_rows_equal(env, src, dst, (name, mode, t))
        if own and not diverged:
            diverged = not torch.equal(env.obs_num[dst_o], env.obs_num[src_o]) or \
                not torch.equal(env.state_field("rb_pos")[dst_o], env.state_field("rb_pos")[src_o])
    assert bool((env.state_field("env_int")[dst][:, abi.EI_RESETS] > resets0).any()), "no cloned env went through an auto-reset"
    if own:
        assert diverged, "own_stream clones never diverged: the stream word is not what keys the random draws"
    env.close()


def test_overlapping_clone_equals_snapshot_restore():
    cfg, pool = _cfg_pool("B")
    n = 512
    a, b = _vec(cfg, pool, n), _vec(cfg, pool, n)
    for t in range(20):
        for e in (a, b):
            e.step(_actions(cfg, n, t), auto_reset=True)
    src = np.random.default_rng(3).permutation(n)[:96]
    dst = np.roll(src, 1)
    a.clone(src, dst)
    b.restore(b.snapshot(src), dst)
    for f in FIELDS:
        assert torch.equal(a.state_field(f), b.state_field(f)), f
    for k in _outs(a):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for e in (a, b):
        e.close()


def _record(env):
    names = list(env.output_rows())
    return {k: getattr(env, k).clone() for k in names}


@pytest.mark.parametrize("name,auto", [("B", "next_step"), ("B", "same_step"), ("F", "next_step"), ("F", True)])
def test_snapshot_restore_replay(name, auto):
    cfg, pool = _cfg_pool(name)
    n = 256
    env = _vec(cfg, pool, n, final_obs=True)
    rec, snap = [], None
    for t in range(50):
        if t == 20:
            snap = env.snapshot()
            if auto == "next_step":
                assert bool(env.done.any()), "no env is done on entry at the snapshot"
        env.step(_actions(cfg, n, t), auto_reset=auto)
        rec.append(_record(env))
    if auto == "same_step":
        assert any(bool(r["ended"].any()) for r in rec[20:]), "no episode ended after the snapshot"
    env.restore(snap.cpu())           # (through the host: the copy is what a saved snapshot brings back)
    for t in range(20, 50):
        env.step(_actions(cfg, n, t), auto_reset=auto)
        got = _record(env)
        for k, v in rec[t].items():
            if auto is True and k in ("final_obs_num", "final_lasers", "final_target", "final_policy_obs"):
                continue                  # auto_reset=True does not write the final buffers
            assert torch.equal(got[k], v), (name, auto, t, k)
    env.close()


def test_slot_accounting():
    cfg, pool = _cfg_pool("B")
    n = 512
    env = _vec(cfg, pool, n)
    for t in range(30):
        env.step(_actions(cfg, n, t), auto_reset=True)
    src, dst = np.arange(0, 32), np.arange(100, 132)
    ei = env.state_field("env_int")
    ei[torch.from_numpy(src).cuda(), abi.EI_ERROR_STICKY] = abi.FTL_ERR_TRAJ_OVERFLOW      # a sticky word to move (or not)
    m0 = env.episode_metrics().clone()
    err0 = env.error_report()
    ep0, ei0 = env.state_field("ep_stats").clone(), ei.clone()
    assert not torch.equal(ep0[src], ep0[dst])
    env.clone(src, dst)
    assert torch.equal(env.episode_metrics(), m0)
    assert env.error_report() == err0
    assert torch.equal(env.state_field("ep_stats")[dst], ep0[dst])
    for w in (abi.EI_EPISODES, abi.EI_ERROR_STICKY):
        assert torch.equal(env.state_field("env_int")[dst][:, w], ei0[dst][:, w])
    dst2 = np.arange(200, 232)
    env.clone(src, dst2, slot_stats=True)
    assert torch.equal(env.state_field("ep_stats")[dst2], ep0[src])
    for w in (abi.EI_EPISODES, abi.EI_ERROR_STICKY):
        assert torch.equal(env.state_field("env_int")[dst2][:, w], ei0[src][:, w])
    assert env.error_report()[0] == int((env.state_field("env_int")[:, abi.EI_ERROR_STICKY] != 0).sum())
    env.close()


def test_checkpoint_and_reshard():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    cfg, pool = _cfg_pool("F")
    n = 4096
    ref = _vec(cfg, pool, n)
    for t in range(40):
        ref.step(_actions(cfg, n, t, seed=5), auto_reset=True)
    buf = io.BytesIO()
    torch.save(ref.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    rec = []
    for t in range(40, 80):
        ref.step(_actions(cfg, n, t, seed=5), auto_reset=True)
        rec.append({k: getattr(ref, k).clone() for k in OUT})
    final = {f: ref.state_field(f).clone() for f in FIELDS}

    def check(outs_at, fields, tag):
        for t in range(40):
            got = outs_at(t)
            for k in OUT:
                assert torch.equal(got[k], rec[t][k]), (tag, t, k)
        for f in FIELDS:
            assert torch.equal(fields(f), final[f]), (tag, f)

    fresh = VecGame(n, device="cuda:0", config=cfg)
    fresh.load_scenarios(pool)
    fresh.load_state_dict(sd)
    steps = []
    for t in range(40, 80):
        fresh.step(_actions(cfg, n, t, seed=5), auto_reset=True)
        steps.append({k: getattr(fresh, k).clone() for k in OUT})
    check(lambda t: steps[t], fresh.state_field, "VecGame(4096)")

    pipe = PipelinedVecGame(n, parts=2, device="cuda:0", config=cfg)
    pipe.load_scenarios(pool)
    pipe.load_state_dict(sd)
    steps = []
    for t in range(40, 80):
        pipe.step(_actions(cfg, n, t, seed=5), auto_reset=True)
        pipe.join()
        steps.append({k: getattr(pipe, k).clone() for k in OUT})
    check(lambda t: steps[t], pipe.state_field, "PipelinedVecGame(4096, parts=2)")

    shards = []
    for base in (0, 2048):
        ck = dataclasses.replace(cfg, c=abi.Config.from_buffer_copy(cfg.c))
        ck.c.env_id_base = base
        g = VecGame(2048, device="cuda:0", config=ck)
        g.load_scenarios(pool)
        g.load_state_dict(sd)
        shards.append(g)
    steps = []
    for t in range(40, 80):
        a = _actions(cfg, n, t, seed=5)
        for k, g in enumerate(shards):
            g.step(a[2048 * k:2048 * (k + 1)].contiguous(), auto_reset=True)
        steps.append({k: torch.cat([getattr(g, k) for g in shards]) for k in OUT})
    check(lambda t: steps[t], lambda f: torch.cat([g.state_field(f) for g in shards]), "2 x VecGame(2048)")
    for e in [ref, fresh, pipe] + shards:
        e.close()


def test_game_facade_clone_restore():
    from continiousenvironment_follower_leader_amd.game import Game
    g = Game(max_steps=400)
    g.seed(3)
    g.reset()
    rng = np.random.default_rng(0)
    lo, hi = g.action_space.low, g.action_space.high
    for _ in range(5):
        g.step(rng.uniform(lo, hi))
    s = g.clone_state()
    acts = [rng.uniform(lo, hi) for _ in range(50)]

    def run():
        return [g.step(a) for a in acts]

    def eq(x, y):
        if isinstance(x, (tuple, list)):
            return len(x) == len(y) and all(eq(a, b) for a, b in zip(x, y))
        if isinstance(x, np.ndarray):
            return x.dtype == y.dtype and np.array_equal(x, y)
        return x == y

    def same(r1, r2):
        for (o1, rw1, d1, i1), (o2, rw2, d2, i2) in zip(r1, r2):
            assert list(o1) == list(o2)
            for k in o1:
                assert eq(o1[k], o2[k]), k
            assert rw1 == rw2 and d1 == d2 and i1 == i2

    first = run()
    state_after = (g.done, g.simulation_number)
    g.restore_state(s)
    same(first, run())
    assert (g.done, g.simulation_number) == state_after
    g.reset()                             # a new generated world replaces the pool
    g.restore_state(s)
    assert g.simulation_number == s["simulation_number"]
    same(first, run())
    g.close()


def test_rejections_leave_state_untouched():
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg, pool = _cfg_pool("B")
    n = 64
    env = _vec(cfg, pool, n)
    for t in range(5):
        env.step(_actions(cfg, n, t), auto_reset=True)
    snap = env.snapshot([1, 2])
    wide = dataclasses.replace(cfg, c=abi.Config.from_buffer_copy(cfg.c))
    wide.c.traj_cap += 64                                              # another layout
    other = VecGame(n, device="cuda:0", config=wide)
    other.load_scenarios(pool)
    foreign = other.snapshot([0, 1])
    torch.cuda.synchronize()
    state0 = env.state.clone()
    outs0 = {k: v.clone() for k, v in env.output_rows().items()}

    def untouched():
        torch.cuda.synchronize()
        assert torch.equal(env.state, state0)
        for k, v in env.output_rows().items():
            assert torch.equal(v, outs0[k]), k

    for call in (lambda: env.snapshot([n]), lambda: env.snapshot([-1]), lambda: env.restore(snap, [0, n]),
                 lambda: env.clone([0], [n]), lambda: env.clone([n], [0]),
                 lambda: env.clone([0, 1], [2, 2]), lambda: env.restore(snap, [3, 3]), lambda: env.restore(snap, [3]),
                 lambda: env.restore(foreign, [3, 4])):
        with pytest.raises(ValueError):
            call()
        untouched()
    pool.write(0, {k: v[0:1].cpu() for k, v in pool.t.items()})       # same contents, but written: a new version
    with pytest.raises(ValueError):
        env.restore(snap, [3, 4])
    untouched()
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    env.load_scenarios(ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0"))
    fresh_snap = env.snapshot([1, 2])
    env.load_scenarios(pool)
    with pytest.raises(ValueError):                                    # another pool object
        env.restore(fresh_snap, [3, 4])
    untouched()
    env.restore(env.snapshot([1, 2]), [3, 4])                          # and a snapshot of the current pool goes through
    other.close()
    env.close()


def test_render_of_a_clone_equals_its_source():
    cfg, pool = _cfg_pool("B")
    n = 64
    env = _vec(cfg, pool, n)
    for t in range(12):
        env.step(_actions(cfg, n, t), auto_reset=True)
    env.clone([5, 6], [40, 41])
    img = env.render([5, 6, 40, 41], scale=2.0)
    assert torch.equal(img[0], img[2]) and torch.equal(img[1], img[3])
    env.step(_actions(cfg, n, 12).index_copy_(0, torch.tensor([40, 41], device="cuda:0"),
                                              _actions(cfg, n, 12)[[5, 6]]), auto_reset=True)
    img = env.render([5, 6, 40, 41])
    assert torch.equal(img[0], img[2]) and torch.equal(img[1], img[3])
    env.close()
