"""GPU tests of the scenario sampler (include/ftl.h: ftl_set_scenario_sampler, ftl_sampler_refresh, ftl_sampler_start,
FTL_STEP_SAMPLE_RESET; ``ScenarioSampler``, ``VecGame.set_scenario_sampler``, ``reset_from_sampler``, ``step(a, auto_reset="sample")``).

The oracle is the behaviour the library had before the sampler: batch O is reset with ``reset(scen0)``, stepped WITHOUT auto-reset, and
after every step the host calls ``reset(scen, mask=done)``, where ``scen0`` / ``scen`` come from the Python twin of the draw
(``abi.sample_scenario``) on O's OWN ``FTL_EI_RESETS`` / ``FTL_EI_STREAM`` words and the test's own cumulative sum of the weights.  Batch S
does the same with ``reset_from_sampler()`` and ``auto_reset="sample"``.  Policies are pure functions of an env's own observation row.
Every comparison is exact equality."""
import ctypes as C
import dataclasses
import json

import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import _lib, abi
from golden_util import GOLDEN, config_for, load_episode

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BASE = 5                     # the sampler's window is [5, pool.n - 4): a proper sub-window of the pool
OBS = ("obs_num", "lasers", "target")
OUT = ("reward", "done", "status")
FIELDS = ("rb_pos", "rb_dbl", "rb_int", "env_int", "env_dbl", "fol_cs", "snap_rects", "snap_win", "traj", "traj_bb", "hist", "corr",
          "corr32", "ep_stats", "hist1")
CALLS = 40


@pytest.fixture(autouse=True, params=["4 lanes per env", "8 lanes per env"])
def lanes_per_env(request, monkeypatch):
    """Both forms of the frame kernel (FTL_DEBUG_G8 at ftl_create, as tests/test_gpu_queue.py)."""
    monkeypatch.setenv("FTL_DEBUG_G8", "0" if request.param.startswith("4") else "1")
    return request.param


_POOLS, _RUNS = {}, {}


def _cfg_pool(name):
    """(cfg, pool) with episodes of a few calls: B the headline world, E random speed / acceleration regimes, F random frames per step (and
    the regimes) -- the two whose episodes depend on the slot's random streams."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    if name not in _POOLS:
        if name == "B":
            z = np.load(GOLDEN + "/pool_B.npz")
            meta = json.loads(str(z["meta"]))
            cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()), max_steps=60, warm_start=10)
            pool = ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", DEV, limit=128)
        else:
            _, meta = load_episode({"E": "E_s3_chase", "F": "F_s7_chase"}[name])
            over = {"E": dict(max_steps=80, warm_start=10, rng_seed=7), "F": dict(max_steps=150, warm_start=10, rng_seed=4)}[name]
            cfg = config_for(meta, scen_route_len=256, **over)
            pool = ScenarioPool.generate(cfg, np.arange(131), DEV)
        _POOLS[name] = (cfg, pool)
    return _POOLS[name]


def _with_base(cfg, base):
    ck = dataclasses.replace(cfg, c=abi.Config.from_buffer_copy(cfg.c))
    ck.c.env_id_base = base
    return ck


def _vec(cfg, pool, n, base=0, **kw):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    env = VecGame(n, device=DEV, config=_with_base(cfg, base), **kw)
    env.load_scenarios(pool)
    return env


def _weights(count):
    """1 .. count with a third of them zeroed."""
    w = np.arange(1, count + 1, dtype=np.int64)
    w[1::3] = 0
    return w


def _new_sampler(pool, base=BASE, count=None, weights=None):
    from continiousenvironment_follower_leader_amd import ScenarioSampler
    count = pool.n - 9 if count is None else count
    s = ScenarioSampler(count, base=base, device=DEV)
    s.set_raw_weights(torch.from_numpy(_weights(count) if weights is None else np.asarray(weights, dtype=np.int64)))
    return s


def _cumsum(weights):
    return [int(c) for c in np.cumsum(np.array([int(w) for w in weights], dtype=object))]


# ---------------------------------------------------------------- policies: action = f(the env's own observation row)
def _policy(kind, cfg):
    ms, mr, md = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed, cfg.c.min_distance
    dev = torch.device(DEV)
    if kind == "chase":
        def chase(obs):
            x = obs[0].double()
            dx, dy = x[:, 0] - x[:, 5], x[:, 1] - x[:, 6]
            want = torch.remainder(torch.rad2deg(torch.atan2(dy, dx)), 360.0)
            err = torch.remainder(want - x[:, 8] + 540.0, 360.0) - 180.0
            w = torch.clamp(err * 0.3, -mr, mr)
            dist = torch.sqrt(dx * dx + dy * dy)
            v = torch.where(dist > md * 2.4, torch.full_like(dist, ms), torch.where(dist < md * 1.5, torch.zeros_like(dist), torch.full_like(dist, 0.9 * ms)))
            return torch.stack([v, w], 1).contiguous()
        return chase
    g = torch.Generator(device="cpu").manual_seed(3)
    v = (0.4 + 0.6 * torch.rand(4093, generator=g, dtype=torch.float64)) * ms
    w = torch.clamp(torch.randn(4093, generator=g, dtype=torch.float64) * 0.4 * mr, -mr, mr)
    table = torch.stack([v, w], 1).to(dev)
    k1 = (torch.arange(abi.FTL_OBS_NUM, device=dev) * 2 + 1) * 2654435761
    k2 = (torch.arange(max(cfg.lasers_len, 1), device=dev) * 2 + 1) * 40503

    def hashed(obs):                                   # exact integer arithmetic over the bytes of the row
        h = (obs[0].view(torch.int32).long() * k1).sum(1) + (obs[1].view(torch.int32).long() * k2).sum(1)
        return table[torch.remainder(h, 4093)].contiguous()
    return hashed


# ---------------------------------------------------------------- the host side of batch O
def _host_draws(env, cdf, base, who):
    """int32 [n] scenario indices: for the envs of the bool array ``who`` the twin's draw on the env's own words, 0 elsewhere."""
    ei = env.state_field("env_int").cpu().numpy()
    seed, id0 = int(env.cfg.c.rng_seed), int(env.cfg.c.env_id_base)
    scen = np.zeros(env.n, np.int32)
    for e in np.nonzero(who)[0]:
        scen[e] = abi.sample_scenario(seed, id0 + int(e) + int(ei[e, abi.EI_STREAM]), int(ei[e, abi.EI_RESETS]), cdf, base)
    return torch.from_numpy(scen)


def _same_state(s, o, what):
    for f in FIELDS:
        a, b = s.state_field(f), o.state_field(f)
        if f == "env_int":                             # FTL_EI_EPISODES: a plain ftl_reset does not count episodes, the sampler's reset pass does.
            a, b = a.clone(), b.clone()                # FTL_EI_ERROR_STICKY is compared: every reset ORs the replaced episode's bits into it
            a[:, abi.EI_EPISODES] = 0
            b[:, abi.EI_EPISODES] = 0
        assert torch.equal(a, b), (what, f)


def _run_pair(name, n, lanes, kind="hashed"):
    """Tests 2 and 3: S against O for CALLS calls, compared at every call; returns S's table, the host recount and S's metrics."""
    key = (name, n, lanes, kind)
    if key in _RUNS:
        return _RUNS[key]
    cfg, pool = _cfg_pool(name)
    smp = _new_sampler(pool)
    count, cdf = smp.count, _cumsum(_weights(pool.n - 9))
    assert torch.equal(smp.cdf.cpu(), torch.zeros(count, dtype=torch.int64))          # (nothing builds it before the attach)
    S, O = _vec(cfg, pool, n, base=3, final_obs=True), _vec(cfg, pool, n, base=3)
    assert S.set_scenario_sampler(smp) is smp
    assert smp.cdf.cpu().tolist() == cdf
    pol = _policy(kind, cfg)
    S.reset_from_sampler()
    scen0 = _host_draws(O, cdf, BASE, np.ones(n, bool))
    assert int(scen0.min()) >= BASE and int(scen0.max()) < BASE + count
    assert bool((torch.from_numpy(_weights(count))[(scen0 - BASE).long()] > 0).all())   # a zero weight is never drawn
    O.reset(scen0)
    assert torch.equal(S.state_field("env_int")[:, abi.EI_SCEN].cpu(), scen0)
    assert int(smp._table.abs().sum()) == 0                                             # the start records nothing
    for k in OBS + OUT:
        assert torch.equal(getattr(S, k), getattr(O, k)), (name, n, "start", k)
    _same_state(S, O, (name, n, "start"))
    route_len = pool.t["route_len"].cpu().numpy()
    rec = np.zeros((count, abi.FTL_N_SCEN_STATS), np.int64)
    scen_seq, ended_total = [], 0
    for t in range(1, CALLS + 1):
        act = pol((S.obs_num, S.lasers))
        S.step(act, auto_reset="sample")
        O.step(act, auto_reset=False)
        done = O.done.bool()
        for k in OUT:
            assert torch.equal(getattr(S, k), getattr(O, k)), (name, n, t, k)
        for k in OBS:
            assert torch.equal(getattr(S, "final_" + k)[done], getattr(O, k)[done]), (name, n, t, "final_" + k)
        assert torch.equal(S.ended, O.done) and torch.equal(S.restarted, O.done), (name, n, t)
        # the host recount of the table, from O's terminal state
        d = done.cpu().numpy()
        ei, ed, st = O.state_field("env_int").cpu().numpy(), O.state_field("env_dbl").cpu().numpy(), O.status.cpu().numpy()
        for e in np.nonzero(d)[0]:
            sc = int(ei[e, abi.EI_SCEN])
            r = rec[sc - BASE]
            assert 0 <= sc - BASE < count
            r[abi.SS_EPISODES] += 1
            if route_len[sc] == 0:
                r[abi.SS_DONE_AT_RESET] += 1
                continue
            r[abi.SS_FRAMES_SUM] += int(ei[e, abi.EI_STEP_COUNT])
            r[abi.SS_RETURN_Q16] += int(np.rint(ed[e, abi.ED_OVERALL_REWARD] * 65536.0))
            r[abi.SS_SUCCESS] += st[e, 0] == abi.MISSION.index("success")
            r[abi.SS_TIMEOUT] += st[e, 0] == abi.MISSION.index("finished_by_time")
            r[abi.SS_CRASH] += st[e, 1] == abi.AGENT.index("crash")
            r[abi.SS_LOW_REWARD] += st[e, 1] == abi.AGENT.index("low_reward")
            r[abi.SS_TOO_FAR] += st[e, 1] == abi.AGENT.index("too_far_from_leader")
            r[abi.SS_LAST_CALL] = t
        ended_total += int(d.sum())
        O.reset(_host_draws(O, cdf, BASE, d), mask=done)
        for k in OBS:                                  # restarted envs: O's rows after its reset; the others: after its step
            assert torch.equal(getattr(S, k), getattr(O, k)), (name, n, t, k)
        _same_state(S, O, (name, n, t))
        scen_seq.append(S.state_field("env_int")[:, abi.EI_SCEN].cpu().numpy().copy())
    assert ended_total >= 2 * n, "the case is worth something: every slot restarted a few times"
    out = dict(table=smp._table.cpu().numpy().copy(), rec=rec, metrics=S.episode_metrics().cpu().numpy().copy(), sampler=smp,
               scen_seq=np.stack(scen_seq), ended=ended_total, episodes_word=S.state_field("env_int")[:, abi.EI_EPISODES].cpu().numpy().copy())
    S.close()
    O.close()
    _RUNS[key] = out
    return out


# ---------------------------------------------------------------- 1. the scan
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4099, 70001])
def test_scan_equals_cumsum(count):
    """Wave, workgroup-chunk and multi-chunk edges; runs of 2**32 - 1 (a prefix beyond 32 bits) and zeros; a second refresh overwrites."""
    from continiousenvironment_follower_leader_amd import ScenarioSampler
    cfg, pool = _cfg_pool("B")
    env = _vec(cfg, pool, 8)
    rng = np.random.default_rng(count)
    w = rng.integers(0, 2 ** 32, count, dtype=np.int64)
    w[rng.random(count) < 0.3] = 0
    w[rng.random(count) < 0.3] = 2 ** 32 - 1
    if count > 70:
        w[5:70] = 2 ** 32 - 1                          # a whole wavefront of the largest weight
        w[count // 2:count // 2 + 40] = 0
    s = ScenarioSampler(count, device=DEV)
    s.set_raw_weights(torch.from_numpy(w))
    want = torch.from_numpy(np.cumsum(w.astype(np.uint64)).view(np.int64))
    c = s.c_struct()                                   # (straight through the C-ABI: a window larger than the pool may be refreshed)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(env.lib.ftl_set_scenario_sampler(env.h, C.byref(c)), env.lib)
    for _ in range(2):
        _lib.check(env.lib.ftl_sampler_refresh(env.h, stream), env.lib)
        assert torch.equal(s.cdf.cpu(), want), count
    if count > 1:                                      # nothing is written past entry count - 1
        sentinel = -0x0102030405060708
        s.cdf.fill_(sentinel)
        c.count = count - 1
        _lib.check(env.lib.ftl_set_scenario_sampler(env.h, C.byref(c)), env.lib)
        _lib.check(env.lib.ftl_sampler_refresh(env.h, stream), env.lib)
        got = s.cdf.cpu()
        assert torch.equal(got[:-1], want[:-1]) and int(got[-1]) == sentinel
    if count > pool.n:                                 # the window is checked against the pool when a sampling call is issued
        assert env.lib.ftl_sampler_start(env.h, C.byref(env._out), stream) == abi.FTL_E_INVALID
        act = torch.zeros(8, 2, dtype=torch.float64, device=DEV)
        assert env.lib.ftl_step(env.h, act.data_ptr(), C.byref(env._out), abi.FTL_STEP_SAMPLE_RESET, stream) == abi.FTL_E_INVALID
    env.close()


# ---------------------------------------------------------------- 2. equivalence with what the library did before
@pytest.mark.parametrize("name, n", [("B", 133), ("B", 1045), ("E", 133), ("F", 133)])
def test_sampled_resets_equal_host_resets(name, n, lanes_per_env):
    r = _run_pair(name, n, lanes_per_env)
    # every restart was counted in the slot's episode word (the one field a plain reset leaves alone)
    assert int(r["episodes_word"].sum()) == r["ended"]
    if name in ("E", "F"):                             # the slots' own random streams went on: episodes on one scenario differ between slots
        seq = r["scen_seq"]
        assert len({tuple(seq[:, e]) for e in range(seq.shape[1])}) > seq.shape[1] // 2


# ---------------------------------------------------------------- 3. the table
@pytest.mark.parametrize("name, n", [("B", 133), ("F", 133)])
def test_table_equals_the_host_recount(name, n, lanes_per_env):
    r = _run_pair(name, n, lanes_per_env)
    for k, col in enumerate(abi.SS_NAMES):
        assert np.array_equal(r["table"][:, k], r["rec"][:, k]), (name, col)
    zero = _weights(r["table"].shape[0]) == 0
    assert (r["table"][zero] == 0).all() and r["table"][:, abi.SS_EPISODES].sum() == r["ended"]
    m, t = r["metrics"], r["table"]
    for mk, sk in ((abi.M_EPISODES, abi.SS_EPISODES), (abi.M_FRAMES_SUM, abi.SS_FRAMES_SUM), (abi.M_SUCCESS, abi.SS_SUCCESS),
                   (abi.M_CRASH, abi.SS_CRASH), (abi.M_LOW_REWARD, abi.SS_LOW_REWARD), (abi.M_TOO_FAR, abi.SS_TOO_FAR),
                   (abi.M_TIMEOUT, abi.SS_TIMEOUT)):
        assert m[mk] == float(t[:, sk].sum()), (name, mk)
    # the float sum of returns against the fixed-point one: each episode is rounded to 2**-16 (an error of at most 2**-17), and the float
    # additions of ep_stats / ftl_episode_metrics round at 2**-53 relative each
    assert abs(m[abi.M_RETURN_SUM] - t[:, abi.SS_RETURN_Q16].sum() / 65536.0) <= r["ended"] * 2.0 ** -17 + 1e-9 * abs(m[abi.M_RETURN_SUM])
    smp = r["sampler"]
    tab = smp.table(clear=True)
    for k, col in enumerate(abi.SS_NAMES):
        assert np.array_equal(tab[col].cpu().numpy(), r["table"][:, k]), col
    ep = np.maximum(r["table"][:, abi.SS_EPISODES], 1)
    assert np.array_equal(tab["mean_return"].cpu().numpy(), r["table"][:, abi.SS_RETURN_Q16] / 65536.0 / ep)
    assert np.array_equal(tab["success_rate"].cpu().numpy(), r["table"][:, abi.SS_SUCCESS] / ep)
    assert int(smp._table.abs().sum()) == 0 and all(int(v.abs().sum()) == 0 for v in smp.table().values())
    smp._table.copy_(torch.from_numpy(r["table"]))      # (the run is shared with the other tests)


# ---------------------------------------------------------------- 4. done at reset
def test_done_at_reset_counts_and_the_slot_moves_on(lanes_per_env):
    """Entry 0 of a hand-built pool has an empty route -- the world ``reset`` leaves done (ENV:508-510)."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    cfg, _ = _cfg_pool("B")
    pool = ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", DEV, limit=16)
    pool.t["route_len"][0] = 0
    n = 5
    env = _vec(cfg, pool, n, final_obs=True)
    smp = _new_sampler(pool, base=0, count=6, weights=[5, 1, 1, 1, 1, 1])
    env.set_scenario_sampler(smp)
    env.reset_from_sampler()
    scen = env.state_field("env_int")[:, abi.EI_SCEN].clone()
    assert torch.equal(env.done.bool(), scen == 0)     # done at reset, and only there
    pol = _policy("chase", cfg)
    n0 = others = 0
    for t in range(30):
        at0 = scen == 0
        resets = env.state_field("env_int")[:, abi.EI_RESETS].clone()
        env.step(pol((env.obs_num, env.lasers)), auto_reset="sample")
        assert bool(env.done[at0].bool().all()) and bool(env.restarted[at0].bool().all())       # recorded by the next call, and restarted
        assert torch.equal(env.ended, env.done) and torch.equal(env.restarted, env.done)
        assert torch.equal(env.state_field("env_int")[:, abi.EI_RESETS], resets + env.restarted.int())
        n0 += int(at0.sum())
        others += int((env.done.bool() & ~at0).sum())
        scen = env.state_field("env_int")[:, abi.EI_SCEN].clone()
    assert n0 > 0 and others > 0
    tab = smp.table()
    row0 = {k: int(v[0]) for k, v in tab.items() if k in abi.SS_NAMES}
    assert row0.pop("episodes") == n0 and row0.pop("done_at_reset") == n0 and not any(row0.values()), row0
    assert int(tab["done_at_reset"][1:].sum()) == 0 and int(tab["episodes"][1:].sum()) == others
    m = env.episode_metrics().cpu().numpy()
    assert m[abi.M_EPISODES] == n0 + others and m[abi.M_FRAMES_SUM] == int(tab["frames_sum"].sum())
    assert int(env.state_field("ep_stats")[:, abi.M_EPISODES].sum()) == n0 + others
    env.close()


# ---------------------------------------------------------------- 5. pipelined batch, one shared sampler
def test_pipelined_parts_share_one_sampler(lanes_per_env):
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    cfg, pool = _cfg_pool("B")
    n = 1045
    one = _vec(cfg, pool, n, final_obs=True)
    two = PipelinedVecGame(n, parts=2, device=DEV, config=cfg, final_obs=True)
    two.load_scenarios(pool)
    s1, s2 = _new_sampler(pool), _new_sampler(pool)
    one.set_scenario_sampler(s1)
    two.set_scenario_sampler(s2)
    assert all(g.sampler is s2 for g in two.games) and torch.equal(s1.cdf, s2.cdf)
    one.reset_from_sampler()
    two.reset_from_sampler()
    pol = _policy("hashed", cfg)
    names = OBS + OUT + ("ended", "restarted") + tuple("final_" + k for k in OBS)
    for t in range(30):
        act = pol((one.obs_num, one.lasers))
        one.step(act, auto_reset="sample")
        two.step(act, auto_reset="sample")
        two.join()
        ended = one.ended.bool()
        for k in names:
            a, b = getattr(one, k), getattr(two, k)
            if k.startswith("final_"):                 # (rows of envs that did not end keep older values)
                a, b = a[ended], b[ended]
            assert torch.equal(a, b), (t, k)
        if t in (14, 29):
            for f in FIELDS:
                assert torch.equal(one.state_field(f), two.state_field(f)), (t, f)
    assert int(s1._table[:, abi.SS_EPISODES].sum()) > n
    t1, t2 = s1.table(), s2.table()
    for k in t1:
        assert torch.equal(t1[k], t2[k]), k
    m1, m2 = one.episode_metrics().cpu().numpy(), two.episode_metrics().cpu().numpy()
    counts = [k for k in range(abi.FTL_N_METRICS) if k != abi.M_RETURN_SUM]         # (the float sum of returns depends on the split into parts)
    assert np.array_equal(m1[counts], m2[counts])
    one.close()
    two.close()


# ---------------------------------------------------------------- 6. snapshots
def test_snapshot_restores_into_another_batch(lanes_per_env):
    """A snapshot at call 10 restored into a batch of another size and base (slot_stats=False, streams kept): the restored envs replay
    the same scenario sequence and outputs for 20 more calls.  Config F: the episodes depend on the envs' random streams."""
    cfg, pool = _cfg_pool("F")
    a, b = _vec(cfg, pool, 133, base=3, final_obs=True), _vec(cfg, pool, 57, base=900, final_obs=True)
    sa, sb = _new_sampler(pool), _new_sampler(pool)
    a.set_scenario_sampler(sa)
    b.set_scenario_sampler(sb)
    pol = _policy("hashed", cfg)
    a.reset_from_sampler()
    b.reset_from_sampler()
    for t in range(10):
        a.step(pol((a.obs_num, a.lasers)), auto_reset="sample")
        b.step(pol((b.obs_num, b.lasers)), auto_reset="sample")
    src = torch.arange(0, 120, 3)                      # 40 envs of a ...
    dst = (torch.arange(40) * 10 + 3) % 57             # ... into 40 distinct slots of b
    assert torch.unique(dst).numel() == 40
    snap = a.snapshot(src)                             # (not refused: the sampler has no per-slot state)
    assert a.state_dict()["n_envs"] == 133
    b.restore(snap, dst)
    src_d, dst_d = src.to(DEV), dst.to(DEV)
    restarts = 0
    for t in range(20):
        for k in OBS + OUT:
            assert torch.equal(getattr(a, k)[src_d], getattr(b, k)[dst_d]), (t, k)
        a.step(pol((a.obs_num, a.lasers)), auto_reset="sample")
        b.step(pol((b.obs_num, b.lasers)), auto_reset="sample")
        assert torch.equal(a.state_field("env_int")[src_d, abi.EI_SCEN], b.state_field("env_int")[dst_d, abi.EI_SCEN]), t
        assert torch.equal(a.restarted[src_d], b.restarted[dst_d]) and torch.equal(a.ended[src_d], b.ended[dst_d]), t
        ended = a.ended[src_d].bool()
        restarts += int(ended.sum())
        for k in OBS:
            assert torch.equal(getattr(a, "final_" + k)[src_d][ended], getattr(b, "final_" + k)[dst_d][ended]), (t, k)
    assert restarts > 40
    b.clone([int(dst[0])], [int(dst[1])])              # (clone is not refused either)
    assert torch.equal(b.obs_num[int(dst[0])], b.obs_num[int(dst[1])])
    a.close()
    b.close()


# ---------------------------------------------------------------- 7. weights changed mid-run
def test_weights_changed_mid_run(lanes_per_env):
    """The draws of the calls after ``set_weights`` follow the new cdf, those up to it the old one; all-zero weights give the uniform form."""
    cfg, pool = _cfg_pool("B")
    n = 133
    env = _vec(cfg, pool, n, base=3)
    smp = _new_sampler(pool)
    count = smp.count
    env.set_scenario_sampler(smp)
    env.reset_from_sampler()
    pol = _policy("hashed", cfg)
    seed, id0 = int(cfg.c.rng_seed), 3
    g = torch.Generator().manual_seed(11)
    phases = [None, torch.rand(count, generator=g, dtype=torch.float64) * (torch.rand(count, generator=g) < 0.5), torch.zeros(count)]
    per_phase = -(-cfg.c.max_steps // cfg.c.frames_per_step) + 1   # calls of the longest episode (the time limit ends it), and one more
    assert per_phase <= 20
    seen = []
    for w in phases:
        if w is not None:
            smp.set_weights(w)                         # (rebuilds the cdf through the batch it is attached to)
        raw = smp.raw_weights().cpu().tolist()
        cdf = _cumsum(raw)
        assert smp.cdf.cpu().tolist() == cdf
        drawn = []
        for t in range(per_phase):
            ei = env.state_field("env_int")
            resets, stream = ei[:, abi.EI_RESETS].cpu().numpy().copy(), ei[:, abi.EI_STREAM].cpu().numpy().copy()
            env.step(pol((env.obs_num, env.lasers)), auto_reset="sample")
            new = env.state_field("env_int")[:, abi.EI_SCEN].cpu().numpy()
            for e in np.nonzero(env.done.cpu().numpy())[0]:
                want = abi.sample_scenario(seed, id0 + int(e) + int(stream[e]), int(resets[e]), cdf, BASE)
                assert new[e] == want, (t, e)
                drawn.append(int(new[e]) - BASE)
        assert len(drawn) >= n                         # (an episode ends at max_steps frames at the latest: every slot drew in this phase)
        if sum(raw):
            assert all(raw[i] > 0 for i in drawn)
        seen.append(set(drawn))
    zero0 = {i for i, w in enumerate(_weights(count)) if w == 0}
    assert not (seen[0] & zero0) and (seen[2] & zero0)         # the uniform phase reaches entries the first phase never could
    env.close()


# ---------------------------------------------------------------- 8. detach: nothing else moved
@pytest.mark.parametrize("name", ["B", "F"])
def test_old_flags_after_attach_and_detach(name):
    cfg, pool = _cfg_pool(name)
    n = 96
    a, b = _vec(cfg, pool, n, final_obs=True), _vec(cfg, pool, n, final_obs=True)
    b.set_scenario_sampler(_new_sampler(pool))
    assert b.set_scenario_sampler(None) is None and b.sampler is None
    with pytest.raises(_lib.FtlError):
        b.step(torch.zeros(n, 2, dtype=torch.float64, device=DEV), auto_reset="sample")
    with pytest.raises(_lib.FtlError):
        b.reset_from_sampler()
    idx = torch.arange(n, dtype=torch.int32) % pool.n
    pol = _policy("hashed", cfg)
    for e in (a, b):
        e.reset(idx)
    for t in range(24):
        mode = (True, "same_step", "next_step", False)[(t // 6) % 4]
        act = pol((a.obs_num, a.lasers))
        a.step(act, auto_reset=mode)
        b.step(act, auto_reset=mode)
        for k in OBS + OUT + ("ended", "restarted"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (name, t, k)
    for f in FIELDS:
        assert torch.equal(a.state_field(f), b.state_field(f)), (name, f)
    assert torch.equal(a.episode_metrics(), b.episode_metrics())
    a.close()
    b.close()
