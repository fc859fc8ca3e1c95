"""The v2 tracker's trim from a running corridor length (csrc/ftl_trktrim.hpp, g_sensors in csrc/ftl_frames_group.hpp).

A saving scan of LeaderPositionsTracker_v2 pops history points while numpy's pairwise sum of the window's segment lengths exceeds
corridor_length (sensors.py:288-297).  The frame kernel keeps the length of the window per env -- FTL_RI_SPARE0/1 of robot 0 hold the
words of the float64 W, those of robot 1 the window (corr_lo, corr_hi) it belongs to -- and evaluates the pairwise sum only when W lies
within a rounding band of the threshold.  FTL_TRK_RUNNING=0 is the twin: both full sums in every saving scan, no length kept.

Here: the default against the twin, bit for bit in every output and every state field except those four words, at every step -- config B
in both lane forms, with the band widened to 3 px (FTL_DEBUG_TRK_BAND: a large share of the decisions falls back to the sum), on the
shapes where the sum changes form (one frame per step: windows of 260 points, the recursion above 128 terms; saving periods 1 and 4; seeded
float64 points or none; config E's crawling leader; a leader that has finished), and across snapshot / restore / clone; the kept length
itself against the in-order float64 sum computed in numpy; and corridor lengths ON the float32 sum of a steady window (and its two
float32 neighbours) against the CPU oracle."""
import copy
import json

import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import config_for, load_episode
from oracle_batch import OracleBatch, pool_scenarios
from test_gpu_configs import _actions, _vec

pytestmark = pytest.mark.gpu

OUTS = ("obs_num", "lasers", "target", "reward", "done", "status")
FIELDS = ("rb_pos", "rb_dbl", "rb_int", "env_int", "env_dbl", "traj", "hist", "corr", "snap_rects", "snap_win", "traj_bb", "ep_stats",
          "hist1", "fol_cs", "corr32")
_POOLS = {}


def _t(a, dtype=torch.float64):
    return torch.tensor(a, dtype=dtype, device="cuda:0")


def _cfg_pool(ep, tracker=None, pool=True, **over):
    """(cfg, pool of 96 generated scenarios -- None without `pool`) of golden episode `ep`, the v2 tracker's keyword arguments updated
    by `tracker`."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    key = (ep, json.dumps(tracker, sort_keys=True), json.dumps(over, sort_keys=True), pool)
    if key not in _POOLS:
        _, meta = load_episode(ep)
        meta = copy.deepcopy(meta)
        if tracker:
            sensors = meta["kwargs"]["follower_sensors"]
            name = [k for k, v in sensors.items() if v.get("sensor_class") == "LeaderPositionsTracker_v2"][0]
            sensors[name].update(tracker)
        cfg = config_for(meta, scen_route_len=256, **over)
        assert cfg.c.has_tracker == 2
        _POOLS[key] = (cfg, ScenarioPool.generate(cfg, np.arange(96), "cuda:0") if pool else None)
    return _POOLS[key]


def _short_routes(pool, keep):
    """The pool with every route cut to its first `keep` way-points: the leader arrives within a few dozen steps."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    p = ScenarioPool.__new__(ScenarioPool)
    p.n = pool.n
    p.t = {k: v.clone() for k, v in pool.t.items()}
    p.t["route_len"].clamp_(max=keep)
    p._bind()
    return p


def _words(env, cfg):
    """(W [n] float64, tag_lo [n], tag_hi [n]) as the state holds them"""
    ri = env.state_field("rb_int").cpu().numpy().reshape(env.n, cfg.n_robots, abi.RI_COUNT)
    hi = ri[:, 0, abi.RI_SPARE0].astype(np.int64) & 0xFFFFFFFF
    lo = ri[:, 0, abi.RI_SPARE1].astype(np.int64) & 0xFFFFFFFF
    w = ((hi << 32) | lo).astype(np.uint64).view(np.float64)
    return w, ri[:, 1, abi.RI_SPARE0].copy(), ri[:, 1, abi.RI_SPARE1].copy()


def _state(env, cfg):
    """every state field, the four words of the running length zeroed"""
    out = {}
    for f in FIELDS:
        x = env.state_field(f).clone()
        if f == "rb_int":
            x.view(env.n, cfg.n_robots, abi.RI_COUNT)[:, :2, abi.RI_SPARE0:abi.RI_SPARE1 + 1] = 0
        out[f] = x
    return out


def _same(a, b, cfg, tag):
    for name in OUTS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (tag, name)
    sa, sb = _state(a, cfg), _state(b, cfg)
    for f in FIELDS:
        assert torch.equal(sa[f], sb[f]), (tag, f)


def _valid(env, cfg):
    """(envs whose kept length belongs to their window [n] bool, W [n])"""
    ei = env.state_field("env_int").cpu().numpy()
    w, tlo, thi = _words(env, cfg)
    return (thi > tlo) & (tlo == ei[:, abi.EI_CORR_LO]) & (thi == ei[:, abi.EI_CORR_HI]), w


def _twins(monkeypatch, n, cfg, pool, **env):
    """(default handle, FTL_TRK_RUNNING=0 handle), both created under the switches `env`"""
    monkeypatch.delenv("FTL_TRK_RUNNING", raising=False)
    monkeypatch.delenv("FTL_DEBUG_TRK_BAND", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = _vec(n, cfg, pool)
    monkeypatch.setenv("FTL_TRK_RUNNING", "0")
    b = _vec(n, cfg, pool)
    monkeypatch.delenv("FTL_TRK_RUNNING")
    return a, b


def _run_twins(monkeypatch, cfg, pool, n, steps, tag, seed, env=None, watch=None):
    """reset + `steps` steps with auto-reset of the default and the twin, everything equal after every call; returns the share of
    (env, step) pairs in which the default held a length that belongs to its window, and whatever `watch(a)` summed up."""
    a, b = _twins(monkeypatch, n, cfg, pool, **(env or {}))
    idx = torch.from_numpy(((np.arange(n) * 3) % pool.n).astype(np.int32))
    a.reset(idx); b.reset(idx)
    _same(a, b, cfg, (tag, "reset"))
    held, seen = 0, 0
    for t in range(steps):
        act = _t(_actions(cfg, n, t, "mixed" if t % 2 else "random", seed=seed))
        a.step(act, auto_reset=True); b.step(act, auto_reset=True)
        _same(a, b, cfg, (tag, t))
        held += int(_valid(a, cfg)[0].sum())
        if watch is not None:
            seen += int(watch(a))
    vb = _valid(b, cfg)[0]
    assert not vb.any(), (tag, "the twin keeps a length")
    assert a.error_report() == b.error_report(), tag
    a.close(); b.close()
    return held / float(n * steps), seen


@pytest.mark.parametrize("lanes", ["4 lanes per env", "8 lanes per env"])
@pytest.mark.parametrize("band", [None, "3"])
def test_config_b_equals_the_twin_at_every_step(monkeypatch, lanes, band):
    """Config B, 64 envs, 150 steps with auto-reset, both lane forms; once more with a band of 3 px, where a large share of the trim
    decisions is handed to the pairwise sum."""
    cfg, pool = _cfg_pool("B_s1_chase")
    env = {"FTL_DEBUG_G8": "0" if lanes.startswith("4") else "1"}
    if band:
        env["FTL_DEBUG_TRK_BAND"] = band
    share, _ = _run_twins(monkeypatch, cfg, pool, 64, 150, ("B", lanes, band), seed=61, env=env)
    print("a length was held in %.1f %% of the env-steps" % (100 * share))
    assert share > 0, "no length was ever held: the two sides ran the same code"


def _inorder_f64(hist, lo, hi, cap, f64):
    """the in-order float64 sum of the window's segment lengths in the array's dtype (float64 while a seed point is inside)"""
    p = hist[np.arange(lo, hi) & (cap - 1)]
    if f64:
        d = p[:-1] - p[1:]
        seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    else:
        q = p.astype(np.float32)
        d = q[:-1] - q[1:]
        seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float64)
        assert seg.dtype == np.float64 and d.dtype == np.float32
    w = 0.0
    for v in seg:
        w += float(v)
    return w


@pytest.mark.parametrize("behind", [True, False])
def test_the_kept_length_is_alive_and_exact(behind):
    """After step 60 (and again after step 140, when config B's seeded float64 points have left every window): the length belongs to the
    window in at least 90 % of the envs -- otherwise the short-cut is dead code --, and where it does it EQUALS the in-order float64 sum
    of the window's segment lengths computed here."""
    cfg, pool = _cfg_pool("B_s1_chase", tracker=dict(start_corridor_behind_follower=behind))
    assert cfg.c.tracker_start_behind == (1 if behind else 0)
    n = 64
    env = _vec(n, cfg, pool)
    env.reset(torch.from_numpy(((np.arange(n) * 3) % pool.n).astype(np.int32)))
    cap = cfg.c.corr_cap
    for t in range(140):
        env.step(_t(_actions(cfg, n, t, "mixed" if t % 2 else "random", seed=63)), auto_reset=True)
        if t + 1 not in (60, 140):
            continue
        ok, w = _valid(env, cfg)
        ei = env.state_field("env_int").cpu().numpy()
        hist = env.state_field("hist").cpu().numpy().reshape(n, cap, 2)
        seeded = 0
        for e in np.flatnonzero(ok):
            lo, hi = int(ei[e, abi.EI_CORR_LO]), int(ei[e, abi.EI_CORR_HI])
            f64 = lo < int(ei[e, abi.EI_SEED_END])
            seeded += int(f64)
            want = _inorder_f64(hist[e], lo, hi, cap, f64)
            if f64:        # a rounded sum kept through appends and pops: within the seed band of the kernel (1e-8 px), not bit for bit
                assert abs(w[e] - want) < 1e-9, (t + 1, e, w[e], want)
            else:
                assert w[e] == want, (t + 1, e, w[e], want)
        print("step %d: length held by %d of %d envs (%d with seed points in the window)" % (t + 1, int(ok.sum()), n, seeded))
        assert ok.sum() >= 0.9 * n, "the running length is dead code: held by %d of %d envs after step %d" % (int(ok.sum()), n, t + 1)
    assert env.error_report() == (0, 0)
    env.close()


def _steady_window_sum(cfg, scen, steps, seed):
    """float32 pairwise sum (numpy's) of env 0's history window after `steps` oracle steps (env 0 of a batch of 16 playing scenario 0)"""
    ora = OracleBatch(cfg, 1)
    ora.reset(scen, [0])
    for t in range(steps):
        ora.step(_actions(cfg, 16, t, "mixed" if t % 2 else "random", seed=seed)[:1])
    d = ora.envs[0].debug()
    assert not d["hist_isf64"].any() and len(d["hist"]) > 8, "not a steady float32 window"
    h = d["hist"].astype(np.float32)
    seg = np.sqrt(((h[:-1] - h[1:]) ** 2).sum(1, dtype=np.float32))
    assert seg.dtype == np.float32
    return np.sum(seg)


def test_knife_edge_corridor_lengths_match_the_oracle():
    """corridor_length ON the float32 pairwise sum of a window the episode really reaches, and on its two float32 neighbours: the trim of
    that step is decided inside the band.  16 envs (env 0 plays the scenario the length was taken from) from reset, oracle and device:
    the window -- its length and its points, i.e. corr_lo and corr_hi -- equal at every step."""
    base, pool = _cfg_pool("B_s1_chase", tracker=dict(start_corridor_behind_follower=False))
    scen = pool_scenarios(pool)
    steps = 40
    p = _steady_window_sum(base, scen, steps, seed=65)
    assert p.dtype == np.float32 and 50.0 < float(p) <= 250.0, p
    n = 16
    for L in (float(p), float(np.nextafter(p, np.float32(np.inf))), float(np.nextafter(p, np.float32(-np.inf)))):
        cfg, _ = _cfg_pool("B_s1_chase", tracker=dict(start_corridor_behind_follower=False, corridor_length=L), pool=False)
        assert cfg.c.corridor_length == L
        env = _vec(n, cfg, pool)
        idx = np.arange(n) % pool.n
        env.reset(torch.from_numpy(idx.astype(np.int32)))
        ora = OracleBatch(cfg, n)
        ora.reset(scen, idx)
        cap = cfg.c.corr_cap
        for t in range(steps + 10):
            a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=65)
            env.step(_t(a)); ora.step(a)
            ei = env.state_field("env_int").cpu().numpy()
            hist = env.state_field("hist").cpu().numpy().reshape(n, cap, 2)
            for e in range(n):
                want = ora.envs[e].debug()["hist"]
                lo, hi = int(ei[e, abi.EI_CORR_LO]), int(ei[e, abi.EI_CORR_HI])
                assert hi - lo == len(want), (L, t, e, "window length", hi - lo, len(want))
                got = hist[e][np.arange(lo, hi) & (cap - 1)]
                assert np.array_equal(got[[0, -1]], want[[0, -1]]), (L, t, e, "window ends")
        ok, _ = _valid(env, cfg)
        assert ok.sum() >= n // 2, (L, "no length held")
        env.close()


SHAPES = {
    "one frame per step": ("B_s1_chase", None, dict(frames_per_step=1), 64, None),
    "saving period 1": ("B_s1_chase", dict(saving_period=1), {}, 32, None),
    "saving period 4": ("B_s1_chase", dict(saving_period=4), {}, 32, None),
    "no seed points": ("B_s1_chase", dict(start_corridor_behind_follower=False), {}, 32, None),
    "config E": ("E_s3_chase", None, dict(rng_seed=9, env_id_base=17000), 64, None),
    "leader finished": ("B_s1_chase", None, {}, 32, 3),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_where_the_sum_changes_form_equal_the_twin(monkeypatch, shape):
    """120 steps with auto-reset, default against twin, on: one frame per step (windows grow towards 260 points: the pairwise sum recurses
    above 128 terms); saving periods 1 and 4; no float64 seed points (config B seeds them: the other tests cover that); config E, whose
    regimes let the leader crawl; routes of three way-points, after which the leader stands still and the saves are skipped."""
    ep, tracker, over, n, keep = SHAPES[shape]
    cfg, pool = _cfg_pool(ep, tracker=tracker, **over)
    if keep:
        pool = _short_routes(pool, keep)
    watch = (lambda a: (a.state_field("env_int")[:, abi.EI_LEADER_FINISHED] != 0).sum().item()) if keep else None
    share, seen = _run_twins(monkeypatch, cfg, pool, n, 120, shape, seed=67, watch=watch)
    print("%s: a length was held in %.1f %% of the env-steps" % (shape, 100 * share))
    if keep:
        print("env-steps with a finished leader: %d" % seen)
        assert seen > 0, "no leader finished: the case did not happen"
    assert share > 0, (shape, "no length was ever held: the two sides ran the same code")


def test_one_frame_per_step_windows_pass_128_points(monkeypatch):
    """The window of one frame per step passes 128 points (the leaf of numpy's pairwise recursion) only after some 150 steps of one
    episode: 500 steps without auto-reset (an env that is done goes on being stepped, as in the reference), default against twin every
    8th step, and the length still exact at the end."""
    cfg, pool = _cfg_pool("B_s1_chase", None, frames_per_step=1)
    n = 32
    a, b = _twins(monkeypatch, n, cfg, pool)
    idx = torch.from_numpy(((np.arange(n) * 3) % pool.n).astype(np.int32))
    a.reset(idx); b.reset(idx)
    for t in range(500):
        act = _t(_actions(cfg, n, t, "mixed" if t % 2 else "random", seed=69))
        a.step(act); b.step(act)
        if t % 8 == 7:
            _same(a, b, cfg, ("long", t))
    ei = a.state_field("env_int").cpu().numpy()
    longest = int((ei[:, abi.EI_CORR_HI] - ei[:, abi.EI_CORR_LO]).max())
    print("longest window: %d points" % longest)
    assert longest > 128, longest
    ok, w = _valid(a, cfg)
    hist = a.state_field("hist").cpu().numpy().reshape(n, cfg.c.corr_cap, 2)
    for e in np.flatnonzero(ok):
        lo, hi = int(ei[e, abi.EI_CORR_LO]), int(ei[e, abi.EI_CORR_HI])
        if lo >= int(ei[e, abi.EI_SEED_END]):
            assert w[e] == _inorder_f64(hist[e], lo, hi, cfg.c.corr_cap, False), e
    assert ok.sum() >= n // 2
    a.close(); b.close()


def test_snapshot_restore_and_clone_carry_the_length(monkeypatch):
    """In the middle of an episode: envs 0..15 are snapshotted and restored into envs 32..47, envs 16..23 cloned into 48..55; 40 more
    steps (destinations under their sources' actions).  Every destination equals its source, which was never packed, in every output and
    every state field -- the words of the length included -- and the whole batch equals the twin's, which did the same."""
    cfg, pool = _cfg_pool("B_s1_chase")
    n = 64
    a, b = _twins(monkeypatch, n, cfg, pool)
    idx = torch.from_numpy(((np.arange(n) * 3) % pool.n).astype(np.int32))
    a.reset(idx); b.reset(idx)
    src = np.r_[0:16, 16:24]
    dst = np.r_[32:48, 48:56]

    def acts(t, paired):
        x = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=71)
        if paired:
            x[dst] = x[src]
        return _t(x)

    for t in range(90):
        a.step(acts(t, False)); b.step(acts(t, False))
    for e in (a, b):
        e.restore(e.snapshot(torch.arange(16)), torch.arange(32, 48))
        e.clone(torch.arange(16, 24), torch.arange(48, 56))
    held = 0
    for t in range(90, 130):
        a.step(acts(t, True)); b.step(acts(t, True))
        _same(a, b, cfg, ("after restore", t))
        keep = torch.ones(abi.EI_COUNT, dtype=torch.bool, device="cuda:0")
        keep[[abi.EI_EPISODES, abi.EI_ERROR_STICKY, abi.EI_STREAM]] = False        # words of the slot, not of the episode
        for name in OUTS:
            assert torch.equal(getattr(a, name)[dst], getattr(a, name)[src]), (t, name)
        for f in FIELDS:
            if f == "ep_stats":
                continue
            x = a.state_field(f)
            if f == "env_int":
                assert torch.equal(x[dst][:, keep], x[src][:, keep]), (t, f)
            else:
                assert torch.equal(x[dst], x[src]), (t, f)
        held += int(_valid(a, cfg)[0][dst].sum())
    assert held >= 0.9 * len(dst) * 40, held
    a.close(); b.close()
