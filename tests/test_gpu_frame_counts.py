"""The frame kernel at the edges of the frame count.  ftl_create picks one of two schedules for the position searches of a step: with a
fixed count of 2..16 frames the searches of frames 1.. wait in LDS for the end of the step (a pending buffer of f_max - 1 items per env),
otherwise every frame resolves its own (one item per env) -- one frame per step, 17 frames and more, and every random_frames_per_step
config.  The shipped configs sit in the middle of the first range (5 and 10 frames) or draw 30..69; here: 1, 2 (frame 0 and the last frame
are neighbours), 16 (the largest pending buffer, four whole words of frame records), 17 (the first undeferred count, a record word read
partly filled), 40; three and six robots and leader regimes on the undeferred schedule; random counts that start at one frame; FTL_DEFER=0
against the default; and one frame per step until the corridor ring holds more points than the ray kernel's LDS copy.

Reference: the oracle batch (tests/oracle_batch.py), every output and the hitboxes at reset and after every step, the tolerances of
test_gpu_configs._compare_with_oracle (whose corner-graze waivers go to the session's shared budget; nothing is waived here)."""
import warnings

import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from oracle_batch import OracleBatch, pool_scenarios
from test_gpu_configs import _actions, _cfg_pool, _compare_with_oracle, _vec

pytestmark = pytest.mark.gpu

OUTS = ("obs_num", "lasers", "target", "reward", "done", "status")


@pytest.fixture(params=["4 lanes per env", "8 lanes per env"])
def lanes_per_env(request, monkeypatch):
    """Both forms of the frame kernel (FTL_DEBUG_G8 at ftl_create, as tests/test_gpu_queue.py): at these batch sizes the library would
    always pick 8 lanes."""
    monkeypatch.setenv("FTL_DEBUG_G8", "0" if request.param.startswith("4") else "1")
    return request.param


def _t(a, dtype=torch.float64):
    return torch.tensor(a, dtype=dtype, device="cuda:0")


def _every_ray_sensor_saw_something(env, cfg):
    """A block that still reads its laser length everywhere would compare equal for nothing (tests/test_gpu_rays_one_pass.py)."""
    las = env.lasers.cpu().numpy()
    for l in cfg.lasers:
        blk = las[:, l.out_offset:l.out_offset + l.history * l.width]
        assert (blk != np.float32(l.length)).any(), l.name


def _run_against_oracle(cfg, pool, n, steps, tag, seed, env_id_base=None, negative_speed=False):
    """reset + `steps` steps of `n` envs, actions alternating "mixed" and "random", everything against the oracle after every call."""
    env = _vec(n, cfg, pool)
    scen = pool_scenarios(pool)
    idx = (np.arange(n) * 3) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n, env_id_base=env_id_base)
    ora.reset(scen, idx)
    _compare_with_oracle(env, ora, cfg, (tag, "reset"))
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=seed)
        if negative_speed:
            a[3::7, 0] = -0.5 * cfg.c.follower.max_speed
        env.step(_t(a))
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, (tag, t))
    _every_ray_sensor_saw_something(env, cfg)
    assert env.error_report() == (0, 0), tag
    assert not ora.counters()[2].any(), (tag, "oracle error flag")
    env.close()


# ---- a. the oracle batch at every edge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [1, 2, 16, 17, 40])
def test_frame_count_edges_match_oracle_batch(frames, lanes_per_env):
    """Config B at 1, 2, 16, 17 and 40 frames per step, both lane counts, 203 envs (a multiple of neither 8 nor 16: the last wavefront is
    partly idle in both layouts) on 128 generated scenarios; 120 steps at 1 and 2 frames so that the tracker saves enough points."""
    cfg, pool = _cfg_pool("B_s1_chase", 128, frames_per_step=frames)
    assert cfg.c.frames_per_step == frames and cfg.c.rand_fps_hi == 0 and cfg.c.n_bears == 1
    _run_against_oracle(cfg, pool, 203, 120 if frames <= 2 else 40, ("edges", frames, lanes_per_env), seed=41)


# ---- b. more robots, regimes and random counts on the undeferred schedule -------------------------------------------------------------------
@pytest.mark.parametrize("ep,base", [("B3_s8_chase", None), ("B6_s2_chase", 2000)])
def test_more_robots_at_17_frames_match_oracle_batch(ep, base):
    """Three bears (five robots: 8 lanes per env are forced) and six (bear 5 draws its way-points from the per-env stream every frame: the
    oracle batch gets the same stream ids, so nothing has to be left out of the comparison) at 17 frames per step."""
    over = {} if base is None else dict(rng_seed=3, env_id_base=base)
    cfg, pool = _cfg_pool(ep, 128, frames_per_step=17, **over)
    assert cfg.c.frames_per_step == 17 and cfg.c.n_bears == (3 if base is None else 6)
    _run_against_oracle(cfg, pool, 203, 40, (ep, 17), seed=43, env_id_base=base)


@pytest.mark.parametrize("frames", [1, 17])
def test_regimes_at_1_and_17_frames_match_oracle_batch(frames, lanes_per_env):
    """Config E (leader regimes: the REG instantiations with a fixed count, which the shipped configs only reach at 5 frames) with per-env
    regime streams; 60 steps at one frame per step.  E's tracker ring is sized by the flat rule for regimes, not from the frame count."""
    cfg, pool = _cfg_pool("E_s3_chase", 128, rng_seed=9, env_id_base=11000, frames_per_step=frames)
    assert cfg.c.n_speed_regime > 0 and cfg.c.frames_per_step == frames and cfg.c.n_bears == 2
    _run_against_oracle(cfg, pool, 203, 60 if frames == 1 else 40, ("E", frames, lanes_per_env), seed=45, env_id_base=11000, negative_speed=True)


@pytest.mark.parametrize("bounds", [[1, 2], [1, 3]])
def test_random_counts_from_one_frame_match_oracle_batch(bounds, lanes_per_env):
    """random_frames_per_step [1, 2] (one frame every step: f_max == 1 in the REG kernel) and [1, 3] (one or two) on config B, the draws from
    the per-env stream on both sides."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")    # ENV:399-401: both frame settings are given
        cfg, pool = _cfg_pool("B_s1_chase", 128, random_frames_per_step=bounds, rng_seed=5, env_id_base=700)
    assert (cfg.c.rand_fps_lo, cfg.c.rand_fps_hi) == tuple(bounds)
    _run_against_oracle(cfg, pool, 203, 120, ("random", tuple(bounds), lanes_per_env), seed=47, env_id_base=700)


# ---- c. FTL_DEFER=0 changes nothing ----------------------------------------------------------------------------------------------------------
# What the position searches leave behind besides their result bits (ftl_frames_group.hpp: the outputs of g_resolve, stored by g_store):
# the cached trajectory point and the two distance bounds.  A step that defers its later frames' searches refreshes them after frame 0 only,
# one that does not after every frame that searched -- either set is valid (they only decide which points a later search looks at), so
# they may differ.  Nothing else in env_int depends on the schedule, and nothing in env_dbl (g_load_late and the tail read no cache).
SEARCH_CACHE_EI = (abi.EI_HINT, abi.EI_HINT_X, abi.EI_HINT_Y, abi.EI_CLR_GREEN, abi.EI_CLR_ALL)
STATE_FIELDS = ("rb_pos", "rb_dbl", "rb_int", "traj", "hist", "corr", "traj_bb", "ep_stats")


@pytest.mark.parametrize("ep,frames", [("B_s1_chase", 2), ("B_s1_chase", 3), ("B_s1_chase", 10), ("B_s1_chase", 16), ("E_s3_chase", 5)])
def test_defer_switch_never_changes_a_result(monkeypatch, ep, frames):
    """One handle created under FTL_DEFER=0 (every frame resolves its own searches) and one without it (frames 1.. wait for the end of the
    step): 256 envs, 40 steps or more with auto-reset and a masked reset after the 20th, outputs bit-identical after every call, the
    state every eighth step; the default side also agrees with the oracle at the end."""
    n = 256
    regimes = ep.startswith("E")
    over = dict(rng_seed=9, env_id_base=13000) if regimes else {}
    cfg, pool = _cfg_pool(ep, 128, frames_per_step=frames, **over)
    assert cfg.c.frames_per_step == frames and cfg.c.rand_fps_hi == 0
    # 40 steps, or as many as a follower at full speed needs for 100 px: it starts ON the leader's trajectory, and a frame after the first
    # needs a search of its own only where the follower crosses leader_pos_epsilon (25 px) or max_dev (50 px) off it inside a step -- in 40
    # steps of 2 or 3 frames it cannot get that far, and both handles would run the same searches
    steps = max(40, int(np.ceil(100.0 / (frames * cfg.c.follower.max_speed))))
    monkeypatch.delenv("FTL_DEFER", raising=False)
    a = _vec(n, cfg, pool)                 # the default: deferred
    monkeypatch.setenv("FTL_DEFER", "0")
    b = _vec(n, cfg, pool)
    monkeypatch.delenv("FTL_DEFER")
    keep = np.ones(abi.EI_COUNT, bool)
    keep[list(SEARCH_CACHE_EI)] = False
    keep = torch.from_numpy(keep).to("cuda:0")

    seen = {"caches differ": 0}      # calls after which some env's search caches differed

    def same(tag, state):
        for name in OUTS:
            assert torch.equal(getattr(a, name), getattr(b, name)), (ep, frames, tag, name)
        seen["caches differ"] += int(not torch.equal(a.state_field("env_int")[:, ~keep], b.state_field("env_int")[:, ~keep]))
        if state:
            for f in STATE_FIELDS:
                assert torch.equal(a.state_field(f), b.state_field(f)), (ep, frames, tag, f)
            assert torch.equal(a.state_field("env_int")[:, keep], b.state_field("env_int")[:, keep]), (ep, frames, tag, "env_int")
            assert torch.equal(a.state_field("env_dbl"), b.state_field("env_dbl")), (ep, frames, tag, "env_dbl")

    scen = pool_scenarios(pool)
    idx = (np.arange(n) * 3) % pool.n
    ora = OracleBatch(cfg, n, env_id_base=13000 if regimes else None)
    ora.reset(scen, idx)
    for e in (a, b):
        e.reset(torch.from_numpy(idx.astype(np.int32)))
    same("reset", True)
    clean = np.ones(n, bool)               # envs that no auto-reset has restarted: the oracle batch has none, it replays their episodes
    for t in range(steps):
        act = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=49)
        for e in (a, b):
            e.step(_t(act), auto_reset=True)
        same(t, t % 8 == 7)
        ora.step(act)
        clean &= ~ora.done.astype(bool)
        if t == 19:
            mask = np.arange(n) % 5 == 0
            idx = np.where(mask, (idx + 7) % pool.n, idx)
            for e in (a, b):
                e.reset(torch.from_numpy(idx.astype(np.int32)), mask=torch.from_numpy(mask.astype(np.uint8)))
            same("masked reset", True)
            ora.reset(scen, idx, mask=mask)
    # the default side against the oracle at the last step, on the envs whose episodes both sides played alike (an auto-reset draws the next
    # scenario from the pool window and advances the env's reset count); test_frame_count_edges_match_oracle_batch covers the rest
    assert clean.sum() > n // 2
    _compare_rows_with_oracle(a, ora, cfg, clean, (ep, frames, "oracle"))
    assert a.error_report() == (0, 0) and b.error_report() == (0, 0)
    # the two handles did run different schedules: a search of a frame after the first refreshes the caches on one side only
    print("search caches differed after %d of %d calls" % (seen["caches differ"], steps + 2))
    assert seen["caches differ"], (ep, frames, "FTL_DEFER=0 left no trace in the search caches: the same schedule ran twice")
    a.close(); b.close()


def _compare_rows_with_oracle(env, ora, cfg, rows, tag):
    """_compare_with_oracle on the envs `rows`: the same checks through a view of both sides that holds those envs only."""
    class Rows:
        pass
    e, o = Rows(), Rows()
    sel = torch.from_numpy(np.flatnonzero(rows)).to("cuda:0")
    e.n = int(rows.sum())
    for name in OUTS:
        setattr(e, name, getattr(env, name)[sel])
        setattr(o, name, getattr(ora, name)[rows])
    e.state_field = lambda f: env.state_field(f)[sel]
    e.pool = env.pool
    o.robot_ints = lambda: ora.robot_ints()[rows]
    _compare_with_oracle(e, o, cfg, tag)


# ---- d. one frame per step to the corridor's steady state ----------------------------------------------------------------------------------
def test_one_frame_per_step_to_the_corridor_steady_state():
    """Config B at one frame per step saves a tracker point about every pixel of the leader's way: the corridor, trimmed to 250 px, grows to
    some 250 points (263 on the device and in the oracle) -- the ring make_config sizes for it holds 512 ("Ring capacity at the frame-count edges", quotes the count
    measured here), and the window is then really longer than the 128 points the ray kernel stages in LDS, the unstaged path that only
    FTL_DEBUG_CORR_LDS_CAP=8 forced so far.  64 envs, 1,300 steps, finished envs re-reset by mask on both sides; against the oracle at
    every step of the first 100 and at every tenth after that."""
    n, steps = 64, 1300
    cfg, pool = _cfg_pool("B_s1_chase", 128, frames_per_step=1)
    assert cfg.c.corr_cap == abi.FTL_MAX_CORR_CAP
    env = _vec(n, cfg, pool)
    scen = pool_scenarios(pool)
    idx = (np.arange(n) * 3) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n)
    ora.reset(scen, idx)
    _compare_with_oracle(env, ora, cfg, ("soak", "reset"))
    longest = 0
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=51)
        env.step(_t(a))
        ora.step(a)
        if t < 100 or t % 10 == 9:
            _compare_with_oracle(env, ora, cfg, ("soak", t))
            ei = env.state_field("env_int").cpu().numpy()
            longest = max(longest, int((ei[:, abi.EI_CORR_HI] - ei[:, abi.EI_CORR_LO]).max()))
            d = ora.done.astype(bool)
            if d.any() and t % 10 == 9:            # masked reset of the finished envs to their next scenario on both sides
                idx = np.where(d, (idx + n) % pool.n, idx)
                env.reset(torch.from_numpy(idx.astype(np.int32)), mask=torch.from_numpy(d.astype(np.uint8)))
                ora.reset(scen, idx, mask=d)
                _compare_with_oracle(env, ora, cfg, ("soak", t, "masked reset"))
    print("longest corridor: %d points of %d" % (longest, cfg.c.corr_cap))
    assert env.error_report() == (0, 0)
    assert not ora.counters()[2].any()
    assert longest > 128, longest
    env.close()
