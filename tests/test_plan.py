"""The host launch plan of a handle -- lanes per env, LDS layout, cost sort, which instantiation of the frame and ray kernels it launches --
as ftl_create and ftl_tune report it under FTL_DEBUG_PRINT_LDS ("The launch plan").  Pure host work except the last test.
The expected template arguments are written out here from the two decision tables; nothing below asks the library what it should say."""
import ctypes as C
import json
import re

import numpy as np
import pytest

from continiousenvironment_follower_leader_amd import abi, make_config
from fuzz_configs import TRACKER
from golden_util import GOLDEN, config_for

SWITCHES = ("FTL_SPLIT", "FTL_NO_REGROUP", "FTL_REGROUP_EVERY", "FTL_DEBUG_G8", "FTL_RAYS_ONE_PASS", "FTL_DEBUG_CORR_LDS_CAP", "FTL_DEFER",
            "FTL_DEBUG_LDS_PAD", "FTL_DEBUG_LDS_PAD_RAYS")
RAYS = r"(rays<\d+,[01],[01],[01],[01]>|no rays)"
REPORT = re.compile(r"ftl: frame kernel LDS (\d+) B per wavefront, (\d+) lanes per env, \d+ frames at most, searches (?:deferred|in frame)\n"
                    r"ftl: ray kernel LDS (\d+) B per env\n"
                    r"ftl: kernels frames<(\d),([01])>, " + RAYS + " on one stream, " + RAYS + r" on two; regroup (on|off) every (\d+), "
                    r"two streams (on|off)\n")
TOO_MUCH_LDS = "the frame kernel needs more than 64 KiB of LDS per wavefront (static rects x frames per step)"


@pytest.fixture(scope="module")
def lib():
    from continiousenvironment_follower_leader_amd import _lib
    _lib.build()
    return _lib.load()


@pytest.fixture
def env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("FTL_DEBUG_PRINT_LDS", "1")
    return monkeypatch


def _parse(text):
    """The one report in `text`: dict of what its three lines say (rays as tuples of the five template arguments, or None)."""
    found = REPORT.findall(text)
    assert len(found) == 1 and text.count("ftl:") == 3, text
    fr_lds, lanes, rays_lds, g, reg, one, two, regroup, every, split = found[0]
    assert lanes == g, text

    def args(s):
        return None if s == "no rays" else tuple(int(v) for v in s[5:-1].split(","))
    return dict(fr_lds=int(fr_lds), rays_lds=int(rays_lds), frames=(int(g), int(reg)), one=args(one), two=args(two),
                regroup=regroup == "on", every=int(every), split=split == "on", text=text)


def _create(lib, capfd, cfg, n):
    capfd.readouterr()
    h = C.c_void_p()
    rc = lib.ftl_create(C.byref(cfg.c), n, 0, C.byref(h))
    assert rc == 0, lib.ftl_last_error().decode()
    return h, _parse(capfd.readouterr().err)


def _plan(lib, capfd, cfg, n=64):
    h, rep = _create(lib, capfd, cfg, n)
    lib.ftl_destroy(h)
    return rep


def _tune(lib, capfd, h, key, value):
    """(return code, message, parsed report or None when nothing was printed)"""
    capfd.readouterr()
    rc = lib.ftl_tune(h, key, value)
    err = capfd.readouterr().err
    return rc, ("" if rc == 0 else lib.ftl_last_error().decode()), (_parse(err) if err else None)


def _prev(history, **kw):
    return dict(sensor_class="LeaderCorridor_Prev_lasers_v2", lasers_count=12, laser_length=100, max_prev_obs=history, pad_sectors=False,
                react_to_obstacles=True, **kw)


FRONT = dict(sensor_class="LeaderCorridor_lasers", react_to_obstacles=True)


def _config(history, front=False, both_sides=False, **kw):
    """Tracker first, so the ray sensors are scanned after it; both_sides puts one more ray sensor before it."""
    sensors = {}
    if both_sides:
        sensors["early"] = _prev(history)
    sensors["LeaderPositionsTracker_v2"] = dict(TRACKER)
    sensors["rays"] = _prev(history)
    if front:
        sensors["front"] = dict(FRONT)
    return make_config(follower_sensors=sensors, **dict(dict(bear_number=1), **kw))


# max_prev_obs -> <HM, EXPL, SPLIT, CAPPED, ONE_PASS> of the one-stream and of the two-stream launch, CAPPED left open
COMMON = {5: ((5, 0, 0, 1), (5, 1, 1, 0)), 8: ((8, 0, 0, 1), (10, 0, 1, 0)), 10: ((10, 0, 0, 1), (10, 0, 1, 0)), 12: ((12, 0, 0, 1), (12, 1, 1, 0)),
          # between the listed sizes: the least of 5, 8, 10, 12 that holds the history
          3: ((5, 0, 0, 1), (5, 1, 1, 0)), 6: ((8, 0, 0, 1), (10, 0, 1, 0)), 9: ((10, 0, 0, 1), (10, 0, 1, 0)), 11: ((12, 0, 0, 1), (12, 1, 1, 0))}
EXPL = {5: ((5, 1, 0, 0), (5, 1, 1, 0)), 8: ((12, 1, 0, 0), (12, 1, 1, 0)), 10: ((12, 1, 0, 0), (12, 1, 1, 0)), 12: ((12, 1, 0, 0), (12, 1, 1, 0))}


def _with_capped(row, capped):
    return row[:3] + (capped,) + row[3:]


@pytest.mark.parametrize("capped", [0, 1])
def test_every_row_of_the_ray_table_is_reached(lib, env, capfd, capped):
    """One stream and two streams, with and without a LeaderCorridor_lasers sensor (EXPL), ring staged whole or capped (corr_cap=512 against
    the 128 points of the LDS copy), ONE_PASS on (every ray sensor behind the tracker) and off (sensors on both sides; FTL_RAYS_ONE_PASS=0)."""
    kw = dict(corr_cap=512) if capped else {}
    for table, front in ((COMMON, False), (EXPL, True)):
        for history, (one, two) in table.items():
            rep = _plan(lib, capfd, _config(history, front=front, **kw))
            assert (rep["one"], rep["two"]) == (_with_capped(one, capped), _with_capped(two, capped)), (history, front, rep["text"])
            assert not rep["split"]
    for history in (5, 8, 10, 12):
        one, two = COMMON[history]
        loop_form = _with_capped(one[:3] + (0,), capped)
        rep = _plan(lib, capfd, _config(history, both_sides=True, **kw))
        assert (rep["one"], rep["two"]) == (loop_form, _with_capped(two, capped)), (history, rep["text"])
        env.setenv("FTL_RAYS_ONE_PASS", "0")
        rep = _plan(lib, capfd, _config(history, **kw))
        assert (rep["one"], rep["two"]) == (loop_form, _with_capped(two, capped)), (history, rep["text"])
        env.delenv("FTL_RAYS_ONE_PASS")
    # the two-stream rows on a handle that runs two streams
    env.setenv("FTL_SPLIT", "1")
    for table, front in ((COMMON, False), (EXPL, True)):
        for history in (5, 8, 10, 12):
            rep = _plan(lib, capfd, _config(history, front=front, **kw), n=8192)
            assert rep["split"] and rep["two"] == _with_capped(table[history][1], capped), (history, front, rep["text"])
            assert not _plan(lib, capfd, _config(history, front=front, **kw), n=8191)["split"]          # below 8,192 envs the switch does nothing


def test_ray_lds_holds_5_or_12_minima_per_ray(lib, env, capfd):
    """The float32 minima of the ray kernel's LDS are sized for the widest instantiation of the history: 5 accumulators up to
    max_prev_obs=5, FTL_HMAX=12 beyond, whichever instantiation runs."""
    def extra(history):           # bytes that grow with the history at 12 rays, 1 bear: 2 rects of 28 B and 2 green caps of 20 B per snapshot
        return 2 * 28 * history + 2 * 20 * history
    base = _plan(lib, capfd, _config(5))["rays_lds"] - extra(5)
    for history in (3, 5, 6, 8, 10, 12):
        assert _plan(lib, capfd, _config(history))["rays_lds"] - extra(history) - base == 12 * 4 * ((5 if history <= 5 else 12) - 5), history


def test_frame_table_lanes_and_regimes(lib, env, capfd):
    """G: 8 lanes up to 256 CUs x 4 SIMDs x 8 envs = 8,192 co-scheduled envs and 4 beyond, always 8 with more than 2 dynamic obstacles,
    FTL_DEBUG_G8 overrides; REG: leader regimes or random frame counts."""
    one_bear = _config(5)
    assert _plan(lib, capfd, one_bear, 8192)["frames"] == (8, 0)
    assert _plan(lib, capfd, one_bear, 8193)["frames"] == (4, 0)
    for n in (64, 8193, 65536):
        assert _plan(lib, capfd, _config(5, bear_number=3), n)["frames"] == (8, 0), n
    with pytest.warns(UserWarning):
        rand = _config(5, random_frames_per_step=[3, 9])
    assert _plan(lib, capfd, rand, 8192)["frames"] == (8, 1) and _plan(lib, capfd, rand, 8193)["frames"] == (4, 1)
    assert _plan(lib, capfd, _config(5, leader_speed_regime={0: [0.2, 1], 60: 0.5}))["frames"] == (8, 1)
    assert _plan(lib, capfd, _config(5, leader_acceleration_regime={0: 0, 40: 0.002}))["frames"] == (8, 1)
    env.setenv("FTL_DEBUG_G8", "0")
    assert _plan(lib, capfd, one_bear, 64)["frames"] == (4, 0) and _plan(lib, capfd, _config(5, bear_number=3), 64)["frames"] == (8, 0)
    env.setenv("FTL_DEBUG_G8", "1")
    assert _plan(lib, capfd, one_bear, 65536)["frames"] == (8, 0)


def test_report_states_the_cost_sort_and_the_streams(lib, env, capfd):
    """regroup: on beyond one round of frame-kernel wavefronts or with random frame counts, FTL_NO_REGROUP=0/1 overrides; the interval is 4
    unless FTL_REGROUP_EVERY says otherwise; two streams: from 8,192 envs on with random frame counts, FTL_SPLIT overrides."""
    cfg = _config(5)
    with pytest.warns(UserWarning):
        rand = _config(5, random_frames_per_step=[3, 9])
    rep = _plan(lib, capfd, cfg)
    assert (rep["regroup"], rep["every"], rep["split"]) == (False, 4, False)
    assert _plan(lib, capfd, cfg, 65536)["regroup"] and _plan(lib, capfd, rand)["regroup"]
    assert _plan(lib, capfd, rand, 8192)["split"] and not _plan(lib, capfd, rand, 8191)["split"] and not _plan(lib, capfd, cfg, 8192)["split"]
    env.setenv("FTL_NO_REGROUP", "0")
    assert _plan(lib, capfd, cfg)["regroup"]
    env.setenv("FTL_NO_REGROUP", "1")
    assert not _plan(lib, capfd, cfg, 65536)["regroup"]
    env.setenv("FTL_REGROUP_EVERY", "2")
    assert _plan(lib, capfd, cfg)["every"] == 2
    env.setenv("FTL_SPLIT", "0")
    assert not _plan(lib, capfd, rand, 8192)["split"]
    assert _plan(lib, capfd, make_config(bear_number=1), 64)["one"] is None          # no ray sensors: nothing to launch


def test_tune_replans_and_reports(lib, env, capfd):
    """ftl_tune(FTL_TUNE_COSCHEDULED_ENVS) runs the same schedule function as ftl_create: 4 lanes beyond 8,192 co-scheduled envs, and back."""
    h, created = _create(lib, capfd, make_config(n_static=12, bear_number=2), 64)
    assert created["frames"] == (8, 0)
    rc, why, rep = _tune(lib, capfd, h, abi.FTL_TUNE_COSCHEDULED_ENVS, 8193)
    assert rc == 0 and rep["frames"] == (4, 0) and rep["fr_lds"] > created["fr_lds"], why        # 16 envs per wavefront
    rc, why, rep = _tune(lib, capfd, h, abi.FTL_TUNE_COSCHEDULED_ENVS, 64)
    assert rc == 0 and rep["text"] == created["text"], why
    rc, why, rep = _tune(lib, capfd, h, abi.FTL_TUNE_REGROUP_EVERY, 7)
    assert rc == 0 and rep["every"] == 7 and rep["fr_lds"] == created["fr_lds"]
    rc, why, rep = _tune(lib, capfd, h, abi.FTL_TUNE_COSCHEDULED_ENVS, 63)
    assert rc == abi.FTL_E_INVALID and rep is None and "below this handle's own" in why
    lib.ftl_destroy(h)


def test_a_refused_tune_changes_nothing(lib, env, capfd):
    """300 static rects fit the frame kernel's LDS with 8 envs per wavefront (8 lanes) and not with 16 (4 lanes): the tune to 8,193
    co-scheduled envs is refused, and the handle keeps the plan it was created with."""
    h, created = _create(lib, capfd, make_config(n_static=300, bear_number=2), 64)
    assert created["frames"] == (8, 0) and created["fr_lds"] == 39920
    rc, why, rep = _tune(lib, capfd, h, abi.FTL_TUNE_COSCHEDULED_ENVS, 8193)
    assert rc == abi.FTL_E_INVALID and why == TOO_MUCH_LDS and rep is None
    rc, why, rep = _tune(lib, capfd, h, abi.FTL_TUNE_REGROUP_EVERY, 4)
    assert rc == 0 and rep["text"] == created["text"], why
    lib.ftl_destroy(h)
    # (create itself keeps its rule: at 8,193 envs it plans 4 lanes and refuses)
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(make_config(n_static=300, bear_number=2).c), 8193, 0, C.byref(h)) == abi.FTL_E_INVALID
    assert lib.ftl_last_error().decode() == TOO_MUCH_LDS


@pytest.mark.gpu
def test_a_refused_tune_leaves_the_batch_stepping_like_its_twin(monkeypatch):
    """Two batches of 64 envs on a world of 300 static rects (pool B's worlds, their rects repeated; the second bear the config asks for is
    pool B's bear once more -- a synthetic world: the untuned twin is the reference, not the recorded episodes).  One is refused a tune to
    8,193 co-scheduled envs; both then reset and take 8 steps on the same actions and agree bit for bit in every output and state field."""
    import torch
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool, VecGame
    monkeypatch.delenv("FTL_DEBUG_G8", raising=False)
    z = np.load(GOLDEN + "/pool_B.npz")
    kw = dict(json.loads(str(z["meta"]))["kwargs"], n_static=300, bear_number=2)
    cfg = config_for(dict(kwargs=kw, post=None), scen_route_len=int(z["route_len"].max()))
    k, n = 64, 64
    rects = np.tile(z["static_rects"][:k], (1, 9, 1))[:, :300].astype(np.int32)
    again = [0, 1, 2, 2]                                       # follower, leader, bear, the bear once more
    pool = ScenarioPool(cfg, rects, z["robot_pos"][:k][:, again], z["robot_dir"][:k][:, again], z["robot_rect"][:k][:, again].astype(np.int32),
                        [z["route"][i, :z["route_len"][i]].astype(np.float64) for i in range(k)],
                        [z["init_traj"][i, :z["init_traj_len"][i]] for i in range(k)], "cuda:0")
    games = [VecGame(n, device="cuda:0", config=cfg) for _ in range(2)]
    for g in games:
        g.load_scenarios(pool)
    with pytest.raises(ValueError, match="64 KiB of LDS per wavefront"):
        games[1].tune(coscheduled_envs=8193)
    gen = torch.Generator(device="cpu").manual_seed(5)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    for g in games:
        g.reset()
    for t in range(8):
        a = torch.stack([(0.5 + 0.5 * torch.rand(n, generator=gen, dtype=torch.float64)) * ms,
                         torch.clamp(torch.randn(n, generator=gen, dtype=torch.float64) * 0.2 * mr, -mr, mr)], 1).contiguous().cuda()
        for g in games:
            g.step(a, auto_reset=True)
        torch.cuda.synchronize()
        for name in ("obs_num", "lasers", "reward", "done", "status"):
            assert torch.equal(getattr(games[0], name), getattr(games[1], name)), (t, name)
    assert not games[0].done.all()
    for name in ("rb_pos", "rb_dbl", "rb_int", "env_int", "env_dbl", "traj", "hist", "corr", "snap_rects", "snap_win", "traj_bb", "ep_stats",
                 "hist1", "fol_cs", "corr32"):
        assert torch.equal(games[0].state_field(name), games[1].state_field(name)), name
    for g in games:
        g.close()
