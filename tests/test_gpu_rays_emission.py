"""Phase 3 of the ray kernel emits its (segment, ray) candidates in two forms (ftl_device.hpp: MASK).  A pass of at most 64 rays runs the
mask form -- per lane one 64-bit word of candidate rays over all sensors, one prefix sum and one store loop per chunk, the list worked off
in windows of FTL_PAIR_CAP pairs (FTL_DEBUG_PAIR_WINDOW=<n> makes the windows smaller) -- and a pass with more rays, the loop over two
passes, the two-stream and the EXPL kernels run the list form, one emission sequence per sensor.  Both list the same pairs, so every
output is the same bit for bit.  Every case: 256 envs x 40 steps against the oracle batch at reset and after every step, every sensor
read something other than its laser length, no error bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from golden_util import config_for, load_episode
from oracle_batch import OracleBatch, pool_scenarios
from test_gpu_configs import _actions, _compare_with_oracle, _vec

pytestmark = pytest.mark.gpu

OUTS = ("obs_num", "lasers", "target", "reward", "done", "status")
TRACKER = "LeaderPositionsTracker_v2"
N, STEPS = 256, 40


def _b_config(counts=None, order="behind"):
    """Config B's world; `counts`: lasers_count of its two LeaderCorridor_Prev_lasers_v2 sensors; `order`: both behind the tracker's key
    (one pass) or one on each side of it (two passes)."""
    _, meta = load_episode("B_s1_chase")
    kw = dict(meta["kwargs"])
    src = {k: dict(v) for k, v in kw["follower_sensors"].items()}
    rays = [k for k, v in src.items() if v["sensor_class"] == "LeaderCorridor_Prev_lasers_v2"]
    assert len(rays) == 2 and TRACKER in src and len(src) == 3
    if counts:
        for k, c in zip(rays, counts):
            src[k]["lasers_count"] = c
            src[k]["_allow_any_lasers_count"] = True      # (the reference accepts 12, 20, 24 and 36 only)
    keys = {"behind": [TRACKER, rays[0], rays[1]], "both": [rays[0], TRACKER, rays[1]]}[order]
    kw["follower_sensors"] = {k: src[k] for k in keys}
    return config_for(dict(kwargs=kw, post=None), scen_route_len=256)


def _state_bytes(env):
    return env.state[env._state_off:env._state_off + env.lib.ftl_state_bytes(env.h)]


def _same(a, b, tag):
    for name in OUTS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (tag, name)
    assert torch.equal(_state_bytes(a), _state_bytes(b)), (tag, "state")


def _near_rect(ora, scen, idx):
    """Envs of the oracle batch whose follower stands inside a rect -- a static one of its scenario, the leader's or a bear's hitbox -- or
    within 2 px of one's edge: phase 3 then lists every ray of every sensor for that edge (dmin2 < 4)."""
    cfg, R = ora.cfg, ora.cfg.n_robots
    pos = np.zeros((R, 2), np.float32); dbl = np.zeros((R, 5)); ints = np.zeros((R, 6), np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros(ora.n, bool)
    for e, o in enumerate(ora.envs):
        ora.lib.ftlo_get_robots(o.h, p(pos), p(dbl), p(ints))
        rects = np.concatenate([np.asarray(scen[int(idx[e])]["static_rects"], np.float64).reshape(-1, 4),
                                ints[[r for r in range(R) if r != 1], :4].astype(np.float64)])
        rects = rects[(rects[:, 2] > 0) & (rects[:, 3] > 0)]
        x, y = float(pos[1, 0]), float(pos[1, 1])
        dx = np.maximum(np.maximum(rects[:, 0] - x, x - (rects[:, 0] + rects[:, 2])), 0.0)
        dy = np.maximum(np.maximum(rects[:, 1] - y, y - (rects[:, 1] + rects[:, 3])), 0.0)
        out[e] = bool((dx * dx + dy * dy < 4.0).any())      # 0 inside a rect, else the distance to its nearest edge
    return out


def _ram(ora, a, scen, idx):
    """Actions `a` with every second env driving at full speed into the nearest static rect, steered from the oracle's own state (random
    actions keep the followers clear of every rect for 40 steps of 2.5 px)."""
    cfg, R = ora.cfg, ora.cfg.n_robots
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    pos = np.zeros((R, 2), np.float32); dbl = np.zeros((R, 5)); ints = np.zeros((R, 6), np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    for e in range(0, ora.n, 2):
        ora.lib.ftlo_get_robots(ora.envs[e].h, p(pos), p(dbl), p(ints))
        r = np.asarray(scen[int(idx[e])]["static_rects"], np.float64).reshape(-1, 4)
        r = r[(r[:, 2] > 0) & (r[:, 3] > 0)]
        cx, cy = r[:, 0] + 0.5 * r[:, 2] - float(pos[1, 0]), r[:, 1] + 0.5 * r[:, 3] - float(pos[1, 1])
        k = int(np.argmin(cx * cx + cy * cy))
        err = (np.degrees(np.arctan2(cy[k], cx[k])) % 360.0 - dbl[1, 0] + 540.0) % 360.0 - 180.0
        a[e] = (ms, float(np.clip(0.3 * err, -mr, mr)))
    return a


def _run(monkeypatch, cfg, env_vars, twin_vars=None, tag="", seed=41, oracle_kw=None, near=False):
    """`cfg` under `env_vars` against the oracle, and -- with `twin_vars` -- against the same run under those switches, bit for bit.
    `near`: every second env drives into the nearest static rect (_ram); returns the number of env-steps with a rect next to the follower or around it."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    for k in ("FTL_RAYS_ONE_PASS", "FTL_DEBUG_PAIR_WINDOW", "FTL_DEBUG_CORR_LDS_CAP"):
        monkeypatch.delenv(k, raising=False)
    pool = ScenarioPool.generate(cfg, np.arange(128), "cuda:0")

    def make(vars_):
        for k, v in vars_.items():
            monkeypatch.setenv(k, v)
        e = _vec(N, cfg, pool)
        for k in vars_:
            monkeypatch.delenv(k)
        return e
    env = make(env_vars)
    twin = make(twin_vars) if twin_vars is not None else None
    scen = pool_scenarios(pool)
    idx = (np.arange(N) * 3) % pool.n
    ora = OracleBatch(cfg, N, **(oracle_kw or {}))
    ora.reset(scen, idx)
    for e in (env, twin):
        if e is not None:
            e.reset(torch.from_numpy(idx.astype(np.int32)))
    _compare_with_oracle(env, ora, cfg, (tag, "reset"))
    if twin is not None:
        _same(env, twin, (tag, "reset"))
    n_near = 0
    for t in range(STEPS):
        a = _actions(cfg, N, t, "mixed" if t % 2 else "random", seed=seed)
        if near:
            a = _ram(ora, a, scen, idx)
        act = torch.tensor(a, dtype=torch.float64, device="cuda:0")
        env.step(act)
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, (tag, t))
        if twin is not None:
            twin.step(act)
            _same(env, twin, (tag, t))
        if near:
            n_near += int(_near_rect(ora, scen, idx).sum())
    las = env.lasers.cpu().numpy()
    for l in cfg.lasers:      # every sensor saw something: a block that still reads its laser length everywhere would compare equal for nothing
        blk = las[:, l.out_offset:l.out_offset + l.history * l.width]
        assert (blk != np.float32(l.length)).any(), l.name
    for e in (env, twin):
        if e is not None:
            assert e.error_report() == (0, 0)
            e.close()
    return n_near


def _form(capfd, monkeypatch, cfg):
    """The emission form ftl_create reports for one-stream launches of `cfg` ("mask" / "list")."""
    from continiousenvironment_follower_leader_amd import _lib
    import re
    lib = _lib.load()
    monkeypatch.setenv("FTL_DEBUG_PRINT_LDS", "1")
    capfd.readouterr()
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), 64, 0, C.byref(h)) == 0, lib.ftl_last_error().decode()
    err = capfd.readouterr().err
    lib.ftl_destroy(h)
    monkeypatch.delenv("FTL_DEBUG_PRINT_LDS")
    m = re.search(r"ray candidates: (mask|list) form on one stream, (mask|list) form on two, window (\d+)\n", err)
    assert m, err
    return m.group(1)


def test_mask_form_equals_the_list_form_on_config_B(monkeypatch):
    """36 rays in one pass: the mask form, against the same run in the loop form (FTL_RAYS_ONE_PASS=0), which emits per sensor."""
    _run(monkeypatch, _b_config(), {}, {"FTL_RAYS_ONE_PASS": "0"}, tag="B mask vs list")


def test_windows_of_16_pairs_equal_the_default_window(monkeypatch):
    """FTL_DEBUG_PAIR_WINDOW=16: every chunk with more than 16 pairs takes several windows, and lanes whose pairs straddle a window edge
    write them in two parts."""
    _run(monkeypatch, _b_config(), {"FTL_DEBUG_PAIR_WINDOW": "16"}, {}, tag="B window 16")


def test_64_rays_fill_the_mask(monkeypatch, capfd):
    """40 + 24 rays: bit 63 of the mask in use, and at 9 / 15 degrees per ray ~45 segments make more than FTL_PAIR_CAP pairs in a chunk
    (several windows without the switch).  The oracle's world must show an env-step with a rect next to the follower (or around it), so
    that the "every ray" rule -- 64 pairs from one lane -- was exercised."""
    cfg = _b_config((40, 24))
    assert _form(capfd, monkeypatch, cfg) == "mask" and _form(capfd, monkeypatch, _b_config()) == "mask"
    n_near = _run(monkeypatch, cfg, {}, tag="40 + 24 rays", near=True)
    assert n_near >= 1, "no env-step with a rect within 2 px of the follower: pick other seeds or actions"


def test_65_rays_take_the_list_form(monkeypatch, capfd):
    """41 + 24 rays: the list form just past the boundary."""
    cfg = _b_config((41, 24))
    assert _form(capfd, monkeypatch, cfg) == "list"
    _run(monkeypatch, cfg, {}, tag="41 + 24 rays")


def test_unstaged_corridor_leaves_empty_masks_between_live_ones(monkeypatch):
    """Config E (CAPPED) with an 8-point LDS copy of the corridor: phase 3 lists every segment of the span, and those outside all windows
    (sm == 0) are lanes with an empty mask inside a run of live ones."""
    _, meta = load_episode("E_s3_chase")
    cfg = config_for(meta, scen_route_len=256, rng_seed=9, env_id_base=7000)
    assert cfg.c.corr_cap > 128 and sum(l.count for l in cfg.lasers) <= 64
    _run(monkeypatch, cfg, {"FTL_DEBUG_CORR_LDS_CAP": "8"}, {"FTL_DEBUG_CORR_LDS_CAP": "8", "FTL_RAYS_ONE_PASS": "0"}, tag="E unstaged",
         seed=33, oracle_kw=dict(env_id_base=7000))


def test_one_sensor_on_each_side_of_the_tracker(monkeypatch, capfd):
    """Two passes (the loop form, which emits per sensor): each pass lists its rays in its own index space (pass_base)."""
    cfg = _b_config(order="both")
    assert [int(cfg.c.lasers[k].after_tracker) for k in range(cfg.c.n_lasers)] == [0, 1]
    assert _form(capfd, monkeypatch, cfg) == "list"
    _run(monkeypatch, cfg, {}, tag="two passes")
