"""GPU tests of ftl_render / VecGame.render / Game.render against the independent numpy rasteriser of the spec (tests/render_numpy.py).

Acceptance rule of an image (include/ftl.h, coverage rules): a pixel may differ only where its centre lies within 1e-3 output pixels of
a primitive boundary in the numpy float64 geometry, and at most 0.05 % of the pixels may differ.  Exact ties (a pixel centre exactly on
a boundary) are not in the band: both sides follow the same <= / < rules."""
import json

import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import GOLDEN, config_for, load_episode, scenario_arrays
from render_numpy import compare, env_scene, render_scene

pytestmark = pytest.mark.gpu

EPISODES = {"B": "B_s1_chase", "D": "D_s2_chase", "F": "F_s1_chase", "L": "L_s2_chase", "T": "T_s3_chase"}


def _episode(name, **over):
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool, VecGame
    z, meta = load_episode(EPISODES[name])
    cfg = config_for(meta, scen_route_len=len(z["scen:route"]), **over)
    s = scenario_arrays(z)
    env = VecGame(1, device="cuda:0", config=cfg)
    env.load_scenarios(ScenarioPool(cfg, s["static_rects"][None], s["robot_pos"][None], s["robot_dir"][None], s["robot_rect"][None],
                                    [s["route"]], [s["init_traj"]], "cuda:0"))
    env.reset(torch.zeros(1, dtype=torch.int32))
    return env, z


def _step(env, z, t):
    raw = z["actions_raw"] if "actions_raw" in z else None
    if raw is None:
        a = torch.tensor(z["actions"][t][None], dtype=torch.float64, device="cuda:0")
    else:
        a = torch.full((1,), raw[t].item(), dtype=torch.int32 if raw.dtype == np.int32 else torch.float64, device="cuda:0")
    env.step(a)


def _views(cfg, sc):
    """(scale, size, origin) of the three views: full size at scale 1, scale 4, and a window around the follower at scale 1.5."""
    fx, fy = (float(v) for v in sc["rb_pos"][1])
    return [(1.0, None, (0.0, 0.0)), (4.0, None, (0.0, 0.0)), (1.5, (256, 192), (fx - 190.25, fy - 140.5))]


def _check(env, e, scale, size, origin, layers=None, got=None, tag=""):
    sc = env_scene(env, e)
    if got is None:
        got = env.render([e], scale=scale, size=size, origin=origin, layers=layers)[0]
    torch.cuda.synchronize()
    h, w = got.shape[:2]
    want, band = render_scene(env.cfg, sc, w, h, scale, origin, env.render_layers() if layers is None else layers)
    r = compare(got.cpu().numpy(), want, band)
    assert r["ok"], (tag, scale, size, origin, layers, r)
    return want


@pytest.mark.parametrize("name", sorted(EPISODES))
def test_render_matches_numpy_along_a_golden_episode(name):
    env, z = _episode(name)
    T = len(z["actions"])
    moments = {-1: "reset", T // 2: "mid-episode", T - 1: "end"}
    views = _views(env.cfg, env_scene(env, 0))
    for t in range(-1, T):
        if t >= 0:
            _step(env, z, t)
        if t in moments:
            for scale, size, origin in views:
                img = _check(env, 0, scale, size, origin, tag=(name, moments[t]))
                if scale == 1.0 and size is None:
                    assert img.shape == (env.cfg.c.height, env.cfg.c.width, 3)
    assert bool(env.done[0]) == bool(z["done"][T - 1])
    env.close()


@pytest.mark.parametrize("name", ["B", "T"])
def test_each_layer_alone(name):
    env, z = _episode(name)
    for t in range(len(z["actions"]) // 2):
        _step(env, z, t)
    for bit in (abi.RENDER_PATH, abi.RENDER_BOX, abi.RENDER_OBJECTS, abi.RENDER_RECTS, abi.RENDER_SENSORS, abi.RENDER_TARGET,
                abi.RENDER_OBJECTS | abi.RENDER_RECTS, 0):
        for scale in (1.0, 4.0):
            _check(env, 0, scale, None, (0.0, 0.0), layers=bit, tag=(name, bit))
    blank = env.render([0], layers=abi.RENDER_RECTS)[0]           # RECTS draws nothing without OBJECTS
    assert bool((blank == 255).all())
    env.close()


@pytest.mark.parametrize("flag", ["show_leader_path_flag", "show_box_flag", "show_objects_flag", "show_rectangles_flag", "show_sensors_flag"])
def test_show_flags_select_the_layers(flag):
    env, z = _episode("B", **{flag: False})
    for t in range(30):
        _step(env, z, t)
    layers = env.render_layers()
    assert layers == abi.RENDER_ALL & ~{"show_leader_path_flag": abi.RENDER_PATH, "show_box_flag": abi.RENDER_BOX,
                                        "show_objects_flag": abi.RENDER_OBJECTS, "show_rectangles_flag": abi.RENDER_RECTS,
                                        "show_sensors_flag": abi.RENDER_SENSORS}[flag]
    _check(env, 0, 1.0, None, (0.0, 0.0), tag=flag)
    _check(env, 0, 4.0, None, (0.0, 0.0), tag=flag)
    env.close()


def _pool_B(**over):
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    z = np.load(GOLDEN + "/pool_B.npz")
    meta = json.loads(str(z["meta"]))
    cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()), **over)
    return cfg, ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0")


def _actions(cfg, n, t):
    g = torch.Generator(device="cpu").manual_seed(1000 + t)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    v = (0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)) * ms
    w = torch.clamp(torch.randn(n, generator=g, dtype=torch.float64) * 0.3 * mr, -mr, mr)
    return torch.stack([v, w], 1).contiguous().cuda()


OUT = ("obs_num", "lasers", "target", "reward", "done", "status")


def test_render_changes_nothing():
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg, pool = _pool_B(max_steps=120, warm_start=10)
    n = 96
    a, b = VecGame(n, config=cfg), VecGame(n, config=cfg)
    for e in (a, b):
        e.load_scenarios(pool)
        e.reset(torch.arange(n, dtype=torch.int32) % pool.n)
    ids = torch.tensor([0, 5, 5, 95, 17, 40], dtype=torch.int32)
    torch.cuda.synchronize()
    blob, outs = a.state.clone(), [getattr(a, k).clone() for k in OUT]
    for scale in (1.0, 4.0):
        a.render(ids, scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(blob, a.state) and all(torch.equal(o, getattr(a, k)) for o, k in zip(outs, OUT))
    frames = torch.empty(40, len(ids), 125, 188, 3, dtype=torch.uint8, device="cuda:0")   # a recorder's [T, k, H, W, 3] buffer
    for t in range(40):
        act = _actions(cfg, n, t)
        a.step(act, auto_reset=True)
        a.render(ids, scale=8.0, out=frames[t])
        b.step(act, auto_reset=True)
        for k in OUT:
            assert torch.equal(getattr(a, k), getattr(b, k)), (t, k)
    torch.cuda.synchronize()
    assert torch.equal(a.state[a._state_off:a._state_off + a.lib.ftl_state_bytes(a.h)],
                       b.state[b._state_off:b._state_off + b.lib.ftl_state_bytes(b.h)])
    # the last recorded frame is what a fresh render of the same state draws
    assert torch.equal(frames[39], a.render(ids, scale=8.0))
    a.close(); b.close()


def test_pipelined_render_spans_parts_under_a_cost_sort(monkeypatch):
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    monkeypatch.setenv("FTL_NO_REGROUP", "0")          # the cost-sorted slot -> env permutation is active in every part
    cfg, pool = _pool_B(max_steps=80, warm_start=10)
    n = 256
    p, v = PipelinedVecGame(n, parts=2, config=cfg), VecGame(n, config=cfg)
    for e in (p, v):
        e.load_scenarios(pool)
        e.reset(torch.arange(n, dtype=torch.int32) % pool.n)
    for t in range(12):
        act = _actions(cfg, n, t)
        p.step(act, auto_reset=True)
        v.step(act, auto_reset=True)
    p.join()
    ids = [3, 200, 3, 130, 127, 128, 255, 0, 200]
    got = p.render(ids, scale=2.0)
    got_gpu_ids = p.render(torch.tensor(ids, dtype=torch.int32, device="cuda:0"), scale=2.0)
    for j, e in enumerate(ids):
        want = v.render([e], scale=2.0)[0]
        assert torch.equal(got[j], want), (j, e)
    assert torch.equal(got, got_gpu_ids)
    _check(p, 130, 2.0, None, (0.0, 0.0), got=got[3], tag="pipelined")
    p.close(); v.close()


def test_game_render_returns_the_screen():
    from continiousenvironment_follower_leader_amd.game import Game
    g = Game()
    g.seed(3)
    g.reset()
    img = g.render()
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (1000, 1500, 3)
    assert (img != 255).any()
    g.step(np.array([0.2, 1.0]))
    img2 = g.render(custom_message="ignored")
    assert img2.shape == (1000, 1500, 3)
    assert g.render(scale=4.0).shape == (250, 375, 3)
    g.close()
    g = Game(return_render_matrix=False)
    g.seed(3)
    g.reset()
    assert g.render() is None
    g.close()


def test_render_in_a_large_stepping_loop():
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg, pool = _pool_B()
    n = 65536
    env = VecGame(n, config=cfg)
    env.load_scenarios(pool)
    env.reset(torch.arange(n, dtype=torch.int32) % pool.n)
    rng = np.random.default_rng(7)
    ids = torch.from_numpy(np.sort(rng.choice(n, 256, replace=False)).astype(np.int32)).cuda()
    frames = None
    for t in range(6):
        env.step(_actions(cfg, n, t), auto_reset=True)
        frames = env.render(ids, scale=8.0)
    torch.cuda.synchronize()
    assert frames.shape == (256, 125, 188, 3)
    for j in rng.choice(256, 8, replace=False):
        _check(env, int(ids[j]), 8.0, None, (0.0, 0.0), got=frames[j], tag=("65536", int(ids[j])))
    env.close()
