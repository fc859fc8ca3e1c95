"""The ray kernel exists in two forms: one that loops over the two scan passes (the ray sensors listed before the tracker, then those
listed after it) and one without the loop, launched when every ray sensor of the config sits on one side of the tracker
(ftl_device.hpp: ONE_PASS; FTL_RAYS_ONE_PASS=0 at ftl_create keeps the loop form).  Config B's world with its two
LeaderCorridor_Prev_lasers_v2 sensors behind the tracker's key (pass 1 only: the one-pass form), in front of it (pass 0 only: the
one-pass form on the other pass) and one on each side (two passes: the loop form): every output against the oracle batch at reset and
after every step, and for the two one-pass layouts the same run in the loop form, outputs and state bit for bit.  The same for the
CAPPED instantiations (config E, whose tracker ring is longer than its LDS copy), staged and unstaged."""
import numpy as np
import pytest
import torch

from golden_util import config_for, load_episode
from oracle_batch import OracleBatch, pool_scenarios
from test_gpu_configs import _actions, _compare_with_oracle, _vec

pytestmark = pytest.mark.gpu

OUTS = ("obs_num", "lasers", "target", "reward", "done", "status")


def _layout_config(layout):
    _, meta = load_episode("B_s1_chase")
    kw = dict(meta["kwargs"])
    src = kw["follower_sensors"]
    tracker = "LeaderPositionsTracker_v2"
    rays = [k for k, v in src.items() if v["sensor_class"] == "LeaderCorridor_Prev_lasers_v2"]
    assert len(rays) == 2 and tracker in src and len(src) == 3
    order = {"behind": [tracker, rays[0], rays[1]], "front": [rays[0], rays[1], tracker], "both": [rays[0], tracker, rays[1]]}[layout]
    kw["follower_sensors"] = {k: src[k] for k in order}
    cfg = config_for(dict(kwargs=kw, post=None), scen_route_len=256)
    want = {"behind": [1, 1], "front": [0, 0], "both": [0, 1]}[layout]
    assert [int(cfg.c.lasers[k].after_tracker) for k in range(cfg.c.n_lasers)] == want
    return cfg


def _state_bytes(env):
    return env.state[env._state_off:env._state_off + env.lib.ftl_state_bytes(env.h)]


@pytest.mark.parametrize("layout", ["behind", "front", "both"])
def test_pass_layouts_match_oracle_and_the_loop_form(monkeypatch, layout):
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    n, steps = 256, 40
    cfg = _layout_config(layout)
    pool = ScenarioPool.generate(cfg, np.arange(128), "cuda:0")
    monkeypatch.delenv("FTL_RAYS_ONE_PASS", raising=False)
    env = _vec(n, cfg, pool)               # the one-pass form for "behind" / "front", the loop form for "both"
    loop = None
    if layout != "both":
        monkeypatch.setenv("FTL_RAYS_ONE_PASS", "0")
        loop = _vec(n, cfg, pool)
        monkeypatch.delenv("FTL_RAYS_ONE_PASS")

    def same_as_loop(tag):
        for name in OUTS:
            assert torch.equal(getattr(env, name), getattr(loop, name)), (layout, tag, name)
        assert torch.equal(_state_bytes(env), _state_bytes(loop)), (layout, tag, "state")

    scen = pool_scenarios(pool)
    idx = (np.arange(n) * 3) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n)
    ora.reset(scen, idx)
    _compare_with_oracle(env, ora, cfg, ("one pass", layout, "reset"))
    if loop is not None:
        loop.reset(torch.from_numpy(idx.astype(np.int32)))
        same_as_loop("reset")
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=31)
        act = torch.tensor(a, dtype=torch.float64, device="cuda:0")
        env.step(act)
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, ("one pass", layout, t))
        if loop is not None:
            loop.step(act)
            same_as_loop(t)
    las = env.lasers.cpu().numpy()
    for l in cfg.lasers:      # every sensor saw something: a block that still reads its laser length everywhere would compare equal for nothing
        blk = las[:, l.out_offset:l.out_offset + l.history * l.width]
        assert (blk != np.float32(l.length)).any(), l.name
    assert env.error_report() == (0, 0)
    env.close()
    if loop is not None:
        assert loop.error_report() == (0, 0)
        loop.close()


@pytest.mark.parametrize("lds_cap", [None, 8])
def test_capped_one_pass_form_matches_oracle_and_the_loop_form(monkeypatch, lds_cap):
    """Config E (leader regimes: a tracker ring of 256 points, longer than its LDS copy) runs the CAPPED instantiations, which have the
    one-pass form too; with FTL_DEBUG_CORR_LDS_CAP=8 every window is too long for the copy and phase 3 reads the ring in place."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    n, steps = 256, 40
    _, meta = load_episode("E_s3_chase")
    cfg = config_for(meta, scen_route_len=256, rng_seed=9, env_id_base=7000)
    assert cfg.c.corr_cap > 128 and all(int(cfg.c.lasers[k].after_tracker) == 1 for k in range(cfg.c.n_lasers))
    pool = ScenarioPool.generate(cfg, np.arange(128), "cuda:0")
    monkeypatch.delenv("FTL_RAYS_ONE_PASS", raising=False)
    if lds_cap:
        monkeypatch.setenv("FTL_DEBUG_CORR_LDS_CAP", str(lds_cap))
    env = _vec(n, cfg, pool)
    monkeypatch.setenv("FTL_RAYS_ONE_PASS", "0")
    loop = _vec(n, cfg, pool)
    monkeypatch.delenv("FTL_RAYS_ONE_PASS")
    monkeypatch.delenv("FTL_DEBUG_CORR_LDS_CAP", raising=False)
    scen = pool_scenarios(pool)
    idx = (np.arange(n) * 5) % pool.n
    ora = OracleBatch(cfg, n, env_id_base=7000)
    ora.reset(scen, idx)
    for e in (env, loop):
        e.reset(torch.from_numpy(idx.astype(np.int32)))
    _compare_with_oracle(env, ora, cfg, ("capped one pass", lds_cap, "reset"))
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=33)
        act = torch.tensor(a, dtype=torch.float64, device="cuda:0")
        env.step(act); loop.step(act)
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, ("capped one pass", lds_cap, t))
        for name in OUTS:
            assert torch.equal(getattr(env, name), getattr(loop, name)), (lds_cap, t, name)
        assert torch.equal(_state_bytes(env), _state_bytes(loop)), (lds_cap, t, "state")
    las = env.lasers.cpu().numpy()
    for l in cfg.lasers:
        blk = las[:, l.out_offset:l.out_offset + l.history * l.width]
        assert (blk != np.float32(l.length)).any(), l.name
    assert env.error_report() == (0, 0) and loop.error_report() == (0, 0)
    env.close(); loop.close()
