"""The ray kernel reads its rays from host-built tables in PASS order: the rays of the sensors scanned before the tracker, then those of
the sensors scanned after it, compas entries left out.  make_config lists the sensors in dict order, where every sensor behind the
tracker's key is an after-tracker one -- so there pass order and config order agree.  A caller of the C ABI may list them in any order.
Here the sensor entries of the ctypes config are permuted (an after-tracker sensor first, a compas entry in the middle, the
before-tracker sensor behind them; three different laser lengths and ray counts) and every output is compared with the oracle batch,
which scans by the same flags and output offsets."""
import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import config_for, load_episode
from oracle_batch import OracleBatch, pool_scenarios
from test_gpu_configs import _actions, _compare_with_oracle, _vec

pytestmark = pytest.mark.gpu


def _prev(count, length, hist, corridor, green, obstacles, offset):
    return dict(sensor_class="LeaderCorridor_Prev_lasers_v2", react_to_safe_corridor=corridor, react_to_green_zone=green,
                react_to_obstacles=obstacles, lasers_count=count, laser_length=length, max_prev_obs=hist, use_prev_obs=True,
                pad_sectors=False, first_laser_angle_offset=offset)


def _permuted_config(with_compas):
    _, meta = load_episode("B_s1_chase")
    kw = dict(meta["kwargs"])
    tracker = kw["follower_sensors"]["LeaderPositionsTracker_v2"]
    sensors = {"before": _prev(12, 150, 5, True, True, True, -45)}
    sensors["LeaderPositionsTracker_v2"] = tracker
    sensors["after_long"] = _prev(24, 200, 5, False, False, True, 0)
    if with_compas:
        sensors["compas"] = dict(sensor_class="LeaderCorridor_lasers_compas", react_to_green_zone=True, react_to_safe_corridor=True,
                                 react_to_obstacles=False, lasers_count=12, laser_length=90, max_prev_obs=5, pad_sectors=False)
    sensors["after_short"] = _prev(20, 100, 3, True, False, "static", 10)
    kw["follower_sensors"] = sensors
    cfg = config_for(dict(kwargs=kw, post=None), scen_route_len=256)
    names = [l.name for l in cfg.lasers]
    order = ["after_long"] + (["compas"] if with_compas else []) + ["before", "after_short"]
    perm = [names.index(n) for n in order]
    assert sorted(perm) == list(range(len(names))) and perm != sorted(perm)
    entries = [type(cfg.c.lasers[0]).from_buffer_copy(cfg.c.lasers[k]) for k in range(len(names))]
    specs = [cfg.lasers[k] for k in perm]
    off = 0
    for k, (src, spec) in enumerate(zip(perm, specs)):
        cfg.c.lasers[k] = entries[src]
        cfg.c.lasers[k].out_offset = off
        spec.out_offset = off
        off += spec.history * spec.width
    total = cfg.lasers_len
    cfg.lasers[:] = specs
    assert cfg.lasers_len == total == off
    assert [int(cfg.c.lasers[k].after_tracker) for k in range(len(names))] == ([1, 1, 0, 1] if with_compas else [1, 0, 1])
    return cfg


@pytest.mark.parametrize("with_compas", [False, True])
def test_sensors_listed_out_of_pass_order_match_oracle(with_compas):
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    n, steps = 256, 40
    cfg = _permuted_config(with_compas)
    pool = ScenarioPool.generate(cfg, np.arange(128), "cuda:0")
    env = _vec(n, cfg, pool)
    scen = pool_scenarios(pool)
    idx = (np.arange(n) * 3) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n)
    ora.reset(scen, idx)
    _compare_with_oracle(env, ora, cfg, ("order", with_compas, "reset"))
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=29)
        env.step(torch.tensor(a, dtype=torch.float64, device="cuda:0"))
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, ("order", with_compas, t))
    las = env.lasers.cpu().numpy()
    for l in cfg.lasers:      # every sensor saw something: a block that still reads its laser length everywhere would compare equal for nothing
        blk = las[:, l.out_offset:l.out_offset + l.history * l.width]
        assert (blk != np.float32(l.length)).any(), l.name
    assert env.error_report() == (0, 0)
    env.close()


def test_after_tracker_is_a_flag():
    """ftl_create keeps after_tracker as 0 / 1 whatever non-zero value the caller passed: host tables and kernels compare it with the pass."""
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg = _permuted_config(False)
    cfg.c.lasers[0].after_tracker = 2
    env = VecGame(4, device="cuda:0", config=cfg)
    got = abi.Config()
    env.lib.ftl_get_config(env.h, got)
    assert [int(got.lasers[k].after_tracker) for k in range(3)] == [1, 0, 1]
    env.close()
