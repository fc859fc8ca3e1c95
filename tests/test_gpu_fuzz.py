"""Randomised configs against the oracle: the golden episodes and the named configs pin a dozen points of the config space; this
walks through it -- sensor sets in random dict order around the tracker (both scan passes), every react_to_* combination, history
lengths 1-12, pad_sectors, 0-4 dynamic obstacles (the 4- and 8-lane instantiations of the frame kernel), frame counts, regimes,
random frames per step, early stopping.  Every output of every env and step is compared with oracle/ftl_oracle.c, which the golden
episodes pin to the reference.  The draws are seeded: a failure names the seed that rebuilds its config."""
import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi, make_config
from fuzz_configs import TRACKER, _aux_sensor, _ray_sensor, draw_config  # noqa: F401  (the draws live there: importable without a GPU)
from golden_util import RADAR_BUDGET, radar_slice, radar_touches_boundary
from oracle_batch import OracleBatch, pool_scenarios
from test_gpu_configs import CORNER_BUDGET, WAIVERS, _actions, _compare_with_oracle, _vec

pytestmark = pytest.mark.gpu


def _radar_knife_edges(env, cfg):
    """(env, column) mask of LeaderTrackDetector_radar readings that sit on a knife edge.  A tracked point whose angle to the
    follower's right-hand vector equals a sector boundary to within rounding goes to one sector or its neighbour depending on the
    last bit of cos / sin of the heading (SEN:423-476: `ar >= sa * t and ar < sa * (t + 1)` on arccos values) -- which libm, numpy
    SIMD kernel or device routine produced it.  After reset() this is the rule, not the exception: the initial trajectory runs
    straight ahead of the follower, 90 degrees from the right-hand vector, and 90 degrees is a boundary for every even sector count.
    Such readings are excluded from the comparison (and counted); everything else must match."""
    from continiousenvironment_follower_leader_amd import abi
    mask = np.zeros((env.n, max(cfg.lasers_len, 1)), bool)
    radars = [j for j in range(cfg.c.n_aux) if cfg.c.aux[j].kind == abi.AUX_TRACK_RADAR]
    if not radars:
        return mask
    ei = env.state_field("env_int").cpu().numpy()
    pos = env.state_field("rb_pos").cpu().numpy().reshape(env.n, cfg.n_robots, 2)[:, 1].astype(np.float64)
    fdir = env.state_field("rb_dbl").cpu().numpy().reshape(env.n, cfg.n_robots, abi.RD_COUNT)[:, 1, abi.RD_DIRECTION]
    hist = env.state_field("hist").cpu().numpy().reshape(env.n, -1, 2)
    cap = hist.shape[1]
    for j in radars:
        A = cfg.c.aux[j]
        lo = ei[:, abi.EI_CORR_LO if A.after_tracker else abi.EI_HW0_LO]; hi = ei[:, abi.EI_CORR_HI if A.after_tracker else abi.EI_HW0_HI]
        for e in range(env.n):
            s0, s1 = radar_slice(int(hi[e] - lo[e]), A.detectable, A.seq_len)
            if s1 <= s0:
                continue
            p = hist[e, (lo[e] + np.arange(s0, s1)) & (cap - 1)]
            if radar_touches_boundary(p, pos[e], fdir[e], A.radar_sectors):
                mask[e, A.out_offset:A.out_offset + A.radar_sectors] = True
    return mask


def _compare(env, ora, cfg, tag, stats):
    edge = _radar_knife_edges(env, cfg)
    if edge.any():
        las = env.lasers.cpu().numpy()
        L = cfg.lasers_len
        stats[0] += int((edge[:, :L] & (las[:, :L] != ora.lasers[:, :L])).any(1).sum())
        ora.lasers[:, :L][edge[:, :L]] = las[:, :L][edge[:, :L]]
    stats[1] += env.n
    _compare_with_oracle(env, ora, cfg, tag)


def _seeds():
    import os
    lo, hi = (int(x) for x in os.environ.get("FTL_FUZZ_SEEDS", "0:96").split(":"))      # a wider sweep: FTL_FUZZ_SEEDS=0:400 pytest ... (400 configs pass, 64 s)
    return range(lo, hi)


@pytest.mark.parametrize("seed", _seeds())
def test_random_config_matches_oracle(seed):
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    kw = draw_config(seed)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = make_config(route_cap=256, **kw)
    n, steps = 96, 60
    pool = ScenarioPool.generate(cfg, np.arange(16) + 50 * seed, "cuda:0")
    env = _vec(n, cfg, pool)
    scen = pool_scenarios(pool)
    idx = np.arange(n) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n, env_id_base=100 * seed)
    ora.reset(scen, idx)
    stats = [0, 0]            # radar readings excused as knife edges, env-steps compared
    err_seen = np.zeros(n, np.int64)
    _compare(env, ora, cfg, (seed, "reset"), stats)
    err_seen |= ora.counters()[2]               # (a sensor ahead of the tracker in the dict can find the corridor empty at reset already)
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed" if t % 3 == 2 else "random", seed=seed)
        env.step(torch.tensor(a, dtype=torch.float64, device="cuda:0"))
        ora.step(a)
        _compare(env, ora, cfg, (seed, t, sorted(kw["follower_sensors"])), stats)
        err_seen |= ora.counters()[2]
        d = ora.done.astype(bool)
        if d.any() and t % 12 == 11:                # masked reset of the finished envs on both sides
            idx = np.where(d, (idx + n) % pool.n, idx)
            env.reset(torch.from_numpy(idx.astype(np.int32)), mask=torch.from_numpy(d.astype(np.uint8)))
            ora.reset(scen, idx, mask=d)
            _compare(env, ora, cfg, (seed, t, "masked reset"), stats)
            err_seen |= ora.counters()[2]
    rep = env.error_report()             # sticky: the bits of every episode since the handle was created
    assert rep[0] == int((err_seen != 0).sum()) and rep[1] == int(np.bitwise_or.reduce(err_seen)), (seed, rep, np.unique(err_seen))
    # capacity overflows of the batched state are never part of a legitimate comparison: both sides would share the truncation
    cap_bits = abi.FTL_ERR_TRAJ_OVERFLOW | abi.FTL_ERR_CORR_OVERFLOW | abi.FTL_ERR_HIST1_OVERFLOW | abi.FTL_ERR_LIDAR_OVERFLOW
    assert rep[1] & cap_bits == 0, (seed, hex(rep[1]))
    WAIVERS["radar_env_steps"] += stats[0]; WAIVERS["env_steps"] += stats[1]
    WAIVERS["radar_worst"] = max(WAIVERS["radar_worst"], stats[0] / max(stats[1], 1))
    assert stats[0] <= RADAR_BUDGET * stats[1], (seed, stats)        # knife edges are the exception
    env.close()


def test_zz_waiver_budget():
    """Runs after the oracle comparisons of tests/test_gpu_configs.py and of this file: the session totals of the two knife-edge waivers
     against their budgets, printed and written to gpurun_out/waivers.json."""
    import json
    import os
    w = dict(WAIVERS)
    w["corner_fraction"] = w["corner"] / max(w["readings"], 1)
    w["radar_fraction"] = w["radar_env_steps"] / max(w["env_steps"], 1)
    print("waivers:", json.dumps(w))
    try:
        os.makedirs("gpurun_out", exist_ok=True)
        with open("gpurun_out/waivers.json", "w") as fh:
            json.dump(w, fh)
    except OSError:
        pass
    assert w["readings"] > 0
    assert w["corner"] <= CORNER_BUDGET * w["readings"] + 2 * abi.FTL_MAX_LASERS * 12, w
    assert w["radar_env_steps"] <= 0.5 * RADAR_BUDGET * max(w["env_steps"], 1) + 5, w
