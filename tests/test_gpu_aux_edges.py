"""csrc/ftl_aux.hpp at the limits of its staging, HIP against the oracle: the lidar's rect list in its three regimes (a 64-bit candidate
mask, the tail loop behind it, the overflow past 128 rects), its float-quotient index split up to 65,535 (ray, point) pairs, compas
sensors on a corridor window longer than the LDS stage, detectors longer than a wavefront on the v2 tracker and on every setting of the
v1 tracker.  The cases live in tests/aux_edge_cases.py; tests/test_aux_edges_host.py shows on the oracle alone that each reaches its
branch, tests/test_oracle_golden.py pins the oracle to the reference there (episodes Ledge, Clong, Tnoeat).  Tolerance and waivers are
those of tests/test_gpu_configs.py and tests/test_gpu_fuzz.py, counted in the same session totals."""
import numpy as np
import pytest
import torch

import aux_edge_cases as X
from continiousenvironment_follower_leader_amd import abi
from golden_util import RADAR_BUDGET, close, radar_slice, radar_touches_boundary
from oracle_batch import OracleBatch
from test_gpu_configs import WAIVERS, _actions, _compare_with_oracle, _vec
from test_gpu_fuzz import _compare as _compare_v2

pytestmark = pytest.mark.gpu

CAP_BITS = abi.FTL_ERR_TRAJ_OVERFLOW | abi.FTL_ERR_CORR_OVERFLOW | abi.FTL_ERR_HIST1_OVERFLOW


@pytest.fixture(autouse=True, params=["4 lanes per env", "8 lanes per env"])
def lanes_per_env(request, monkeypatch):
    """Both forms of the frame kernel, as in tests/test_gpu_parity.py (every batch here is small enough to choose)."""
    monkeypatch.setenv("FTL_DEBUG_G8", "0" if request.param.startswith("4") else "1")


def _compare(env, ora, cfg, tag, stats):
    """tests/test_gpu_fuzz.py::_compare; on the v1 tracker the radar knife-edge criterion (golden_util.radar_touches_boundary, the one
    arithmetic of that waiver) looks at the float32 history list of that tracker instead of the v2 ring."""
    if cfg.c.has_tracker != 1:
        return _compare_v2(env, ora, cfg, tag, stats)
    radars = [j for j in range(cfg.c.n_aux) if cfg.c.aux[j].kind == abi.AUX_TRACK_RADAR]
    L = cfg.lasers_len
    edge = np.zeros((env.n, L), bool)
    if radars:
        ei = env.state_field("env_int").cpu().numpy()
        pos = env.state_field("rb_pos").cpu().numpy().reshape(env.n, cfg.n_robots, 2)[:, 1].astype(np.float64)
        fdir = env.state_field("rb_dbl").cpu().numpy().reshape(env.n, cfg.n_robots, abi.RD_COUNT)[:, 1, abi.RD_DIRECTION]
        hist = env.state_field("hist1").cpu().numpy().reshape(env.n, -1, 2).astype(np.float64)
        for j in radars:
            A = cfg.c.aux[j]
            for e in range(env.n):
                s0, s1 = radar_slice(int(ei[e, abi.EI_HIST1_LEN]), A.detectable, A.seq_len)
                if s1 > s0 and radar_touches_boundary(hist[e, s0:s1], pos[e], fdir[e], A.radar_sectors):
                    edge[e, A.out_offset:A.out_offset + A.radar_sectors] = True
    if edge.any():
        las = env.lasers.cpu().numpy()
        stats[0] += int((edge & (las[:, :L] != ora.lasers[:, :L])).any(1).sum())
        ora.lasers[:, :L][edge] = las[:, :L][edge]
    stats[1] += env.n
    _compare_with_oracle(env, ora, cfg, tag)


def _finish(env, cfg, err_seen, stats, tag, extra_bits=0, extra_envs=None):
    """Case e: the sticky error words against the OR of the oracle's (plus `extra_bits` in the envs `extra_envs`), no capacity bit,
    the radar waivers of the case within the per-config budget and into the session totals."""
    seen = err_seen.copy()
    if extra_envs is not None:
        seen[extra_envs] |= extra_bits
    rep = env.error_report()
    assert rep == (int((seen != 0).sum()), int(np.bitwise_or.reduce(seen))), (tag, rep, np.unique(seen))
    assert rep[1] & CAP_BITS == 0, (tag, hex(rep[1]))
    sticky = env.state_field("env_int")[:, abi.EI_ERROR_STICKY].cpu().numpy()
    assert np.array_equal(sticky.astype(np.int64), seen), (tag, "sticky error words")
    WAIVERS["radar_env_steps"] += stats[0]; WAIVERS["env_steps"] += stats[1]
    WAIVERS["radar_worst"] = max(WAIVERS["radar_worst"], stats[0] / max(stats[1], 1))
    assert stats[0] <= RADAR_BUDGET * stats[1], (tag, stats)


def _dev(a, dtype=torch.float64):
    return torch.tensor(a, dtype=dtype, device="cuda:0")


def _reset(env, ora, scen, idx, mask=None):
    if mask is None:
        env.reset(torch.from_numpy(idx.astype(np.int32)))
    else:
        env.reset(torch.from_numpy(idx.astype(np.int32)), mask=torch.from_numpy(mask.astype(np.uint8)))
    ora.reset(scen, idx, mask=mask)


# ---- a. lidar rect staging --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["distances", "all_points"])
def test_lidar_rect_list_mask_tail_and_overflow(variant):
    """32 dense worlds x 8 steps, three lidars on one follower: 33-37 objects in range of the first (the mask alone), 91-93 of the second
    (rects 64.. go through the tail loop; tests/test_aux_edges_host.py shows that they stop rays), 154-155 of the third.  The first two
    equal the oracle's and raise nothing.  The third raises FTL_ERR_LIDAR_OVERFLOW, live and sticky, in exactly the envs a numpy count
    puts above 128; it ignores the rects past the 128th, so each of its rays reads at least what the oracle reads (which has no cap)
    and at most its range -- to be exact, what the ray reads when nothing stops it: the float32 norm of its end minus the position, which
    in the reference's own records exceeds the range of 250 by up to 8e-5; everything else in those envs still equals the oracle's."""
    cfg = X.dense_config(variant)
    scen = X.dense_scenarios(cfg)
    n = X.DENSE_ENVS
    env = _vec(n, cfg, X.scenario_pool(cfg, scen, "cuda:0"))
    ora = OracleBatch(cfg, n)
    idx = np.arange(n)
    _reset(env, ora, scen, idx)
    j5 = [a.name for a in cfg.aux].index("lidar_r5")
    A5, blk = cfg.c.aux[j5], slice(cfg.aux[j5].out_offset, cfg.aux[j5].out_offset + cfg.aux[j5].out_len)
    stats, err_seen, over_live, over_ever, longer = [0, 0], np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n, bool), 0

    def check(tag, fresh=None):
        nonlocal over_live, over_ever, longer
        counts = X.lidar_counts(cfg, ora, scen, idx)
        for j, (cnt, gap, _) in counts.items():
            assert gap > 1e-6, (tag, cfg.aux[j].name, "an object on the range threshold")
            if j != j5:
                assert (cnt <= X.LIDAR_RECTS).all(), (tag, cfg.aux[j].name, cnt.max())
        over = counts[j5][0] > X.LIDAR_RECTS
        over_live = over | (over_live & ~fresh) if fresh is not None else over | over_live
        over_ever |= over
        ei = env.state_field("env_int").cpu().numpy()
        ora_err = X.oracle_counters(ora)[:, 14]
        err_seen[:] |= ora_err
        assert np.array_equal(ei[:, abi.EI_ERROR] & abi.FTL_ERR_LIDAR_OVERFLOW != 0, over_live), (tag, "live overflow bit")
        assert np.array_equal(ei[:, abi.EI_ERROR_STICKY] & abi.FTL_ERR_LIDAR_OVERFLOW != 0, over_ever), (tag, "sticky overflow bit")
        assert np.array_equal(ei[:, abi.EI_ERROR] & ~abi.FTL_ERR_LIDAR_OVERFLOW, ora_err), (tag, "other error bits")
        got, ref = env.lasers.cpu().numpy()[:, blk], ora.lasers[:, blk]
        tol = np.maximum(1e-5, np.spacing(np.maximum(got, ref).astype(np.float32)).astype(np.float64))
        assert (got[over] >= ref[over] - tol[over]).all(), (tag, "a ray of the overflowing lidar reads less than the oracle's")
        pos, fdir, _ = X.oracle_robots(ora)
        free = np.stack([X.lidar_free_readings(A5, pos[e, 1], fdir[e, 1]) for e in range(n)]).astype(np.float64)
        assert (got[over] <= free[over] + tol[over]).all(), (tag, "a ray of the overflowing lidar reads more than a ray that nothing stops")
        longer += int((~close(got[over], ref[over])).sum())
        ref[over] = got[over]
        _compare(env, ora, cfg, tag, stats)

    check((variant, "reset"))
    for t in range(X.DENSE_STEPS):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=31)
        env.step(_dev(a)); ora.step(a)
        check((variant, t))
        r = X.dense_reset(t, idx, len(scen))
        if r is not None:
            idx = r[1]
            _reset(env, ora, scen, idx, mask=r[0])
            check((variant, t, "masked reset"), fresh=r[0])
    assert over_ever.all()
    print("aux_edges dense[%s]: %d readings of the overflowing lidar longer than the oracle's" % (variant, longer))
    _finish(env, cfg, err_seen, stats, variant, abi.FTL_ERR_LIDAR_OVERFLOW, over_ever)
    env.close()


# ---- b. lidar index split ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rays", "all_points"])
def test_lidar_index_split(which):
    """(n_angles, points_number) = (361, 181), (127, 513), (3, 1000), (1, 1023) as distances and as points, and (63, 1024) with
    return_all_points in both forms (129,025 and 64,513 floats per env): 8 envs x 5 steps, every reading against the oracle."""
    cfg = X.split_config(which)
    n = X.SPLIT_ENVS
    scen = X.generated_scenarios(cfg, np.arange(12))[:n]
    env = _vec(n, cfg, X.scenario_pool(cfg, scen, "cuda:0"))
    ora = OracleBatch(cfg, n)
    idx = np.arange(n)
    _reset(env, ora, scen, idx)
    stats, err_seen = [0, 0], np.zeros(n, np.int64)
    _compare(env, ora, cfg, (which, "reset"), stats)
    for t in range(X.SPLIT_STEPS):
        a = _actions(cfg, n, t, seed=37)
        env.step(_dev(a)); ora.step(a)
        _compare(env, ora, cfg, (which, t), stats)
        err_seen |= X.oracle_counters(ora)[:, 14]
    _finish(env, cfg, err_seen, stats, which)
    assert env.error_report()[1] & abi.FTL_ERR_LIDAR_OVERFLOW == 0
    env.close()


@pytest.mark.parametrize("which,message", [("pairs", "65535"), ("points", "1024 points per ray")])
def test_create_refuses_a_lidar_past_the_index_split(which, message):
    """361 x 182 pairs and 1025 points per ray pass make_config; ftl_create refuses them and says why."""
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg = X.refused_lidar_config(which)
    with pytest.raises(ValueError, match=message):
        VecGame(4, device="cuda:0", config=cfg)


# ---- c. compas off the stage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy_obs", [False, True])
def test_compas_on_a_window_longer_than_the_stage(policy_obs):
    """The config of episode Clong on 64 envs x 70 steps with an explicit reset of an eighth of the envs every 10 steps: corridor windows
    of exactly 128 points (staged in LDS) and of 129 and more (read from the ring in place) both occur.  A second handle takes the same
    steps without sensors and scans once at the end: the same readings bit for bit.  With policy_obs (one history length for all
    sensors, as the wrapper demands) the fused rows of the compas sensors are the clipped readings over the ray length."""
    cfg = X.compas_config(history=8 if policy_obs else None)
    scen = X.generated_scenarios(cfg, np.arange(96))
    n = X.COMPAS_ENVS
    pool = X.scenario_pool(cfg, scen, "cuda:0")
    env, blind = _vec(n, cfg, pool, policy_obs=policy_obs), _vec(n, cfg, pool)
    ora = OracleBatch(cfg, n)
    idx = np.arange(n) % len(scen)
    _reset(env, ora, scen, idx)
    blind.reset(torch.from_numpy(idx.astype(np.int32)))
    stats, err_seen, seen = [0, 0], np.zeros(n, np.int64), set()

    def check(tag):
        _compare(env, ora, cfg, tag, stats)
        cnt = X.oracle_counters(ora)
        err_seen[:] |= cnt[:, 14]
        seen.update(int(v) for v in cnt[:, 13])
        ei = env.state_field("env_int").cpu().numpy()
        assert np.array_equal(ei[:, abi.EI_CORR_HI] - ei[:, abi.EI_CORR_LO], cnt[:, 13]), (tag, "corridor length")
        if policy_obs:
            las, pol, off = env.lasers.cpu().numpy(), env.policy_obs.cpu().numpy(), 0
            for l in cfg.lasers:
                if not l.in_policy_obs:
                    continue
                if l.compas:
                    rows = las[:, l.out_offset:l.out_offset + l.history * l.width].reshape(n, l.history, l.width)
                    want = np.clip(rows / np.float32(l.length), np.float32(0), np.float32(1))
                    assert np.array_equal(pol[:, :, off:off + l.width], want), (tag, l.name, "policy_obs")
                off += l.width
        return cnt[:, 13]

    check("reset")
    for t in range(X.COMPAS_STEPS):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=41)
        env.step(_dev(a)); ora.step(a); blind.step(_dev(a), sensors=False)
        w = check(t)
        r = X.periodic_reset(t, 10, idx, len(scen))
        if r is not None:
            idx = r[1]
            _reset(env, ora, scen, idx, mask=r[0])
            blind.reset(torch.from_numpy(idx.astype(np.int32)), mask=torch.from_numpy(r[0].astype(np.uint8)))
            check((t, "masked reset"))
    assert X.COMPAS_STAGE in seen and X.COMPAS_STAGE + 1 in seen and (w > X.COMPAS_STAGE).sum() * 2 >= n, sorted(seen)[-5:]
    blind.scan()
    assert torch.equal(blind.lasers, env.lasers), "scan() after steps without sensors"
    _finish(env, cfg, err_seen, stats, "compas")
    env.close(); blind.close()


# ---- d. detectors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracker", X.DETECT_TRACKERS)
def test_detectors_longer_than_a_wavefront(tracker):
    """48 envs x 90 steps, eight detectors per config (position_sequence_length 1 / 64 / 65 / 300 with every detectable_positions value,
    1 / 7 / 180 / 181 / 4096 radar sectors over the seven configs) on the v2 tracker saving every scan and on the v1 tracker with
    saving_period 1 / 3 / 7, eating or not; every 10th step the tracker's own state -- counter, history, corridor -- against the oracle's."""
    cfg = X.detector_config(tracker)
    scen = X.generated_scenarios(cfg, np.arange(64))
    n = X.DETECT_ENVS
    env = _vec(n, cfg, X.scenario_pool(cfg, scen, "cuda:0"))
    ora = OracleBatch(cfg, n)
    idx = np.arange(n) % len(scen)
    _reset(env, ora, scen, idx)
    stats, err_seen = [0, 0], np.zeros(n, np.int64)
    _compare(env, ora, cfg, (tracker, "reset"), stats)
    err_seen |= X.oracle_counters(ora)[:, 14]
    for t in range(X.DETECT_STEPS):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=43)
        env.step(_dev(a)); ora.step(a)
        _compare(env, ora, cfg, (tracker, t), stats)
        err_seen |= X.oracle_counters(ora)[:, 14]
        if t % 10 == 9:
            ei = env.state_field("env_int").cpu().numpy()
            for e, o in enumerate(ora.envs):
                d = o.debug()
                n_hist = ei[e, abi.EI_HIST1_LEN] if cfg.c.has_tracker == 1 else ei[e, abi.EI_CORR_HI] - ei[e, abi.EI_CORR_LO]
                got = (ei[e, abi.EI_TRK_COUNTER], n_hist, ei[e, abi.EI_CORR_HI] - ei[e, abi.EI_CORR_LO])
                assert tuple(int(v) for v in got) == tuple(int(v) for v in d["counters"][11:14]), (tracker, t, e, got, d["counters"][11:14])
                hist, corr = env.tracker_obs(e)
                assert np.allclose(hist, d["hist"], rtol=0, atol=1e-9), (tracker, t, e, "tracker history")
                assert np.allclose(corr.reshape(-1, 4), d["corr"], rtol=0, atol=1e-9), (tracker, t, e, "corridor")
    _finish(env, cfg, err_seen, stats, tracker)
    env.close()
