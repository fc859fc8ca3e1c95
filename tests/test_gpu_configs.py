"""GPU parity tests of the BASELINE configs beyond B and of the kernel instantiations only they reach:
config D (100 rocks, one 180-ray sensor: the `n_static > 64` second pass and the wide-arc loop of the ray kernel),
config E (regimes, 2 bears) at its 32,768-envs-per-GPU size, and the two-stream split path of config F
(`ftl_rays_kernel<*, *, true>`), which is on by default from 8,192 envs under random_frames_per_step."""
import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import close, config_for, load_episode
from oracle_batch import OracleBatch, pool_scenarios

pytestmark = pytest.mark.gpu

_POOLS = {}


def _cfg_pool(ep, n_seeds, **over):
    """(cfg, ScenarioPool) of the config of golden episode `ep`, scenarios from the host generator (cached per test session)."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    key = (ep, n_seeds, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _POOLS:
        _, meta = load_episode(ep)
        cfg = config_for(meta, scen_route_len=256, **over)
        _POOLS[key] = (cfg, ScenarioPool.generate(cfg, np.arange(n_seeds), "cuda:0"))
    return _POOLS[key]


def _vec(n, cfg, pool, **kw):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    env = VecGame(n, device="cuda:0", config=cfg, **kw)
    env.load_scenarios(pool)
    return env


def _actions(cfg, n, t, policy="random", seed=0):
    rng = np.random.default_rng(seed * 7919 + t)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    v = rng.uniform(0.5, 1.0, n) * ms
    w = np.clip(rng.normal(0, 0.2 * mr, n), -mr, mr)
    if policy == "mixed":
        w[::3] = 0.0
        v[1::4] = 0.0
        w[2::5] = mr
    return np.stack([v, w], 1)


def _corner_grazes(env, cfg, bad):
    """(env, column) mask of the mismatching ray readings that are knife edges: the ray passes EXACTLY through a corner of an
    axis-aligned rect (a static one, or a robot's hitbox now or in one of the snapshots).  Whether the reference's strict `ccw`
    inequalities (SEN:608-614) count that as a hit depends on the last bit of cos / sin of the ray's direction -- numpy's, glibc's
    and the device's differ there.  It is not a measure-zero event: reset() puts the follower on an exact
    diagonal of the leader (x - y an integer) and the rects sit on a 5-px lattice, so a 45-degree ray meets lattice corners."""
    out = np.zeros_like(bad)
    pos = env.state_field("rb_pos").cpu().numpy().reshape(env.n, cfg.n_robots, 2)[:, 1].astype(np.float64)
    fdir = env.state_field("rb_dbl").cpu().numpy().reshape(env.n, cfg.n_robots, abi.RD_COUNT)[:, 1, abi.RD_DIRECTION]
    ei = env.state_field("env_int").cpu().numpy()
    ri = env.state_field("rb_int").cpu().numpy().reshape(env.n, cfg.n_robots, abi.RI_COUNT)[:, :, :4]
    sr = env.state_field("snap_rects").cpu().numpy().reshape(env.n, -1, 4)
    st = env.pool.t["static_rects"].cpu().numpy() if hasattr(env, "pool") and env.pool is not None else None
    for e, col in np.argwhere(bad):
        for k in range(cfg.c.n_lasers):
            l = cfg.c.lasers[k]
            w = l.count * (5 if l.compas else (4 if l.pad_sectors else 1))
            if not (l.out_offset <= col < l.out_offset + l.history * w) or l.compas:
                continue
            i = (col - l.out_offset) % w % l.count
            ang = np.radians(fdir[e] + (l.ray_angles[i % 8] if l.explicit_angles else l.angle_offset + i * 360.0 / l.count))
            d = np.array([np.cos(ang), np.sin(ang)])
            rects = [ri[e].reshape(-1, 4), sr[e]]
            if st is not None:
                rects.append(st[ei[e, abi.EI_SCEN]])
            r = np.concatenate(rects).astype(np.float64)
            cx = np.concatenate([r[:, 0], r[:, 0] + r[:, 2], r[:, 0], r[:, 0] + r[:, 2]]) - pos[e, 0]
            cy = np.concatenate([r[:, 1], r[:, 1], r[:, 1] + r[:, 3], r[:, 1] + r[:, 3]]) - pos[e, 1]
            along = cx * d[0] + cy * d[1]; across = np.abs(cx * d[1] - cy * d[0])
            if np.any((across < 1e-6) & (along > 0) & (along < l.length + 1)):
                out[e, col] = True
    return out


# Budget of the knife-edge waivers: every ray reading compared with the oracle and every one excused as a corner
# graze is counted over the whole test session; the running ratio is asserted after every comparison and reported at the end of the
# session (tests/test_gpu_fuzz.py::test_zz_waiver_budget).  A graze shows up in up to max_prev_obs rows while its snapshot ages, so the
# bound has a constant part of two such events.
WAIVERS = dict(readings=0, corner=0, radar_env_steps=0, env_steps=0, radar_worst=0.0,
               lasers_not_bit_identical=0, num_compared=0, num_not_bit_identical=0,     # float32 outputs within the tolerance but not equal bit for bit
               config_space_radar=0, config_space_steps=0)      # tests/test_gpu_config_space_golden.py: radar blocks waived / steps compared with the reference's records
CORNER_BUDGET = 1e-6


def _compare_with_oracle(env, ora, cfg, tag):
    num = env.obs_num.cpu().numpy(); las = env.lasers.cpu().numpy()
    assert np.array_equal(env.done.cpu().numpy(), ora.done), (tag, "done")
    assert np.array_equal(env.status.cpu().numpy(), ora.status), (tag, "status")
    assert np.abs(env.reward.cpu().numpy() - ora.reward).max() <= 1e-5, (tag, "reward")
    assert close(num, ora.obs_num).all(), (tag, "num", np.abs(num - ora.obs_num).max())
    assert np.array_equal(env.target.cpu().numpy(), ora.target), (tag, "target")
    L = cfg.lasers_len
    bad = ~close(las[:, :L], ora.lasers[:, :L])
    WAIVERS["readings"] += int(sum(l.history * l.width for l in cfg.lasers)) * env.n
    WAIVERS["lasers_not_bit_identical"] += int((las[:, :L] != ora.lasers[:, :L]).sum())
    WAIVERS["num_compared"] += num.size; WAIVERS["num_not_bit_identical"] += int((num != ora.obs_num).sum())
    if bad.any():
        graze = _corner_grazes(env, cfg, bad)
        WAIVERS["corner"] += int((bad & graze).sum())
        bad &= ~graze
    assert not bad.any(), (tag, "lasers", np.argwhere(bad)[:5], np.abs(las[:, :L] - ora.lasers[:, :L]).max())
    assert WAIVERS["corner"] <= CORNER_BUDGET * WAIVERS["readings"] + 2 * abi.FTL_MAX_LASERS * 12, (tag, "corner-graze waivers over budget", WAIVERS)
    ri = env.state_field("rb_int").cpu().numpy().reshape(env.n, cfg.n_robots, abi.RI_COUNT)
    assert np.array_equal(ri[:, :, :6], ora.robot_ints()), (tag, "hitboxes")


@pytest.mark.parametrize("policy", ["random", "mixed"])
def test_config_D_matches_oracle_batch(policy):
    """256 envs x 60 steps of config D (102 static rects, 180 rays): every output of every env and step against the oracle."""
    n, steps = 256, 60
    cfg, pool = _cfg_pool("D_s2_chase", 192)
    assert cfg.c.n_static == 102 and cfg.lasers[0].count == 180
    env = _vec(n, cfg, pool)
    scen = pool_scenarios(pool)
    idx = np.arange(n) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n)
    ora.reset(scen, idx)
    _compare_with_oracle(env, ora, cfg, ("reset",))
    for t in range(steps):
        a = _actions(cfg, n, t, policy, seed=3)
        env.step(torch.tensor(a, dtype=torch.float64, device="cuda:0"))
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, (policy, t))
    assert env.error_report() == (0, 0)
    env.close()


@pytest.mark.parametrize("ep", ["C_s1_chase", "L_s2_chase", "T_s3_chase"])
def test_f3_sensors_match_oracle_batch(ep):
    """Row f3: LeaderCorridor_lasers_compas (config C), LaserSensor + LeaderTrackDetector_vector / _radar (L), the v1 tracker with
    detectors and lenient ray sensors (T) on 192 envs x 50 steps with explicit resets of finished envs -- every output block."""
    n, steps = 192, 50
    cfg, pool = _cfg_pool(ep, 96)
    env = _vec(n, cfg, pool)
    scen = pool_scenarios(pool)
    idx = np.arange(n) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n)
    ora.reset(scen, idx)
    _compare_with_oracle(env, ora, cfg, (ep, "reset"))
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=13)
        env.step(torch.tensor(a, dtype=torch.float64, device="cuda:0"))
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, (ep, t))
        d = ora.done.astype(bool)
        if d.any() and t % 10 == 9:                 # masked reset of the finished envs to their next scenario on both sides
            idx = np.where(d, (idx + n) % pool.n, idx)
            env.reset(torch.from_numpy(idx.astype(np.int32)), mask=torch.from_numpy(d.astype(np.uint8)))
            ora.reset(scen, idx, mask=d)
            _compare_with_oracle(env, ora, cfg, (ep, t, "masked reset"))
    assert env.error_report() == (0, 0)
    env.close()


def _full_size_properties(cfg, pool, N, n_small, steps, frames_fixed):
    """Batch-composition independence, domain invariants and determinism at a BASELINE batch size."""
    big, small = _vec(N, cfg, pool), _vec(n_small, cfg, pool)
    sel = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:n_small].sort().values
    idx_big = torch.arange(N, dtype=torch.int64) % pool.n
    big.reset(idx_big.to(torch.int32))
    # (per-env random streams are keyed by the env index: the small batch can only mirror envs whose results do not
    #  depend on them -- configs without regimes; with regimes the comparison is skipped and determinism carries the check)
    streams = cfg.c.n_speed_regime >= 0 or cfg.c.rand_fps_hi > 0
    if not streams:
        small.reset(idx_big[sel].to(torch.int32))
    first = {}
    for t in range(steps):
        act = torch.tensor(_actions(cfg, N, t, seed=11), dtype=torch.float64, device="cuda:0")
        big.step(act)
        if not streams:
            small.step(act[sel.cuda()].contiguous())
            s = sel.cuda()
            assert torch.equal(big.obs_num[s], small.obs_num) and torch.equal(big.lasers[s], small.lasers), t
            assert torch.equal(big.reward[s], small.reward) and torch.equal(big.done[s], small.done) and torch.equal(big.status[s], small.status)
        first[t] = (big.obs_num.clone(), big.lasers.clone(), big.reward.clone(), big.done.clone())
    Lmax = torch.cat([torch.full((l.history * l.width,), l.length) for l in cfg.lasers]).cuda()
    assert bool((big.lasers >= 0).all()) and bool((big.lasers <= Lmax * (1 + 1e-6)).all())
    R = cfg.n_robots
    pos = big.state_field("rb_pos").view(N, R, 2).double()
    ri = big.state_field("rb_int").view(N, R, abi.RI_COUNT)
    centre = torch.stack([ri[..., 0] + (ri[..., 2] >> 1), ri[..., 1] + (ri[..., 3] >> 1)], -1).double()
    assert float((pos - centre).abs().max()) < 1.0          # |position - rect.center| < 1
    ei = big.state_field("env_int")
    if frames_fixed:
        assert bool((ei[:, abi.EI_STEP_COUNT] == steps * cfg.c.frames_per_step).all())
    init_len = pool.t["init_traj_len"][idx_big.cuda()]
    assert torch.equal(ei[:, abi.EI_TRAJ_LEN].long(), init_len.long() + ei[:, abi.EI_STEP_COUNT].long() // 5)
    assert big.error_report() == (0, 0)
    # a ray that hits something reads less than its length: with 100 rocks / in-corridor rays that must happen somewhere
    assert bool((big.lasers < Lmax * 0.999).any())
    # determinism: a fresh handle (the per-env random streams are keyed by the reset count, so a second reset() of the same
    # handle legitimately draws other numbers) replays the run bit for bit
    big.close(); small.close()
    again = _vec(N, cfg, pool)
    again.reset(idx_big.to(torch.int32))
    for t in range(steps):
        again.step(torch.tensor(_actions(cfg, N, t, seed=11), dtype=torch.float64, device="cuda:0"))
        o, l, r, d = first[t]
        assert torch.equal(again.obs_num, o) and torch.equal(again.lasers, l) and torch.equal(again.reward, r) and torch.equal(again.done, d), t
    again.close()


def test_config_D_full_size_properties_4096_envs():
    cfg, pool = _cfg_pool("D_s2_chase", 192)
    _full_size_properties(cfg, pool, 4096, 512, 12, True)


def test_config_E_full_size_properties_32768_envs():
    cfg, pool = _cfg_pool("E_s3_chase", 512, rng_seed=9)
    _full_size_properties(cfg, pool, 32768, 1024, 12, True)


def test_config_E_matches_oracle_batch_1024_envs():
    """Config E on a batch of distinct env ids (per-env regime streams), 2 bears, negative follower speed."""
    n, steps = 1024, 40
    cfg, pool = _cfg_pool("E_s3_chase", 512, rng_seed=9, env_id_base=5000)
    env = _vec(n, cfg, pool)
    scen = pool_scenarios(pool)
    idx = np.arange(n) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n, env_id_base=5000)
    ora.reset(scen, idx)
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed", seed=5)
        a[3::7, 0] = -0.5 * cfg.c.follower.max_speed          # negative_speed=True in this config
        env.step(torch.tensor(a, dtype=torch.float64, device="cuda:0"))
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, ("E", t))
    env.close()


def test_unstaged_corridor_window_matches_oracle(monkeypatch):
    """The ray kernel keeps a float32 copy of at most 128 corridor points in LDS; a longer window of the snapshots (a leader crawling
    under a speed regime) is read from the tracker's ring in place.  FTL_DEBUG_CORR_LDS_CAP=8 makes every window too long: config E,
    300 envs x 45 steps against the oracle through that path."""
    n, steps = 300, 45
    cfg, pool = _cfg_pool("E_s3_chase", 512, rng_seed=9, env_id_base=9000)
    monkeypatch.setenv("FTL_DEBUG_CORR_LDS_CAP", "8")
    env = _vec(n, cfg, pool)
    monkeypatch.delenv("FTL_DEBUG_CORR_LDS_CAP")
    scen = pool_scenarios(pool)
    idx = (np.arange(n) * 5) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n, env_id_base=9000)
    ora.reset(scen, idx)
    _compare_with_oracle(env, ora, cfg, ("unstaged", "reset"))
    for t in range(steps):
        a = _actions(cfg, n, t, "mixed" if t % 2 else "random", seed=21)
        env.step(torch.tensor(a, dtype=torch.float64, device="cuda:0"))
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, ("unstaged", t))
    env.close()


# ---- the two-stream split path (ftl_abi.hip launch(): FTL_SPLIT, rays kernels <*, *, true>) ----------------------------------
def _two(monkeypatch, n, cfg, pool, **kw):
    monkeypatch.setenv("FTL_SPLIT", "1")
    a = _vec(n, cfg, pool, **kw)
    monkeypatch.setenv("FTL_SPLIT", "0")
    b = _vec(n, cfg, pool, **kw)
    monkeypatch.delenv("FTL_SPLIT")
    return a, b


def test_split_path_never_changes_a_result(monkeypatch):
    """Config F at 8192+37 envs: FTL_SPLIT=1 (two interleaved halves of the slot groups on two streams) against
    FTL_SPLIT=0, 32 steps with auto-reset plus a masked reset in the middle -- bit-identical outputs and state."""
    n = 8192 + 37
    cfg, pool = _cfg_pool("F_s7_chase", 256, rng_seed=4)
    a, b = _two(monkeypatch, n, cfg, pool, policy_obs=True)
    idx = torch.arange(n, dtype=torch.int32) % pool.n
    a.reset(idx); b.reset(idx)
    fields = ["rb_pos", "rb_dbl", "rb_int", "env_int", "env_dbl", "traj", "hist", "corr", "traj_bb", "ep_stats"]
    outs = ("obs_num", "lasers", "target", "reward", "done", "status", "policy_obs")
    for t in range(32):
        act = torch.tensor(_actions(cfg, n, t, seed=2), dtype=torch.float64, device="cuda:0")
        a.step(act, auto_reset=True); b.step(act, auto_reset=True)
        for name in outs:
            assert torch.equal(getattr(a, name), getattr(b, name)), (t, name)
        if t == 15:
            mask = (torch.arange(n) % 5 == 0).to(torch.uint8)
            a.reset((idx + 7) % pool.n, mask=mask); b.reset((idx + 7) % pool.n, mask=mask)
            for name in outs:
                assert torch.equal(getattr(a, name), getattr(b, name)), ("masked reset", name)
        if t % 8 == 7:
            for f in fields:
                assert torch.equal(a.state_field(f), b.state_field(f)), (t, f)
    assert torch.equal(a.episode_metrics(), b.episode_metrics())
    a.close(); b.close()


@pytest.mark.parametrize("ep,over,want", [
    ("F_s7_chase", {}, "<10, false, true>"),                 # the shipped training config: H = 10
    ("Bpad_s4_chase", {}, "<5, true, true>"),                # pad_sectors, H = 5
    ("Bpad_s4_chase", {"max_prev_obs": 7}, "<12, true, true>"),   # pad_sectors with H = 7 -> the FTL_HMAX instantiation
])
def test_split_path_matches_oracle_at_8192_envs(monkeypatch, ep, over, want):
    """Each ray-kernel instantiation of the two-stream mode runs at least once against the oracle, at a batch size where the
    split is actually taken (>= 8192 envs)."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    n, steps = 8192, 5
    z, meta = load_episode(ep)
    meta = dict(meta)
    if over:
        kw = dict(meta["kwargs"]); sens = {k: dict(v) for k, v in kw["follower_sensors"].items()}
        for v in sens.values():
            if "max_prev_obs" in v:
                v["max_prev_obs"] = over["max_prev_obs"]
        kw["follower_sensors"] = sens; meta["kwargs"] = kw
    cfg = config_for(meta, scen_route_len=256, rng_seed=6, env_id_base=300)
    pool = ScenarioPool.generate(cfg, np.arange(160), "cuda:0")
    monkeypatch.setenv("FTL_SPLIT", "1")
    env = _vec(n, cfg, pool)
    monkeypatch.delenv("FTL_SPLIT")
    scen = pool_scenarios(pool)
    idx = np.arange(n) % pool.n
    env.reset(torch.from_numpy(idx.astype(np.int32)))
    ora = OracleBatch(cfg, n, env_id_base=300)
    ora.reset(scen, idx)
    _compare_with_oracle(env, ora, cfg, (want, "reset"))
    for t in range(steps):
        a = _actions(cfg, n, t, seed=8)
        env.step(torch.tensor(a, dtype=torch.float64, device="cuda:0"))
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, (want, t))
    env.close()
