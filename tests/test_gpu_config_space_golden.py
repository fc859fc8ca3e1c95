"""The HIP path against the reference's own records of the config space that tests/test_gpu_fuzz.py draws from.

tests/test_gpu_fuzz.py compares the kernels with the oracle on 96 drawn configs; tests/test_oracle_fuzz_golden.py pins the oracle to
records of the unmodified reference on the same configs (tests/golden/fuzz_s{seed}.npz).  This file closes the triangle: the kernels
replay those records directly, as tests/test_gpu_parity.py::test_hip_matches_reference_episode replays the named ones -- the same
assertions, plus a zero error word for every episode that ran, and the matching FTL_ERR_* bit at the reset or step where the reference
raised.  It reads tests/golden/ only.  (The name sorts before test_gpu_configs.py, so the waiver counts reach test_zz_waiver_budget.)"""
import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import abi
from golden_util import RADAR_BUDGET, close, fuzz_seeds, load_fuzz, radar_waived, scenario_arrays
from test_gpu_configs import WAIVERS
from test_gpu_parity import _robots, _vec
from test_oracle_fuzz_golden import NO_EDGES, RAISE_SITES, fuzz_config

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["4 lanes per env", "8 lanes per env"])
def lanes_per_env(request, monkeypatch):
    """Both forms of the frame kernel (FTL_DEBUG_G8 at ftl_create, as tests/test_gpu_parity.py)."""
    monkeypatch.setenv("FTL_DEBUG_G8", "0" if request.param.startswith("4") else "1")


@pytest.mark.parametrize("seed", fuzz_seeds())
def test_hip_matches_reference_on_fuzz_config(seed, lanes_per_env):
    z, meta = load_fuzz(seed)
    name = "fuzz_s%03d" % seed
    cfg, warned = fuzz_config(z, meta)
    raised = meta.get("raised")
    scen = scenario_arrays(z)
    n = 3   # the same episode in three envs: exercises multi-workgroup launches and env indexing
    env = _vec(cfg, n, [scen])
    env.reset(torch.zeros(n, dtype=torch.int32))
    torch.cuda.synchronize()
    lnames = meta["laser_names"]
    # a random speed regime / random_frames_per_step draws from the per-env counter stream (env id in the key): only env 0 replays the episode
    rnd = any(cfg.c.speed_is_range[i] for i in range(max(cfg.c.n_speed_regime, 0))) or cfg.c.rand_fps_hi > 0 \
        or (cfg.c.n_bears > 5 and cfg.c.move_bear_v4)
    envs = [0] if rnd else list(range(n))
    last = envs[-1]
    waived = [0]

    def errors():
        return env.state_field("env_int").cpu().numpy()[envs, abi.EI_ERROR]

    def check(tag, t):
        num = env.obs_num.cpu().numpy()
        ref = z[tag + ":num"] if t is None else z[tag + ":num"][t]
        for e in envs:
            assert close(num[e], ref).all(), (name, t, e, "num", num[e] - ref)
        for ln in lnames:
            got = env.laser_view(ln).cpu().numpy()
            ref = z[tag + ":laser:" + ln] if t is None else z[tag + ":laser:" + ln][t]
            assert got.shape[1:] == ref.shape
            for e in envs:
                assert close(got[e], ref).all(), (name, t, e, ln, np.abs(got[e] - ref).max())
        edge = False
        for j, a in enumerate(cfg.aux):             # LaserSensor / LeaderTrackDetector_vector / _radar
            got = env.aux_view(a.name).cpu().numpy()
            ref = z[tag + ":aux:" + a.name] if t is None else z[tag + ":aux:" + a.name][t]
            assert got.shape[1:] == ref.shape, (a.name, got.shape, ref.shape)
            for e in envs:
                ok = close(got[e], ref).all()
                # the one waiver: a radar block on a sector-boundary knife edge of the REFERENCE's recorded state
                if not ok and a.kind == abi.AUX_TRACK_RADAR and radar_waived(z, tag, t, cfg.c.aux[j]):
                    edge = True
                    continue
                assert ok, (name, t, e, a.name, np.abs(got[e] - ref).max())
        waived[0] += int(edge)
        for fname, _k in cfg.follower_info:
            fref = z[tag + ":finfo:" + fname] if t is None else z[tag + ":finfo:" + fname][t]
            got = env.follower_info(fname).cpu().numpy()
            for e in envs:
                assert np.array_equal(got[e], fref), (fname, t, e, got[e], fref)
        reft = z[tag + ":target"] if t is None else z[tag + ":target"][t]
        assert np.array_equal(env.target.cpu().numpy()[0], reft), (name, t, "target")

    def step(action):
        env.step(torch.tensor(np.tile(np.asarray(action, np.float64), (n, 1)), dtype=torch.float64, device="cuda:0"))

    def finish(steps):
        WAIVERS["config_space_radar"] += waived[0]; WAIVERS["config_space_steps"] += steps
        env.close()

    site = None if raised is None else (raised["file"], raised["line"])
    if raised is not None:
        assert site in RAISE_SITES, (name, "the reference raises where this project has neither an error bit nor a warning", raised)
    if raised is not None and raised["phase"] == "reset":
        n_steps = 0
    else:
        assert (errors() == 0).all(), (name, "reset", errors())
        check("reset", None)
        n_steps = len(z["actions"]) if raised is None else raised["step"]
    for t in range(n_steps):
        step(z["actions"][t])
        check("obs", t)
        rew = env.reward.cpu().numpy(); done = env.done.cpu().numpy(); st = env.status.cpu().numpy()
        for e in envs:
            assert abs(rew[e] - z["reward"][t]) <= 1e-5, (name, t, rew[e], z["reward"][t])
            assert bool(done[e]) == bool(z["done"][t]), (name, t, "done")
            assert tuple(st[e]) == tuple(z["info"][t]), (name, t, st[e], z["info"][t])
        # internal state against the reference's own objects
        pos, dbl, ints = _robots(env, last)
        assert np.array_equal(ints[:, :6], z["dbg:robot_i32"][t]), (name, t, "hitboxes / rotation dirs", ints[:, :6], z["dbg:robot_i32"][t])
        assert close(pos, z["dbg:robot_pos"][t]).all(), (name, t, "positions")
        assert np.allclose(dbl, z["dbg:robot_f64"][t], rtol=0, atol=1e-9), (name, t, "controller state")
        ei = env.state_field("env_int")[last].cpu().numpy()
        cnt = z["dbg:counters"][t]
        got = [ei[abi.EI_STEP_COUNT], ei[abi.EI_TRAJ_LEN], ei[abi.EI_GREEN_COUNT], ei[abi.EI_TARGET_ID], ei[abi.EI_LEADER_FINISHED],
               ei[abi.EI_IN_BOX], ei[abi.EI_ON_TRACE], ei[abi.EI_TOO_CLOSE], ei[abi.EI_CRASH], ei[abi.EI_DONE], ei[abi.EI_FINISH_TIMER]]
        assert list(cnt) == [int(v) for v in got], (name, t, "counters", cnt, got)
        assert (errors() == 0).all(), (name, t, errors())
        if "dbg:trk" in z:
            tr = z["dbg:trk"][t]
            n_hist = ei[abi.EI_HIST1_LEN] if cfg.c.has_tracker == 1 else ei[abi.EI_CORR_HI] - ei[abi.EI_CORR_LO]
            assert int(tr[0]) == ei[abi.EI_TRK_COUNTER] and int(tr[1]) == n_hist and int(tr[2]) == ei[abi.EI_CORR_HI] - ei[abi.EI_CORR_LO], (name, t, tr, ei)
            hist, corr = env.tracker_obs(last)
            assert np.allclose(hist, z["dbg:hist"][t][:int(tr[1])], rtol=0, atol=1e-9), (name, t, "tracker history")
            assert np.allclose(corr.reshape(-1, 4), z["dbg:corr"][t][:int(tr[2])], rtol=0, atol=1e-9), (name, t, "corridor")
        if "dbg:dyn_index" in z:
            nb = z["dbg:dyn_index"].shape[1]
            assert np.array_equal(ei[abi.EI_DYN_INDEX0:abi.EI_DYN_INDEX0 + nb], z["dbg:dyn_index"][t])
    if raised is None:
        assert not any(NO_EDGES in m for m in warned), (name, warned)
        if not rnd:
            assert env.error_report() == (0, 0), (name, env.error_report())
        return finish(1 + n_steps)
    # ---- the reset or step at which the reference raised ----
    if raised["phase"] == "step":
        step(raised["action"])
    kind, what = RAISE_SITES[site]
    rep = env.error_report()
    if kind == "bit":
        assert (errors() & what != 0).all(), (name, raised, errors())
        assert rep[0] >= len(envs) and rep[1] & what, (name, raised, rep)
    else:               # decidable from the config: make_config warned, the device sets no bit and reads laser_length on the edgeless sensors
        assert any(what in m for m in warned), (name, raised, warned)
        assert (errors() == 0).all() and (rnd or rep == (0, 0)), (name, raised, errors(), rep)
        edgeless = [l for l in cfg.lasers if not l.react_corridor and not l.react_green
                    and (l.react_obstacles == 0 or (l.react_obstacles == 3 and cfg.c.n_bears == 0))]
        assert edgeless
        for l in edgeless:
            got = env.laser_view(l.name).cpu().numpy()[envs]
            got = got[got != 0] if l.pad_sectors else got                                    # (pad_sectors: zeros outside a ray's sector)
            assert got.size and (got == np.float32(l.length)).all(), (name, l.name)
    finish(n_steps)


def test_zz_config_space_radar_budget():
    """The radar knife edge is the only waiver of this file, judged on the reference's recorded state; every use is counted
    (config_space_radar of config_space_steps in the file test_zz_waiver_budget writes) and all of them together stay within RADAR_BUDGET."""
    print("config space golden, HIP: %d radar blocks waived in %d compared steps" % (WAIVERS["config_space_radar"], WAIVERS["config_space_steps"]))
    assert WAIVERS["config_space_steps"] > 0
    assert WAIVERS["config_space_radar"] <= RADAR_BUDGET * WAIVERS["config_space_steps"], WAIVERS
