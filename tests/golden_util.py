"""Helpers shared by the parity tests: load the golden episodes emitted by the reference
(tests/golden/gen/make_golden.py) and rebuild the matching config."""
import glob
import json
import os

import numpy as np

from continiousenvironment_follower_leader_amd import make_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fuzz_seeds():
    """Seeds of the recorded configs of tests/fuzz_configs.py (fuzz_s{seed}.npz; deliberately not episode_*.npz)."""
    return sorted(int(os.path.basename(p)[len("fuzz_s"):-4]) for p in glob.glob(os.path.join(GOLDEN, "fuzz_s*.npz")))


def load_fuzz(seed):
    z = np.load(os.path.join(GOLDEN, "fuzz_s%03d.npz" % seed))
    return z, json.loads(str(z["meta"]))


def episode_names():
    return sorted(os.path.basename(p)[len("episode_"):-4] for p in glob.glob(os.path.join(GOLDEN, "episode_*.npz")))


def load_episode(name):
    z = np.load(os.path.join(GOLDEN, "episode_%s.npz" % name))
    meta = json.loads(str(z["meta"]))
    return z, meta


def config_for(meta, scen_route_len=None, **over):
    kw = dict(meta["kwargs"])
    sensors = kw.get("follower_sensors")
    if sensors and meta.get("post"):
        # config D: the generator sets lasers_count on the constructed sensor; mirror it here
        for sname, attrs in meta["post"].items():
            sensors[sname] = dict(sensors[sname])
            if "lasers_count" in attrs:
                sensors[sname]["lasers_count"] = attrs["lasers_count"]
                sensors[sname]["_allow_any_lasers_count"] = True
    if scen_route_len is not None:
        kw["route_cap"] = max(128, int(scen_route_len))
    kw.update(over)
    return make_config(**kw)


def scenario_arrays(z):
    return dict(static_rects=z["scen:static_rects"], robot_pos=z["scen:robot_pos"],
                robot_dir=z["scen:robot_f64"][:, 0], robot_rect=z["scen:robot_i32"][:, :4],
                route=z["scen:route"], init_traj=z["scen:init_traj"])


# ---- the LeaderTrackDetector_radar knife edge: the one arithmetic behind every use of that waiver ----------------
RADAR_BUDGET = 0.01      # env-steps per config with a radar reading excused as a sector-boundary knife edge (worst of the 96 configs: 0.26 %; all of them together 6e-5)


def radar_slice(n, detectable, seq_len):
    """[s0, s1) of the n tracked points that a radar with detectable_positions new (0) / old (1) / near (2) looks at."""
    s0, s1 = 0, n
    if detectable == 0: s0 = max(n - seq_len, 0)
    elif detectable == 1: s1 = min(n, seq_len)
    return s0, s1


def radar_touches_boundary(p, pos, fdir, sectors):
    """True when one of the points `p` [k, 2] lies within 1e-6 of a sector width of a sector boundary, seen from a follower at `pos`
    heading `fdir` degrees (SEN:423-476: the angle to the right-hand vector, `ar >= sa * t and ar < sa * (t + 1)` on arccos values)."""
    sa = np.pi / sectors
    v = p - pos
    r = np.radians((fdir + 90.0) % 360.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.arccos(np.clip((v[:, 0] * np.cos(r) + v[:, 1] * np.sin(r)) / np.hypot(v[:, 0], v[:, 1]), -1, 1)) / sa
    return bool(np.any(np.abs(q - np.rint(q)) < 1e-6))


# tolerance of BASELINE.json north_star: 1e-5 for float positions / sensor readings / reward.
# Observations are float32: for |x| >= 128 one f32 ulp already exceeds 1e-5, so the check is
# "1e-5 absolute OR one float32 ulp" (hard part 3).
def close(a, b, atol=1e-5):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.abs(a - b) <= np.maximum(atol, ulp)


def radar_waived(z, tag, t, a):
    """The knife-edge criterion of tests/test_gpu_fuzz.py::_radar_knife_edges for radar `a` (an abi aux entry) at reset (`t` None) or step
    `t` of record `z`, evaluated on the state the REFERENCE recorded there (follower pose and tracker history), never on the state of the
    code under test.  (A radar ahead of the tracker in dict order saw the history before the step's second tracker scan, which differs from
    the recorded one by the point that scan may have appended or dropped; the recorded one is the one there is.)"""
    pre = "reset_dbg:" if t is None else "dbg:"
    get = (lambda k: z[pre + k]) if t is None else (lambda k: z[pre + k][t])
    n = int(get("trk")[1])
    s0, s1 = radar_slice(n, a.detectable, a.seq_len)
    if s1 <= s0:
        return False
    return radar_touches_boundary(get("hist")[:n][s0:s1], get("robot_pos")[1].astype(np.float64), get("robot_f64")[1, 0], a.radar_sectors)


def check_oracle_episode(name, z, meta, cfg, env, n_steps=None, radar_waivers=None):
    """Replays record `z` on the oracle env `env` (fresh, not yet reset) and checks every observable of reset() and of the first `n_steps`
    steps (default: all), plus the internal state the generator dumped, against it -- the checks of
    tests/test_oracle_golden.py::test_oracle_matches_reference_episode.  `radar_waivers`: None, or a list that collects (tag, t, name) of
    the LeaderTrackDetector_radar blocks that differ from the record on a proven knife edge (radar_waived); any other difference fails.
    Returns the number of compared steps (reset included)."""
    from continiousenvironment_follower_leader_amd import abi
    obs = env.reset(**scenario_arrays(z))
    lnames = meta["laser_names"]

    def check_obs(tag, t, obs):
        ref = z[tag + ":num"] if t is None else z[tag + ":num"][t]
        assert close(obs["num"], ref).all(), (name, t, "num", obs["num"] - ref)
        for ln in lnames:
            ref = z[tag + ":laser:" + ln] if t is None else z[tag + ":laser:" + ln][t]
            assert obs[ln].shape == ref.shape
            assert close(obs[ln], ref).all(), (name, t, ln, np.abs(obs[ln] - ref).max())
        for j, a in enumerate(cfg.aux):                      # LaserSensor / LeaderTrackDetector_vector / _radar (float32 arrays)
            ref = z[tag + ":aux:" + a.name] if t is None else z[tag + ":aux:" + a.name][t]
            assert obs[a.name].shape == ref.shape, (name, a.name, obs[a.name].shape, ref.shape)
            ok = close(obs[a.name], ref).all()
            if not ok and radar_waivers is not None and a.kind == abi.AUX_TRACK_RADAR and radar_waived(z, tag, t, cfg.c.aux[j]):
                radar_waivers.append((tag, t, a.name))
                continue
            assert ok, (name, t, a.name, np.abs(obs[a.name] - ref).max(), np.argwhere(~close(obs[a.name], ref))[:4])

    check_obs("reset", None, obs)
    assert np.array_equal(obs["target"], z["reset:target"])
    for t in range(len(z["actions"]) if n_steps is None else n_steps):
        obs, rew, done, st = env.step(z["actions"][t])
        check_obs("obs", t, obs)
        assert abs(rew - z["reward"][t]) <= 1e-5, (name, t, rew, z["reward"][t])
        assert done == bool(z["done"][t]), (name, t)
        assert tuple(st) == tuple(z["info"][t]), (name, t, st, z["info"][t])
        assert np.array_equal(obs["target"], z["obs:target"][t]), (name, t)
        d = env.debug()
        assert np.array_equal(d["counters"][:11], z["dbg:counters"][t]), (name, t, d["counters"][:11], z["dbg:counters"][t])
        assert np.array_equal(d["robot_i32"], z["dbg:robot_i32"][t]), (name, t, "hitboxes")
        assert close(d["robot_pos"], z["dbg:robot_pos"][t]).all(), (name, t)
        assert np.allclose(d["robot_f64"], z["dbg:robot_f64"][t], rtol=0, atol=1e-9), (name, t)
        assert abs(d["acc"] - z["dbg:acc"][t]).max() <= 1e-9
        if "dbg:trk" in z:
            tr = z["dbg:trk"][t]
            assert tuple(tr) == tuple(d["counters"][11:14]), (name, t, tr, d["counters"][11:14])
            assert np.allclose(d["hist"], z["dbg:hist"][t][:int(tr[1])], rtol=0, atol=1e-9)
            assert np.allclose(d["corr"], z["dbg:corr"][t][:int(tr[2])], rtol=0, atol=1e-9)
            assert np.array_equal(d["hist_isf64"], z["dbg:hist_isf64"][t][:int(tr[1])])
        if "dbg:dyn_index" in z:
            nb = z["dbg:dyn_index"].shape[1]
            assert np.array_equal(d["counters"][15:15 + nb], z["dbg:dyn_index"][t])
        assert d["counters"][14] == 0, "oracle raised an error flag"
    return 1 + (len(z["actions"]) if n_steps is None else n_steps)
