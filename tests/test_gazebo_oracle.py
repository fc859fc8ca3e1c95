"""Row f4 on the CPU: the oracle's follower-relative tracker / ray sensors (oracle/ftl_oracle_gazebo.c) against the vectors the
UNMODIFIED reference classes of gazebo_tracker.py produced (tests/golden/gen/make_golden_gazebo.py)."""
import glob
import json
import os

import numpy as np
import pytest

from continiousenvironment_follower_leader_amd.gazebo import make_gz_config
from golden_util import GOLDEN, close
from oracle import OracleGazebo

NAMES = sorted(os.path.basename(p)[len("gazebo_"):-4] for p in glob.glob(os.path.join(GOLDEN, "gazebo_*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN, "gazebo_%s.npz" % name))
    return z, json.loads(str(z["meta"]))


@pytest.mark.parametrize("name", NAMES)
def test_gazebo_oracle_matches_reference(name):
    z, meta = load(name)
    cfg = make_gz_config(meta["lasers"], meta["max_pts"])
    o = OracleGazebo(cfg)
    o.reset()
    off = 0
    blocks = []
    for k, kw in enumerate(meta["lasers"]):
        w = kw["lasers_count"] * (4 if kw["pad_sectors"] else 1)
        blocks.append((off, kw["max_prev_obs"], w)); off += kw["max_prev_obs"] * w
    for t in range(meta["steps"]):
        n = int(z["n_pts"][t])
        if "reset" in z.files and z["reset"][t]:      # the scenario reset the tracker and the sensors before this call
            o.reset()
        las = o.step(z["leader"][t], z["yaw"][t], z["delta"][t], z["pts1"][t][:n], z["pts2"][t][:n])
        st = o.state()
        assert st["error"] == 0
        assert st["counter"] == int(z["counter"][t]) and len(st["hist"]) == int(z["n_hist"][t]) and len(st["corr"]) == int(z["n_corr"][t]), (name, t)
        assert np.allclose(st["hist"], z["hist"][t][:len(st["hist"])], rtol=0, atol=1e-12), (name, t, "history")
        # (equal_nan: ten identical seed points make a corridor of 0 / 0 in the reference too, fixture seed_line)
        assert np.allclose(st["corr"], z["corr"][t][:len(st["corr"])], rtol=0, atol=1e-9, equal_nan=True), (name, t, "corridor")
        for k, (b, h, w) in enumerate(blocks):
            got = las[b:b + h * w].reshape(h, w)
            ref = z["laser%d" % k][t]
            assert got.shape == ref.shape
            assert close(got, ref).all(), (name, t, k, np.abs(got - ref).max())


def test_gazebo_vectors_are_not_trivial():
    z, meta = load("arctic_s1")
    assert (z["laser0"] < 9.99).mean() > 0.5 and (z["laser1"] < 14.99).mean() > 0.02      # corridor walls and obstacle points are hit
    assert int(z["n_hist"].max()) > 15 and len(set(z["counter"].tolist())) > 20           # appends, trims and skipped scans all occur


def test_gazebo_many_pts_vectors_reach_past_the_lane_stride():
    z, meta = load("many_pts")
    assert meta["max_pts"] > 129 and set(z["n_pts"].tolist()) == {63, 64, 65, 66, 127, 128, 129, meta["max_pts"]}
    # hits among the points beyond index 64: without them the oracle reads something else than the reference recorded
    cfg = make_gz_config(meta["lasers"], meta["max_pts"])
    full, cut = OracleGazebo(cfg), OracleGazebo(cfg)
    full.reset(); cut.reset()
    differ = 0
    for t in range(meta["steps"]):
        n = int(z["n_pts"][t])
        a = full.step(z["leader"][t], z["yaw"][t], z["delta"][t], z["pts1"][t][:n], z["pts2"][t][:n])
        b = cut.step(z["leader"][t], z["yaw"][t], z["delta"][t], z["pts1"][t][:64], z["pts2"][t][:64])
        differ += int(n > 64 and not close(a, b).all())
    assert differ >= int((z["n_pts"] > 64).sum()) // 2


def test_gazebo_few_pts_vectors_have_no_obstacle_segment():
    z, meta = load("few_pts")
    assert z["n_pts"].tolist() == [t % 4 for t in range(meta["steps"])]
    assert not meta["lasers"][1]["react_to_safe_corridor"] and not meta["lasers"][1]["react_to_green_zone"]
    length = meta["lasers"][1]["laser_length"]
    few = np.nonzero(z["n_pts"] < 2)[0]
    assert (z["laser1"][few[0]] == length).all()                          # the whole block, before any snapshot has a segment
    assert all((z["laser1"][t][-1] == length).all() for t in few)         # the newest row of every such call ...
    assert any((z["laser1"][t][:-1] < length * 0.999).any() for t in few)  # ... while older rows of the same block still see their segments
    assert (z["laser1"][z["n_pts"] >= 2][:, -1] < length * 0.999).any()


def test_gazebo_seed_line_vectors_have_zero_linspace_steps():
    z, meta = load("seed_line")
    first = np.nonzero(z["counter"] == 1)[0]
    assert len(first) == 2 and z["reset"].tolist() == [t == first[1] for t in range(meta["steps"])]
    assert (z["yaw"] == np.pi).all() and z["leader"][first].tolist() == [[7.0, 0.0], [10.0, 0.0]]
    assert (z["hist"][first[0]][:10, 1] == 0).all() and len(set(z["hist"][first[0]][:10, 0].tolist())) == 10      # zero step on y
    assert (z["hist"][first[1]][:10] == [10.0, 0.0]).all()                                                         # zero step on both axes


def test_gazebo_jump_vectors_trim_several_points_and_part_the_lengths():
    z, meta = load("jump")
    assert (np.diff(z["n_hist"]) <= -3).any() and (np.diff(z["n_corr"]) <= -3).any()     # (one point appended, four or more dropped)
    assert (z["n_hist"] != z["n_corr"]).any()


def test_gazebo_out_of_range_vectors_grow_the_corridor_alone():
    z, meta = load("out_of_range")
    assert int(z["n_corr"].max()) >= 50 and int(z["n_corr"].max()) < 64 and (z["n_hist"] == 10).all()
    assert (np.hypot(*z["leader"][1:].T) > 25).all()


# ---- the oracle at its capacity (FTL_GZ_HIST_CAP pairs) and on an empty corridor: the yardstick of the same walks on the device ------
OVERFLOW_CALL = 165      # 10 pairs at call 0, one more at every third call: 64 at call 162, the 65th is due at call 165


def far_leader(t):
    """The walk of fixture out_of_range, of any length: seeded at (7, 0), then 26-40 m away (never appended to the history)."""
    return np.array([7.0, 0.0]) if t == 0 else (26.0 + 14.0 * (t % 7) / 6.0) * np.array([np.cos(0.02 * t), np.sin(0.02 * t)])


FAR_PTS1 = np.array([[6.0, -2.0], [6.1, 2.0], [2.0, 6.0], [0.0, 0.0]])
FAR_PTS2 = FAR_PTS1 + np.array([0.0, 1.0])


def test_gazebo_oracle_corridor_overflow():
    from continiousenvironment_follower_leader_amd import abi
    from continiousenvironment_follower_leader_amd.gazebo import ARCTIC_ENV_LASERS, FTL_GZ_HIST_CAP
    z, meta = load("out_of_range")
    o = OracleGazebo(make_gz_config(ARCTIC_ENV_LASERS, 4))
    o.reset()
    kept = None
    for t in range(200):
        las = o.step(far_leader(t), 0.0, np.zeros(2), FAR_PTS1[:3], FAR_PTS2[:3])
        st = o.state()
        assert np.isfinite(las).all() and (las > 0).all() and (las <= 15).all(), t
        if t < meta["steps"]:                      # the growth rule is the reference's as far as it was recorded
            assert np.allclose(z["leader"][t], far_leader(t), rtol=0, atol=1e-12) and len(st["corr"]) == int(z["n_corr"][t]), t
        if t < OVERFLOW_CALL:
            assert st["error"] == 0 and len(st["corr"]) == min(10 + t // 3, FTL_GZ_HIST_CAP), t
            kept = st
        else:                                      # the 65th pair is refused; nothing stored moves, at that call or after it
            assert st["error"] == abi.FTL_ERR_CORR_OVERFLOW and st["counter"] == t + 1, t
            assert len(st["corr"]) == FTL_GZ_HIST_CAP and np.array_equal(st["corr"], kept["corr"]) and np.array_equal(st["hist"], kept["hist"]), t


def test_gazebo_oracle_empty_corridor():
    from continiousenvironment_follower_leader_amd import abi
    from continiousenvironment_follower_leader_amd.gazebo import ARCTIC_ENV_LASERS
    o = OracleGazebo(make_gz_config(ARCTIC_ENV_LASERS, 4))
    o.reset()
    expect = np.concatenate([np.full(10 * 12, 10.0), np.full(10 * 36, 15.0)]).astype(np.float32)
    for t in range(4):             # 400 m away at the first call: ten seed points 45 m apart, trimmed to one; no pair
        las = o.step([400.0, 0.0], 0.0, [0.3, 0.0], FAR_PTS1[:3], FAR_PTS2[:3])
        st = o.state()
        assert st["error"] == abi.FTL_ERR_EMPTY_CORRIDOR and len(st["hist"]) == 1 and len(st["corr"]) == 0, t
        assert np.array_equal(las, expect), t
    o.reset()
    fresh = OracleGazebo(make_gz_config(ARCTIC_ENV_LASERS, 4))
    fresh.reset()
    for t in range(5):
        a = o.step([7.0 + 0.1 * t, 0.5], 0.1, [0.3, 0.0], FAR_PTS1[:3], FAR_PTS2[:3])
        b = fresh.step([7.0 + 0.1 * t, 0.5], 0.1, [0.3, 0.0], FAR_PTS1[:3], FAR_PTS2[:3])
        assert o.state()["error"] == 0 and np.array_equal(a, b) and (a < 9.99).any(), t
