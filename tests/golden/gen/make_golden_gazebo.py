#!/usr/bin/env python3
"""Golden vectors of the follower-relative ("Gazebo") tracker / ray sensors -- runs ONLY in the build container.

Drives the UNMODIFIED reference classes GazeboLeaderPositionsTracker_v2 and GazeboCorridor_Prev_lasers_v2
(/root/reference/src/arctic_gym/gazebo_utils/gazebo_tracker.py:13-297), constructed as arctic_env.py:62-90 does, on synthetic
follower / leader motion and lidar point pairs, and dumps inputs + outputs per call into tests/golden/gazebo_<name>.npz.

Two accommodations, both on the LIBRARY side of the boundary (the reference file is executed as it is):
  * the module is loaded by file path: `src/arctic_gym/__init__.py` imports ray, which is not installed;
  * numpy >= 2 raises ValueError for `ndarray != []` with unbroadcastable shapes, which the laser's scan() evaluates at
    gazebo_tracker.py:226; numpy 1.x -- what the reference ran on (ray 1.9.5 / torch 1.13 pin it) -- returned the scalar True with a
    DeprecationWarning.  The generator hands the module a numpy whose `array()` yields an ndarray subclass with exactly that legacy
    answer for a comparison with an empty list; every other operation is numpy 2.2's own.  For an array of size 0 -- what
    collect_obstacle_edges returns for fewer than two obstacle points on an obstacles-only sensor -- numpy 1.x compared (0,) with
    (0,) into an empty bool array, whose truth value is False (numpy 2.2 raises there as well): the stand-in answers False, and the
    rays of that snapshot read their end points.

`run()` takes a scripted scenario (a generator of per-call inputs); the scenarios below the default `wander` take the classes to the
edges of the kernel's capacity and inputs.  `python make_golden_gazebo.py [OUT_DIR]` writes every fixture into OUT_DIR (default: tests/golden).
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "standins"))
sys.path.insert(0, "/root/reference")


class _LegacyNe(np.ndarray):
    def __ne__(self, other):
        if isinstance(other, list) and len(other) == 0:
            if self.size == 0:
                return False                 # numpy 1.x: (0,) against (0,) broadcasts to an empty bool array, whose truth value is False
            return True                      # numpy 1.x: "elementwise comparison failed; returning scalar instead"
        return np.ndarray.__ne__(self, other)


def load_reference():
    with contextlib.redirect_stdout(io.StringIO()):
        spec = importlib.util.spec_from_file_location("gazebo_tracker", "/root/reference/src/arctic_gym/gazebo_utils/gazebo_tracker.py")
        gt = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gt)
    legacy = types.ModuleType("numpy_legacy_ne")
    legacy.__dict__.update(np.__dict__)
    legacy.array = lambda *a, **k: np.array(*a, **k).view(_LegacyNe)
    gt.np = legacy
    return gt


LASERS = (dict(sensor_name="LeaderCorridor_Prev_lasers_v2_compas", react_to_green_zone=True, react_to_safe_corridor=True,
               react_to_obstacles=True, lasers_count=12, laser_length=10, max_prev_obs=10, pad_sectors=False),     # arctic_env.py:69-78
          dict(sensor_name="LaserPrevSensor_compas", react_to_green_zone=False, react_to_safe_corridor=False,
               react_to_obstacles=True, lasers_count=36, laser_length=15, max_prev_obs=10, pad_sectors=False))     # arctic_env.py:80-90
LASERS_PAD = (dict(LASERS[0], max_prev_obs=4, pad_sectors=True, lasers_count=20), dict(LASERS[1], max_prev_obs=4, lasers_count=24))


def wander(rng, steps, max_pts):
    """The default scenario: world-frame motion, the follower chases a leader that wanders ahead of it; rocks are fixed world points
    seen by a fake lidar."""
    f = np.array([0.0, 0.0]); fyaw = rng.uniform(-0.5, 0.5)
    lead = f + 7.0 * np.array([np.cos(fyaw), np.sin(fyaw)]); lyaw = fyaw
    rocks = rng.uniform(-25, 60, (40, 2))
    prev_f = f.copy()
    for t in range(steps):
        lyaw += rng.normal(0, 0.08)
        lead = lead + (0.35 if (t // 25) % 3 != 2 else 0.02) * np.array([np.cos(lyaw), np.sin(lyaw)])            # the leader pauses now and then
        want = np.arctan2(lead[1] - f[1], lead[0] - f[0])
        fyaw += np.clip((want - fyaw + np.pi) % (2 * np.pi) - np.pi, -0.12, 0.12)
        gap = np.linalg.norm(lead - f)
        f = f + (0.4 if gap > 6 else 0.1) * np.array([np.cos(fyaw), np.sin(fyaw)])
        delta = np.array([f[0] - prev_f[0], f[1] - prev_f[1]])                                                   # arctic_env.py:165-175
        prev_f = f.copy()
        # fake lidar: points on the rocks within 16 m, as pairs (one end, the other end) -- some closer than 0.5 m to their successor
        rel = rocks - f
        near = rel[np.linalg.norm(rel, axis=1) < 16.0]
        near = near[np.argsort(np.arctan2(near[:, 1], near[:, 0]))][:max_pts // 2]
        p1 = np.repeat(near, 2, axis=0) + np.tile(np.array([[0.0, 0.0], [0.3, 0.1]]), (len(near), 1)) if len(near) else np.zeros((0, 2))
        p2 = p1 + rng.uniform(0.4, 1.2, p1.shape)
        yield lead - f, fyaw, delta, p1, p2


RESET = "reset"      # a script yields this between two calls: tracker.reset() + every laser.reset() (SEN:217-220, 964-968)


def run(name, seed, steps, lasers, max_pts=48, script=wander, out_dir=GOLDEN):
    """`script(rng, steps, max_pts)` yields `leader_rel, yaw, delta, p1, p2` per call (follower frame; delta = (delta_x, delta_y);
    p1 / p2 [n_pts, 2]), or RESET.  The calls after a RESET are marked in the optional array `reset` (absent when a script never resets)."""
    gt = load_reference()
    rng = np.random.default_rng(seed)
    trk = gt.GazeboLeaderPositionsTracker_v2(host_object="arctic_robot", sensor_name="LeaderTrackDetector", saving_period=5,
                                             corridor_width=2, corridor_length=25)                                 # arctic_env.py:62-66
    sens = [gt.GazeboCorridor_Prev_lasers_v2(host_object="arctic_robot", **kw) for kw in lasers]
    rec = dict(leader=[], yaw=[], delta=[], pts1=[], pts2=[], n_pts=[], counter=[], hist=[], corr=[], n_hist=[], n_corr=[])
    outs = [[] for _ in sens]
    resets, pending = [], False
    for call in script(rng, steps, max_pts):
        if isinstance(call, str) and call == RESET:
            trk.reset()
            for s in sens:
                s.reset()
            pending = True
            continue
        leader_rel, fyaw, d, p1, p2 = call
        leader_rel = np.asarray(leader_rel, np.float64); p1 = np.asarray(p1, np.float64).reshape(-1, 2); p2 = np.asarray(p2, np.float64).reshape(-1, 2)
        assert len(p1) == len(p2) <= max_pts
        resets.append(pending); pending = False
        delta = {"delta_x": np.float64(d[0]), "delta_y": np.float64(d[1])}
        orient = np.array([0.0, 0.0, fyaw])
        hist, corr = trk.scan(leader_rel, orient, delta)
        for k, s in enumerate(sens):
            with np.errstate(all="ignore"):
                outs[k].append(np.asarray(s.scan(orient, corr, list(p1), list(p2))).astype(np.float32 if not lasers[k]["pad_sectors"] else np.float64))
        rec["leader"].append(leader_rel.copy()); rec["yaw"].append(fyaw); rec["delta"].append([delta["delta_x"], delta["delta_y"]])
        a1 = np.zeros((max_pts, 2)); a2 = np.zeros((max_pts, 2)); a1[:len(p1)] = p1; a2[:len(p2)] = p2
        rec["pts1"].append(a1); rec["pts2"].append(a2); rec["n_pts"].append(len(p1))
        h = np.full((64, 2), np.nan); c = np.full((64, 4), np.nan)
        hh = np.array([np.asarray(p, np.float64) for p in hist]).reshape(-1, 2)
        cc = np.array([[q[0][0], q[0][1], q[1][0], q[1][1]] for q in corr], np.float64).reshape(-1, 4)
        h[:len(hh)] = hh; c[:len(cc)] = cc
        rec["hist"].append(h); rec["corr"].append(c); rec["n_hist"].append(len(hh)); rec["n_corr"].append(len(cc)); rec["counter"].append(trk.saving_counter)
    assert len(rec["yaw"]) == steps, (name, len(rec["yaw"]), steps)
    out = {k: np.array(v) for k, v in rec.items()}
    for k, o in enumerate(outs):
        out["laser%d" % k] = np.stack(o)
    import json
    out["meta"] = np.array(json.dumps(dict(name=name, seed=seed, steps=steps, max_pts=max_pts, numpy=np.__version__,
                                           lasers=[{k: v for k, v in kw.items() if k != "sensor_name"} for kw in lasers])))
    if any(resets):
        out["reset"] = np.array(resets)
    path = os.path.join(out_dir, "gazebo_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("gazebo", name, "steps", steps, "hist", out["n_hist"].min(), out["n_hist"].max(), "corr", out["n_corr"].max(),
          "pts", out["n_pts"].max(), "laser0 hit frac", float((out["laser0"] < lasers[0]["laser_length"] * 0.999).mean()),
          "laser1 hit frac", float((out["laser1"] < lasers[1]["laser_length"] * 0.999).mean()), os.path.getsize(path))


# ---- scripted scenarios: the edges of the kernel's capacity and inputs (follower frame throughout) -----------------------------------
MANY_PTS = (63, 64, 65, 66, 127, 128, 129, 136)      # either side of one and of two wavefronts' lanes, and max_pts


def _spiral_points(rng, n, total):
    """n of `total` obstacle points on an inward spiral: the later the index, the nearer the point (9.5 m -> 3.5 m), so the segments
    of the high indices shadow rays that the low ones would stop; every fourth point has its successor 0.32 m away (the < 0.5 m
    branch of collect_obstacle_edges), every other segment runs about 1 m across the rays to its points_2 end."""
    i = np.arange(n)
    th = 2.399963 * i + rng.normal(0, 0.02, n)
    r = 9.5 - 6.0 * i / total + rng.normal(0, 0.05, n)
    p1 = np.stack([r * np.cos(th), r * np.sin(th)], 1)
    close = (i % 4 == 1)
    p1[close] = p1[np.nonzero(close)[0] - 1] + np.array([0.3, 0.1])
    p2 = p1 + np.stack([-np.sin(th), np.cos(th)], 1) * rng.uniform(0.8, 1.4, (n, 1))
    return p1, p2


def _follow(rng, t, lead):
    """One call of an ordinary chase along +x: the leader gains 0.05 m per call on a follower that moves 0.3 m."""
    delta = np.array([0.3, rng.normal(0, 0.02)])
    lead = lead + np.array([0.35, rng.normal(0, 0.05)]) - delta
    return lead, delta


def many_pts(rng, steps, max_pts):
    lead, yaw = np.array([7.0, 0.0]), 0.1
    for t in range(steps):
        lead, delta = _follow(rng, t, lead)
        yaw += rng.normal(0, 0.03)
        p1, p2 = _spiral_points(rng, MANY_PTS[t % len(MANY_PTS)], max_pts)
        yield lead, yaw, delta, p1, p2


def few_pts(rng, steps, max_pts):
    lead, yaw = np.array([7.0, 0.0]), -0.2
    for t in range(steps):
        lead, delta = _follow(rng, t, lead)
        n = t % 4                                      # 0 and 1 point: no obstacle segment at all
        sgn = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        p1 = np.stack([2.5 + 0.8 * np.arange(n) + rng.normal(0, 0.05, n), 2.0 * sgn], 1).reshape(-1, 2)
        p2 = p1 + np.stack([np.full(n, 0.2), -4.0 * sgn], 1).reshape(-1, 2)      # across the x axis, 2.5 - 4 m ahead
        yield lead, yaw, delta, p1, p2


def seed_line(rng, steps, max_pts):
    """yaw = pi puts the seed's start point at (10, 0): np.linspace gets a zero step on the y axis for a leader at (7, 0), and on both
    axes for a leader at (10, 0) (ten identical seed points, a corridor of 0 / 0)."""
    for x0 in (7.0, 10.0):
        if x0 != 7.0:
            yield RESET
        lead = np.array([x0, 0.0])
        for t in range(steps // 2):
            p1 = np.array([[3.0, -1.5], [3.2, 1.5], [-4.0, 1.0]]) + rng.normal(0, 0.05, (3, 2))
            yield lead, np.pi, np.array([0.1, 0.0]) if t else np.zeros(2), p1, p1 + np.array([0.5, 2.0])
            lead = lead + np.array([0.45, 0.0 if t < 4 else 0.05]) - np.array([0.1, 0.0])


def jump(rng, steps, max_pts):
    """Call 9: the leader is suddenly 13 m further off (a saving call: the path grows by as much, and several history points and
    corridor pairs go in that one call).  Call 24: the follower is set back 9 m, history, corridor and leader with it.  Calls 27-44:
    the follower closes in faster than the leader moves, so the leader's distance shrinks, nothing is appended to the history, and
    the corridor still gains a pair per saving call: the two lengths part company."""
    lead, yaw = np.array([7.0, 0.0]), 0.0
    for t in range(steps):
        fast = 27 <= t < 45
        delta = np.array([-9.0 if t == 24 else (1.6 if fast else 0.3), rng.normal(0, 0.02)])
        lead = lead + np.array([13.0 if t == 9 else 0.35, rng.normal(0, 0.3 if fast else 0.05)]) - delta
        p1 = np.array([[4.0, -3.0], [4.2, -2.9], [5.0, 3.0], [-2.0, 2.0]]) + rng.normal(0, 0.05, (4, 2))
        yield lead, yaw, delta, p1, p1 + np.array([0.3, 1.5])


def out_of_range(rng, steps, max_pts):
    """After the seeding call the leader stays 26-40 m away: nothing is appended to the history (new_dist < 25 fails), nothing is
    trimmed, and every saving call appends one more pair to the corridor.  Stopped below the kernel's 64 pairs.  (The follower moves
    on every tenth call only, so that consecutive records repeat and the file stays small.)"""
    for t in range(steps):
        ang = 0.02 * t
        lead = np.array([7.0, 0.0]) if t == 0 else (26.0 + 14.0 * (t % 7) / 6.0) * np.array([np.cos(ang), np.sin(ang)])
        delta = np.array([0.125, -0.0625]) if t % 10 == 9 else np.zeros(2)
        p1 = np.array([[6.0, -2.0], [6.1, 2.0], [2.0, 6.0]])
        yield lead, 0.05 * np.sin(0.3 * t), delta, p1, p1 + np.array([0.0, 1.0])


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    run("arctic_s1", 1, 160, LASERS, out_dir=out_dir)
    run("arctic_s4", 4, 120, LASERS, out_dir=out_dir)
    run("pad_s7", 7, 100, LASERS_PAD, out_dir=out_dir)
    run("many_pts", 11, 40, LASERS, max_pts=136, script=many_pts, out_dir=out_dir)
    run("few_pts", 12, 24, LASERS, max_pts=4, script=few_pts, out_dir=out_dir)
    run("seed_line", 13, 24, LASERS, max_pts=4, script=seed_line, out_dir=out_dir)
    run("jump", 14, 60, LASERS, max_pts=4, script=jump, out_dir=out_dir)
    run("out_of_range", 15, 126, LASERS, max_pts=4, script=out_of_range, out_dir=out_dir)
