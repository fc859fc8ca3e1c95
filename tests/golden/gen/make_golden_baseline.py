#!/usr/bin/env python3
"""Golden vectors of the reference's baseline controller -- runs ONLY in the build container (needs /root/reference), like
``make_golden.py``, whose ``Runner`` and stand-ins it imports unchanged.

  * ``baseline_table.npz``: 4,096 rows (direction f32, pos f32 x 2, target f64 x 2, v, w) out of the reference's own
    ``utils/misc.py:move_to_the_point`` -- random rows plus crafted ones for every branch of MISC:16-26 and MISC:73-91.
  * ``baseline_{A_s0,B_s1,Bastar_s1,E_s3}.npz``: the loop of ``run_2d.py`` lines 119-148 (restated in ``baseline_episode`` below; the
    file itself needs a display, a video recorder and gym's registry) around ``Game(**kwargs)`` of those configs, to ``done`` or 300
    steps: scenario and per-step action / obs / reward / done / info as the episode fixtures hold them, plus the FIFO length the decision
    of every step saw, and the append and the pop that followed the step.

A seed is kept only if the reference does not raise (the FIFO never runs empty), the FIFO never exceeds 64 points and no ``v`` lies within
4 ulp of the pop threshold 20.0; ``tests/test_baseline_host.py`` checks the same on the files.

usage:  python tests/golden/gen/make_golden_baseline.py [--only NAME]
"""
import argparse
import json
import os

import numpy as np

import make_golden as MG            # (puts the stand-ins and the reference on sys.path)

GOLDEN = MG.GOLDEN
N_TABLE = 4096
MAX_STEPS = 300
FIFO_LIMIT = 64
POP_AT = 20.0

# (name, config of make_golden.CONFIGS, python seed)
EPISODES = [("A_s0", "A", 0), ("B_s1", "B", 1), ("Bastar_s1", "B_astar", 1), ("E_s3", "E", 3)]


def reference_controller():
    MG.import_reference()
    from continuous_grid_arctic.utils.misc import move_to_the_point
    from scipy.spatial import distance
    return move_to_the_point, distance


def near_threshold(v):
    return abs(v - POP_AT) <= 4 * np.spacing(POP_AT)


def table_rows(rng):
    """(direction f32, pos f32[2], target f64[2], target is integer) rows: crafted first, random to N_TABLE."""
    rows = []
    dirs = [0.0, 0.5, 10.0, 45.3, 90.0, 179.9, 180.0, 180.2, 225.0, 270.0, 350.0, 359.99]
    for pos in ((700.0, 500.0), (700.25, 500.5)):
        for k in range(24):                                    # targets on 24 compass bearings: rx == 0 at 90 / 270, rx < 0 on the left half
            ang = np.radians(15.0 * k)
            for integer in (True, False):
                off = np.array([np.cos(ang), np.sin(ang)]) * (120.0 if integer else 37.3)
                off[np.abs(off) < 1e-9] = 0.0                  # exactly on the axes
                tgt = np.array(pos) + (np.rint(off) if integer else off)
                if integer:
                    tgt = np.floor(tgt) if pos[0] != 700.0 else tgt
                    if pos[0] != 700.0 and k in (6, 18):       # rx == 0 away from integer positions too
                        tgt[0] = pos[0]
                for d in dirs:
                    rows.append((np.float32(d), np.array(pos, np.float32), tgt.astype(np.float64), bool(integer and np.all(tgt == np.rint(tgt)))))
    # an angle difference of exactly 0, of exactly 180, above 180 in both senses, at unit distance steps
    for des, cur in ((0, 0.3), (45, 45.9), (0, 180.6), (180, 0.2), (350, 10.0), (10, 350.0), (359, 0.0), (0, 359.99), (181, 0.9), (1, 181.5)):
        for dist in (5.0, 20.0, 21.0, 300.0):
            a = np.radians(des + 0.5)
            rows.append((np.float32(cur), np.array((640.0, 480.0), np.float32), np.array([640.0 + dist * np.cos(a), 480.0 + dist * np.sin(a)]), False))
    while len(rows) < N_TABLE:
        pos = np.array([rng.uniform(0, 1500), rng.uniform(0, 1000)], np.float32)
        near = rng.random() < 0.3
        tgt = pos.astype(np.float64) + rng.uniform(-30, 30, 2) if near else np.array([rng.uniform(0, 1500), rng.uniform(0, 1000)])
        integer = rng.random() < 0.5
        if integer:
            tgt = np.rint(tgt)
        rows.append((np.float32(rng.uniform(0, 360)), pos, tgt, bool(integer)))
    return rows[:N_TABLE]


def make_table():
    move_to_the_point, _ = reference_controller()
    rows = table_rows(np.random.default_rng(20240))
    out = dict(direction=np.zeros(N_TABLE, np.float32), pos=np.zeros((N_TABLE, 2), np.float32), target=np.zeros((N_TABLE, 2)),
               target_is_int=np.zeros(N_TABLE, np.uint8), v=np.zeros(N_TABLE), w=np.zeros(N_TABLE))
    for i, (d, pos, tgt, integer) in enumerate(rows):
        # what run_2d.py:128-136 hands over: a float32 scalar, a float32 pair, and the target point as the env holds it (ints or floats)
        nxt = tgt.astype(np.int64) if integer else tgt
        a = move_to_the_point(d, pos, nxt)
        out["direction"][i], out["pos"][i], out["target"][i], out["target_is_int"][i] = d, pos, tgt, integer
        out["v"][i], out["w"][i] = a[0], a[1]
    path = os.path.join(GOLDEN, "baseline_table.npz")
    np.savez_compressed(path, **out)
    print("table rows=%d rx==0: %d  integer targets: %d -> %s %d bytes" % (
        N_TABLE, int((out["pos"][:, 0].astype(np.float64) == out["target"][:, 0]).sum()), int(out["target_is_int"].sum()), path, os.path.getsize(path)))


def baseline_episode(config_name, seed):
    """run_2d.py:119-148 without the window and the recorder.  Returns the record, or a string saying which condition the seed breaks."""
    move_to_the_point, distance = reference_controller()
    r = MG.Runner(config_name)
    obs = r.reset(seed)
    g = r.game
    laser_names = [k for k, v in g.follower_sensors.items()
                   if v.get("sensor_class", k) in ("LeaderCorridor_Prev_lasers_v2", "LeaderCorridor_lasers_v2", "LeaderCorridor_lasers",
                                                   "LeaderCorridor_lasers_compas")]
    out = {"scen:" + k: v for k, v in MG.scenario_of(g).items()}
    for k, v in MG.obs_record(g, obs, laser_names).items():
        out["reset:" + k] = v
    stack = [obs["leader_target_point"]]
    acts, rews, dones, infos, fifo, apps, pops, rows = [], [], [], [], [], [], [], {}
    for t in range(MAX_STEPS):
        if not stack:
            return "the FIFO ran empty at step %d (the reference raises IndexError)" % t
        if len(stack) > FIFO_LIMIT:
            return "the FIFO holds %d points at step %d" % (len(stack), t)
        direction = obs["numerical_features"][8]
        position = np.array((obs["numerical_features"][5], obs["numerical_features"][6]))
        next_point = stack[0]
        action = move_to_the_point(direction, position, next_point)
        if near_threshold(float(action[0])):
            return "v = %r at step %d is within 4 ulp of the pop threshold" % (float(action[0]), t)
        fifo.append(len(stack))
        obs, rew, done, info = r.step(action)
        appended = not np.array_equal(obs["leader_target_point"], stack[-1])
        if appended:
            stack.append(np.array(obs["leader_target_point"]))
        popped = bool(distance.euclidean(position, next_point) <= 20)
        if popped:
            stack.pop(0)
        acts.append((float(action[0]), float(action[1]))); rews.append(float(rew)); dones.append(bool(done))
        infos.append([MG.MISSION[info["mission_status"]], MG.AGENT[info["agent_status"]], MG.LEADER[info["leader_status"]]])
        apps.append(appended); pops.append(popped)
        for k, v in MG.obs_record(g, obs, laser_names).items():
            rows.setdefault(k, []).append(v)
        if done:
            break
    out.update(actions=np.array(acts, np.float64), reward=np.array(rews), done=np.array(dones, np.uint8), info=np.array(infos, np.uint8))
    out["bl:fifo_len"], out["bl:append"], out["bl:pop"] = np.array(fifo, np.int32), np.array(apps, np.uint8), np.array(pops, np.uint8)
    for k, v in rows.items():
        out["obs:" + k] = np.stack(v)
    meta = dict(config=config_name, seed=seed, policy="baseline", n_steps=len(acts), kwargs=json.loads(json.dumps(r.cfg["kwargs"], default=str)),
                post=r.cfg["post"], laser_names=laser_names, numpy=np.__version__, tick="frame k sees get_ticks()==k")
    out["meta"] = np.array(json.dumps(meta))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if a.only in (None, "table"):
        make_table()
    limit = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("episode_"))
    for name, cfg, seed in EPISODES:
        if a.only not in (None, name):
            continue
        out = baseline_episode(cfg, seed)
        if isinstance(out, str):
            raise SystemExit("baseline_%s: %s -- choose another seed" % (name, out))
        path = os.path.join(GOLDEN, "baseline_%s.npz" % name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size <= limit, (name, size, limit)
        print("baseline %-10s steps=%3d done=%d fifo<=%d appends=%d pops=%d return=%.2f bytes=%d" % (
            name, len(out["done"]), int(out["done"][-1]), int(out["bl:fifo_len"].max()), int(out["bl:append"].sum()), int(out["bl:pop"].sum()),
            float(out["reward"].sum()), size), flush=True)


if __name__ == "__main__":
    main()
