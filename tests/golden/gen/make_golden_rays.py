#!/usr/bin/env python3
"""Records of the UNMODIFIED reference's ray sensors on the crafted worlds of tests/ray_edge_cases.py -- runs only where the reference
is installed (see make_golden.py: same stand-ins for pygame and gym, reference imported at run time).

For every case of groups A-E and G the oracle is stepped through the case (ray_edge_cases.get_case keeps its trace).  After the reset and
after every step the oracle's state -- follower pose, leader and bear hitboxes, static rects, the corridor of OracleEnv.debug() -- is
handed to the reference's own sensor objects (LeaderCorridor_Prev_lasers_v2, LeaderCorridor_lasers_v2, LeaderCorridor_lasers), which are
constructed once per env and keep their own obstacle history.  Their outputs go to tests/golden/ray_edges.npz, laid out like the
oracle's `lasers` row; tests/test_ray_edges_host.py compares the oracle with them.  Only the envs a case lists under "golden" are
recorded (group D: every 8th heading).

A sensor registered ahead of the tracker is scanned before the tracker's second scan of the step and sees an older corridor than
debug() returns; every such sensor of these cases reacts to obstacles only, so the corridor it is handed matters by `len(corridor) > 1`
alone.

usage:  python tests/golden/gen/make_golden_rays.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, os.path.join(HERE, "standins"))
sys.path.insert(0, "/root/reference/src")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import pygame  # noqa: E402  (the stand-in)
from continuous_grid_arctic.utils import sensors as ref  # noqa: E402

import ray_edge_cases as X  # noqa: E402


class _Obj:
    blocks_vision = True

    def __init__(self):
        self.rectangle = pygame.Rect(0, 0, 1, 1)
        self.position = np.zeros(2, np.float32)
        self.direction = 0.0


class _Env:
    """What collect_obstacle_edges reads of the Game: the two object lists and the follower."""

    def __init__(self, n_static, n_bears):
        self.leader, self.follower = _Obj(), _Obj()
        self.statics = [_Obj() for _ in range(n_static)]
        self.bears = [_Obj() for _ in range(n_bears)]
        self.game_object_list = [self.leader, self.follower] + self.statics         # ENV:533-536: the robots, then the rocks
        self.game_dynamic_list = list(self.bears)

    def load(self, static, rec):
        for o, q in zip(self.statics, static):
            o.rectangle = pygame.Rect(*(int(v) for v in q))
        for o, q in zip([self.leader, self.follower] + self.bears, rec["boxes"]):
            o.rectangle = pygame.Rect(*(int(v) for v in q))
        self.follower.position = rec["fpos"].astype(np.float32)
        self.follower.direction = float(rec["fdir"])


def _sensor(spec, host):
    kw = {k: v for k, v in spec.items() if k not in ("sensor_class", "_allow_any_lasers_count", "sensor_name")}
    cls = getattr(ref, spec["sensor_class"])
    n = kw.get("lasers_count")
    if n is not None and n not in (12, 20, 24, 36):          # the constructor accepts four counts only (SEN:761); as make_golden.py does for
        kw["lasers_count"] = 12                                # config D, the count is set on the constructed object
    s = cls(host, **kw)
    if n is not None and n != s.lasers_count:
        s.lasers_count, s.laser_period = n, 360 / n
    return s


def record(case):
    cfg = case["cfg"]
    specs = cfg.kwargs["follower_sensors"]
    out = np.zeros((len(case["golden"]), case["steps"] + 1, cfg.lasers_len), np.float32)
    for g, e in enumerate(case["golden"]):
        env = _Env(cfg.c.n_static, cfg.c.n_bears)
        sens = [(l, _sensor(specs[l.name], env.follower)) for l in cfg.lasers]
        for t, rec in enumerate(case["trace"][e]):
            env.load(case["scen"][e]["static_rects"], rec)
            corridor = [[np.array(c[0:2]), np.array(c[2:4])] for c in rec["corr"]]
            for l, s in sens:
                got = np.asarray(s.scan(env, corridor), np.float32).reshape(-1)
                assert got.size == l.history * l.width, (case["name"], l.name, got.shape)
                out[g, t, l.out_offset:l.out_offset + got.size] = got
    return out


def main():
    names = X.case_names()
    n_dense, _ = X.largest_n_static()
    names.append("G-dense-%d" % n_dense)
    arrays, same, total = {}, 0, 0
    for name in names:
        case = X.get_case(name)
        ref_out = record(case)
        ora = np.stack([np.stack([r["lasers"] for r in case["trace"][e]]) for e in case["golden"]])
        arrays[name] = ref_out
        arrays[name + "/envs"] = np.array(case["golden"], np.int32)
        same += int((ora == ref_out).sum()); total += ref_out.size
        print("%-24s envs %3d  states %2d  readings %7d  not bit-identical to the oracle %d, worst |diff| %.3g"
              % (name, len(case["golden"]), case["steps"] + 1, ref_out.size, int((ora != ref_out).sum()), float(np.abs(ora - ref_out).max())), flush=True)
    path = os.path.join(GOLDEN, "ray_edges.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes, %d of %d readings bit-identical to the oracle" % (path, os.path.getsize(path), same, total))


if __name__ == "__main__":
    main()
