#!/usr/bin/env python3
"""What the baseline follower costs on bench.py's workload B (65,536 envs, the captured pool), from device events, every round from
the same snapshot so that all of them do the same work:
  (i)   ms per call of BaselineFollower.act() alone;
  (ii)  ms per closed-loop step of rollout_baseline (T steps, sensors=False, actions recorded);
  (iii) ms per step of rollout on those recorded, resident actions at the same T;
  (iv)  ms per step of rollout on actions of bench.py's action sets at the same T.
(ii) against (iii) is the price of the act kernel inside the loop.  On a tree without the baseline module only (iv) is measured: the
figure that compares `rollout` itself across commits.  Prints one JSON line.
usage: baseline_rollout_times.py [--envs N] [--T T] [--rounds R]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (build_workload / make_actions: the workload bench.py measures)
from continiousenvironment_follower_leader_amd import shard  # noqa: E402
from continiousenvironment_follower_leader_amd.vec_game import VecGame  # noqa: E402

try:
    from continiousenvironment_follower_leader_amd.baseline import BaselineFollower
except ImportError:
    BaselineFollower = None


def timed(fn, per):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg, pool, _, _, _ = bench.build_workload("B", 0, 0, dev)
    n, T = a.envs, a.T
    env = VecGame(n, device=dev, config=cfg)
    env.load_scenarios(pool)
    env.reset(shard.scenario_index(0, 0, n, pool.n))
    snap = env.snapshot()
    result = dict(workload="B", envs=n, T=T, rounds=a.rounds, baseline=BaselineFollower is not None)
    times = dict(act=[], rollout_baseline=[], rollout=[], rollout_bench_actions=[])
    sets = bench.make_actions(cfg, n, 16, 0, dev)
    fixed = torch.stack([sets[t % 16] for t in range(T)]).contiguous()
    env.rollout(fixed, sensors=False)                                                   # warm-up
    if BaselineFollower is not None:
        env.restore(snap, slot_stats=True)
        f = BaselineFollower(env)
        acts = env.rollout_baseline(f, T, sensors=False, record=True)[3].clone()       # warm-up; the actions every timed round replays
    for _ in range(a.rounds):
        if BaselineFollower is not None:
            env.restore(snap, slot_stats=True)
            f.state.zero_()
            times["rollout_baseline"].append(timed(lambda: env.rollout_baseline(f, T, sensors=False, record=True), T))
            times["act"].append(timed(lambda: [f.act() for _ in range(100)], 100))
            env.restore(snap, slot_stats=True)
            times["rollout"].append(timed(lambda: env.rollout(acts, sensors=False), T))
        env.restore(snap, slot_stats=True)
        times["rollout_bench_actions"].append(timed(lambda: env.rollout(fixed, sensors=False), T))
    result["ms"] = {k: statistics.median(v) for k, v in times.items() if v}
    result["all_rounds_ms"] = {k: v for k, v in times.items() if v}
    if BaselineFollower is not None:
        result["closed_over_open_loop"] = result["ms"]["rollout_baseline"] / result["ms"]["rollout"]
        result["followers_flagged"] = int(f.flags().ne(0).sum())
    print(json.dumps(result))
    env.close()


if __name__ == "__main__":
    main()
