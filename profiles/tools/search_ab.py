#!/usr/bin/env python3
"""What the action search costs and what it buys, on bench.py's workload B (the captured pool) on one GPU.  Measured, not asserted.

Cost: n real envs a few steps into their episodes, K candidates, horizon T, hold, iters 1 and 3 -- milliseconds per ``ActionSearch.act()`` as
the median of ``--blocks`` blocks of ``--reps`` calls, each block ending in a device synchronise, and beside it the milliseconds of the
``iters * T`` blind steps of the n * K clones it contains (``rollout(cand, sensors=False)`` after an untimed fan-out, from device events),
so that the share of pack, fan-out, sample and select is visible.

Quality: one fixed list of ``--scenarios`` scenarios played once each with ``evaluate(policy, sensors=False)`` on ``--slots`` slots by the
search (iters 1 and 3, clones on their source's stream and on their own), by ``BaselineFollower`` and by the constant action
(max_speed, 0): mean return and number of successful missions.

Writes one JSON file (default profiles/search_ab.json) and prints it.
usage: search_ab.py [--envs 1024] [--K 64] [--T 8] [--hold 2] [--blocks 5] [--reps 4] [--scenarios 256] [--slots 256] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (build_workload: the workload bench.py measures)
from continiousenvironment_follower_leader_amd import _lib, abi, shard  # noqa: E402
from continiousenvironment_follower_leader_amd.baseline import BaselineFollower  # noqa: E402
from continiousenvironment_follower_leader_amd.search import ActionSearch  # noqa: E402
from continiousenvironment_follower_leader_amd.vec_game import VecGame  # noqa: E402


def cost(cfg, pool, dev, a):
    env = VecGame(a.envs, device=dev, config=cfg)
    env.load_scenarios(pool)
    env.reset(shard.scenario_index(0, 0, a.envs, pool.n))
    follower = BaselineFollower(env)
    for _ in range(8):                                         # under way, on the baseline's actions
        env.step(follower.act(), sensors=False)
    out = {}
    for iters in (1, 3):
        s = ActionSearch(env, a.K, a.T, hold=a.hold, iters=iters)
        s.act()
        torch.cuda.synchronize()
        act_ms, roll_ms = [], []
        for _ in range(a.blocks):
            t0 = time.perf_counter()
            for _ in range(a.reps):
                s.act()
            torch.cuda.synchronize()
            act_ms.append((time.perf_counter() - t0) * 1e3 / a.reps)
        st = env._stream()
        for _ in range(a.blocks):
            total = 0.0
            for _ in range(a.reps):
                _lib.check(s.lib.ftl_unpack_envs_from(s.clones.h, s.rows.data_ptr(), s.row_ids.data_ptr(), s.env_ids.data_ptr(), a.envs * a.K, 0, st), s.lib)
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                s.clones.rollout(s.cand, gamma=1.0, sensors=False)
                ev1.record()
                torch.cuda.synchronize()
                total += ev0.elapsed_time(ev1)
            roll_ms.append(total / a.reps * iters)
        out["iters_%d" % iters] = dict(act_ms=statistics.median(act_ms), act_ms_blocks=act_ms,
                                       blind_steps_ms=statistics.median(roll_ms), blind_steps=iters * a.T, clones=a.envs * a.K,
                                       best_ret_mean=float(s.best_ret.mean()), best_k_nonzero=int(s.best_k.ne(0).sum()))
        s.close()
    env.close()
    return out


def quality(cfg, pool, dev, a):
    scen = (torch.arange(a.scenarios) * 7) % pool.n
    speed = cfg.c.follower.max_speed

    def play(make):
        env = VecGame(a.slots, device=dev, config=cfg)
        env.load_scenarios(pool)
        policy = make(env)
        t0 = time.perf_counter()
        recs = env.evaluate(policy, scen, sensors=False)
        sec = time.perf_counter() - t0
        if hasattr(policy, "close"):
            policy.close()
        env.close()
        return dict(mean_return=float(recs["ret"].mean()), success=int((recs["status"][:, 0] == abi.MISSION.index("success")).sum()),
                    crash=int((recs["status"][:, 1] == abi.AGENT.index("crash")).sum()), mean_frames=float(recs["frames"].mean()),
                    seconds=sec)

    def constant(env):
        action = torch.tensor([speed, 0.0], dtype=torch.float64, device=dev).repeat(env.n, 1).contiguous()
        return lambda obs: action
    out = dict(scenarios=a.scenarios, slots=a.slots, constant=play(constant), baseline=play(BaselineFollower))
    for iters in (1, 3):
        for own in (False, True):
            out["search_iters_%d_%s" % (iters, "own_stream" if own else "source_stream")] = play(
                lambda env: ActionSearch(env, a.K, a.T, hold=a.hold, iters=iters, own_stream=own))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--T", type=int, default=8)
    ap.add_argument("--hold", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--scenarios", type=int, default=256)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg, pool, _, _, _ = bench.build_workload("B", 0, 0, dev)
    result = dict(workload="B", device=torch.cuda.get_device_name(dev), envs=a.envs, K=a.K, T=a.T, hold=a.hold, gamma=1.0, spread=1.0, decay=0.5,
                  cost=cost(cfg, pool, dev, a), quality=quality(cfg, pool, dev, a))
    text = json.dumps(result, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
