#!/usr/bin/env python3
"""What a feed-forward policy with tanh hidden layers costs in the loop on bench.py's workload B (65,536 envs, the captured pool, net
180-64-64-2), by the protocol of mlp_policy_times.py: device events around windows that end in a device synchronise, every window from the
same snapshot, the variants alternated, `rounds` windows each after a warm-up, the median and every window kept; one set of weights and
1,024 sets of 64 envs:
  (a) ms per closed-loop step of rollout_mlp(T) with MlpPolicy(activation="tanh");
  (b) ms per step of the same closed loop written with step() and torch ops on the same stream: float32 addmm (baddbmm for a
      population) / torch.tanh / the head map in float64, then step();
  (c) ms per launch of the tanh act kernel alone and, in the same run and alternated with it, of the ReLU act kernel alone on the same
      weights (200 launches between two device events).
Writes one JSON document.
usage: mlp_tanh_times.py [--envs N] [--T T] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (build_workload: the workload bench.py measures)
from continiousenvironment_follower_leader_amd import shard  # noqa: E402
from continiousenvironment_follower_leader_amd.mlp import MlpPolicy  # noqa: E402
from continiousenvironment_follower_leader_amd.vec_game import VecGame  # noqa: E402

WIDTHS = (180, 64, 64, 2)
LAUNCHES = 200


def timed(fn, per):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / per


def param_count(widths):
    return sum((a + 1) * b for a, b in zip(widths[:-1], widths[1:]))


def layer_views(params, widths):
    """[(W [sets, in, out], b [sets, out])] of a [sets, param_count] tensor in the layout of ftl_mlp."""
    out, off = [], 0
    for a, b in zip(widths[:-1], widths[1:]):
        out.append((params[:, off:off + a * b].view(-1, a, b), params[:, off + a * b:off + a * b + b]))
        off += (a + 1) * b
    return out


def torch_loop(env, params, n_sets, T, lo, hi):
    """(b): T closed-loop steps of the tanh net with step() and torch ops."""
    ls = layer_views(params, WIDTHS)
    n = env.n
    for _ in range(T):
        h = env.policy_obs.view(n_sets, n // n_sets, WIDTHS[0])
        for l, (W, b) in enumerate(ls):
            h = torch.addmm(b[0], h[0], W[0])[None] if n_sets == 1 else torch.baddbmm(b[:, None, :], h, W)
            if l + 1 < len(ls):
                h = torch.tanh(h)
        u = h.view(n, 2).double().clamp(-1.0, 1.0)
        env.step(torch.minimum(torch.maximum(lo + ((u + 1.0) * 0.5) * (hi - lo), lo), hi))


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_tanh_B65536.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg, pool, _, _, _ = bench.build_workload("B", 0, 0, dev)
    n, T = a.envs, a.T
    env = VecGame(n, device=dev, config=cfg, policy_obs=True)
    env.load_scenarios(pool)
    env.reset(shard.scenario_index(0, 0, n, pool.n))
    snap = env.snapshot()
    lo = torch.tensor(cfg.action_low, dtype=torch.float64, device=dev)
    hi = torch.tensor(cfg.action_high, dtype=torch.float64, device=dev)
    result = dict(workload="B", envs=n, widths=WIDTHS, T=T, rounds=a.rounds, activation="tanh", act_launches_per_window=LAUNCHES,
                  method="device events around a window that ends in a device synchronise; every window from the same snapshot; the "
                         "variants alternated; `rounds` windows each after a warm-up; median and min..max of the windows")
    for n_sets in (1, 1024):
        g = torch.Generator(device="cpu")
        g.manual_seed(n_sets)
        params = (torch.randn(n_sets, param_count(WIDTHS), generator=g) * 0.1).to(dev)
        pol = MlpPolicy(env, WIDTHS, params=params, n_sets=n_sets, activation="tanh")
        relu = MlpPolicy(env, WIDTHS, params=params, n_sets=n_sets, activation="relu")
        times = dict(rollout_mlp_tanh=[], torch_loop_tanh=[], act_tanh=[], act_relu=[])
        env.restore(snap, slot_stats=True)
        torch_loop(env, params, n_sets, 20, lo, hi)                                    # warm-up of every shape the windows use
        env.restore(snap, slot_stats=True)
        env.rollout_mlp(pol, 20)
        for p in (pol, relu):
            for _ in range(20):
                p.act()
        for _ in range(a.rounds):
            env.restore(snap, slot_stats=True)
            times["rollout_mlp_tanh"].append(timed(lambda: env.rollout_mlp(pol, T), T))
            env.restore(snap, slot_stats=True)
            times["torch_loop_tanh"].append(timed(lambda: torch_loop(env, params, n_sets, T, lo, hi), T))
            times["act_tanh"].append(timed(lambda: [pol.act() for _ in range(LAUNCHES)], LAUNCHES))
            times["act_relu"].append(timed(lambda: [relu.act() for _ in range(LAUNCHES)], LAUNCHES))
        r = dict(ms={k: spread(v) for k, v in times.items()}, all_windows_ms=times)
        a_w, b_w = times["rollout_mlp_tanh"], times["torch_loop_tanh"]
        r["rollout_minus_torch_loop_ms"] = statistics.median(a_w) - statistics.median(b_w)
        r["gap_slowest_a_to_fastest_b_ms"] = min(b_w) - max(a_w)
        r["bar_slowest_a_below_fastest_b_by_more_than_b_spread"] = bool(min(b_w) - max(a_w) > max(b_w) - min(b_w))
        r["act_tanh_over_act_relu"] = statistics.median(times["act_tanh"]) / statistics.median(times["act_relu"])
        r["act_note"] = "%d back-to-back launches between two device events: launch gaps included" % LAUNCHES
        result["sets_%d" % n_sets] = r
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    env.close()


if __name__ == "__main__":
    main()
