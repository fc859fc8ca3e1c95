#!/usr/bin/env python3
"""What a feed-forward policy in the loop costs on bench.py's workload B (65,536 envs, the captured pool, net 180-64-64-2), from device
events, every window from the same snapshot so that all of them do the same work; one set of weights and 1,024 sets of 64 envs:
  (a) ms per closed-loop step of rollout_mlp(T): the act kernel, the step with its sensor kernels and the fold, one call;
  (b) ms per step of the same closed loop written with step() and torch ops on the same stream: float32 addmm (baddbmm for a
      population) / relu / the head map in float64, then step().  It needs nothing of the MLP module, so it runs on a tree without it;
  (c) ms per launch of the act kernel alone (200 launches between two device events).
Windows of T steps, (a) and (b) alternated, `rounds` windows each; the median and every window are kept.  The arithmetic of (c): fmaf per
env-step and bytes per tile from the shapes and the kernel's staging constants, against the f32 vector peak and the HBM bandwidth of
MI355X_MICROARCH.md.  Writes one JSON document.
usage: mlp_policy_times.py [--envs N] [--T T] [--rounds R] [--out PATH]"""
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
from continiousenvironment_follower_leader_amd import abi, shard  # noqa: E402
from continiousenvironment_follower_leader_amd.vec_game import VecGame  # noqa: E402

try:
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
except ImportError:
    MlpPolicy = None

WIDTHS = (180, 64, 64, 2)
PEAK_F32_VECTOR_FLOPS = 157.3e12      # MI355X_MICROARCH.md: 256 CUs x 4 SIMDs x 64 FLOP per clock x 2.4 GHz
PEAK_HBM_BYTES = 8.0e12               # MI355X_MICROARCH.md: HBM3E, 8 TB/s


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
    """(b): T closed-loop steps with today's API."""
    ls = layer_views(params, WIDTHS)
    n = env.n
    for _ in range(T):
        h = env.policy_obs.view(n_sets, n // n_sets, WIDTHS[0])
        for l, (W, b) in enumerate(ls):
            h = torch.addmm(b[0], h[0], W[0])[None] if n_sets == 1 else torch.baddbmm(b[:, None, :], h, W)
            if l + 1 < len(ls):
                h = torch.relu(h)
        u = h.view(n, 2).double().clamp(-1.0, 1.0)
        env.step(torch.minimum(torch.maximum(lo + ((u + 1.0) * 0.5) * (hi - lo), lo), hi))


def arithmetic(n, n_sets):
    """The least time the act kernel could take: its fmaf against the f32 vector peak, its bytes against the HBM bandwidth."""
    fma = sum(a * b for a, b in zip(WIDTHS[:-1], WIDTHS[1:]))
    tile = getattr(abi, "FTL_MLP_ENV_TILE", None)
    r = dict(fmaf_per_env_step=fma, flop_per_launch=2 * fma * n, compute_bound_us=2 * fma * n / PEAK_F32_VECTOR_FLOPS * 1e6)
    if tile:
        eps = n // n_sets
        tiles = n_sets * ((eps + tile - 1) // tile)
        weight_bytes_per_tile = 4 * param_count(WIDTHS)
        io = n * (4 * WIDTHS[0] + 16)                              # every env's policy_obs row in, its action out
        r.update(env_tile=tile, tiles=tiles, weight_bytes_per_tile=weight_bytes_per_tile, weight_bytes_per_launch_from_l2=tiles * weight_bytes_per_tile,
                 distinct_weight_bytes=4 * param_count(WIDTHS) * n_sets, obs_and_action_bytes=io,
                 memory_bound_us=(io + 4 * param_count(WIDTHS) * n_sets) / PEAK_HBM_BYTES * 1e6)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_policy_B65536.json"))
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
    result = dict(workload="B", envs=n, widths=WIDTHS, T=T, rounds=a.rounds, mlp_module=MlpPolicy is not None,
                  method="device events around a window of T steps that ends in a device synchronise; every window from the same snapshot; "
                         "(a) and (b) alternated; median of the windows",
                  step_kernels_us=dict(source="profiles/rays_cull_kernel_stats_timed.csv, tree_p1 (one part, 65,536 envs, rocprofv3 --kernel-trace)",
                                       ftl_frames_group_kernel=159.1, ftl_rays_kernel=113.0))
    for n_sets in (1, 1024):
        g = torch.Generator(device="cpu")
        g.manual_seed(n_sets)
        params = (torch.randn(n_sets, param_count(WIDTHS), generator=g) * 0.1).to(dev)
        pol = MlpPolicy(env, WIDTHS, params=params, n_sets=n_sets) if MlpPolicy is not None else None
        times = dict(rollout_mlp=[], torch_loop=[], act=[])
        env.restore(snap, slot_stats=True)
        torch_loop(env, params, n_sets, 20, lo, hi)                                    # warm-up of every shape the windows use
        if pol is not None:
            env.restore(snap, slot_stats=True)
            env.rollout_mlp(pol, 20)
        for _ in range(a.rounds):
            if pol is not None:
                env.restore(snap, slot_stats=True)
                times["rollout_mlp"].append(timed(lambda: env.rollout_mlp(pol, T), T))
            env.restore(snap, slot_stats=True)
            times["torch_loop"].append(timed(lambda: torch_loop(env, params, n_sets, T, lo, hi), T))
            if pol is not None:
                times["act"].append(timed(lambda: [pol.act() for _ in range(200)], 200))
        r = dict(ms_per_step={k: statistics.median(v) for k, v in times.items() if v}, all_windows_ms={k: v for k, v in times.items() if v})
        b = times["torch_loop"]
        r["torch_loop_spread_ms"] = dict(min=min(b), max=max(b), spread=max(b) - min(b))
        r["arithmetic"] = ar = arithmetic(n, n_sets)
        if pol is not None:
            r["rollout_mlp_minus_torch_loop_ms"] = r["ms_per_step"]["rollout_mlp"] - r["ms_per_step"]["torch_loop"]
            r["bar_a_le_b_beyond_spread"] = bool(max(times["rollout_mlp"]) < min(b))
            act_us = r["ms_per_step"]["act"] * 1e3
            bound = max(ar["compute_bound_us"], ar.get("memory_bound_us", 0.0))
            r["act_kernel"] = dict(us_per_launch=act_us, tflops=ar["flop_per_launch"] / act_us / 1e6,
                                   share_of_f32_vector_peak=ar["compute_bound_us"] / act_us,
                                   bound="compute" if bound == ar["compute_bound_us"] else "memory", share_of_bound=bound / act_us,
                                   note="200 back-to-back launches between two device events: launch gaps included")
        result["sets_%d" % n_sets] = r
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    env.close()


if __name__ == "__main__":
    main()
