#!/usr/bin/env python3
"""What a recurrent policy in the loop costs on bench.py's workload B (65,536 envs, the captured pool, net 180-64-64, LSTM cell 64, head
2, previous action and reward fed to the cell), from device events, every window from the same snapshot so that all of them do the same
work; one set of weights and 1,024 sets of 64 envs:
  (a) ms per closed-loop step of rollout_rnn(T): the recurrent kernel, the step with its sensor kernels and the fold, one call;
  (b) ms per step of the loop a user writes without it, on the same stream: float32 addmm (baddbmm for a population) / relu, cat of the
      cell input, the gate product, sigmoid / tanh, the cell update, the head and its map in float64, the state zeroed where the env
      was done on entry, then step();
  (c) ms per launch of the recurrent kernel alone (200 launches between two device events);
  (d) ms per step of collect_rnn(32) (with its randn) against its torch loop: (b) with noise, step(auto_reset="next_step") and copy_ of
      policy_obs, head, action, reward, done and the mission status into preallocated [T, N, ...] buffers.
Windows alternated, `rounds` windows each after a warm-up of every shape; the median and every window are kept.  Writes one JSON document.
usage: rnn_policy_times.py [--envs N] [--T T] [--Tc T] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402  (build_workload: the workload bench.py measures)
from continiousenvironment_follower_leader_amd import abi, rnn, shard  # noqa: E402
from continiousenvironment_follower_leader_amd.vec_game import VecGame  # noqa: E402
from mlp_policy_times import PEAK_F32_VECTOR_FLOPS, PEAK_HBM_BYTES, timed  # noqa: E402

WIDTHS, CELL = (180, 64, 64, 2), 64


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), windows=v)


class TorchLoop:
    """(b) and (d)'s reference: the recurrent net with torch ops on the policy's own parameter views."""

    def __init__(self, env, pol, lo, hi):
        self.env, self.pol, self.lo, self.hi = env, pol, lo, hi
        self.sets, self.per = pol.n_sets, env.n // pol.n_sets
        self.trunk = [pol.layer(l) for l in range(len(pol.trunk) - 1)]
        self.cell, self.head = pol.cell_weights(), pol.head_weights()
        dev, n, C = env.device, env.n, pol.cell
        self.h, self.c = torch.zeros(self.sets, self.per, C, device=dev), torch.zeros(self.sets, self.per, C, device=dev)
        self.a_prev, self.live = torch.zeros(self.sets, self.per, 2, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)

    def _mm(self, b, x, W):
        return torch.addmm(b[0], x[0], W[0])[None] if self.sets == 1 else torch.baddbmm(b[:, None, :], x, W)

    def decide(self, done_in, noise=None, sigma=None):
        env, C = self.env, self.pol.cell
        x = env.policy_obs.view(self.sets, self.per, WIDTHS[0])
        for W, b in self.trunk:
            x = torch.relu(self._mm(b, x, W))
        r_prev = torch.where(self.live, env.reward.float(), 0.0).view(self.sets, self.per, 1)
        z = self._mm(self.cell[1], torch.cat([x, self.a_prev, r_prev, self.h], 2), self.cell[0])
        i, f, g, o = torch.sigmoid(z[..., :C]), torch.sigmoid(z[..., C:2 * C]), torch.tanh(z[..., 2 * C:3 * C]), torch.sigmoid(z[..., 3 * C:])
        c = f * self.c + i * g
        h = o * torch.tanh(c)
        y = self._mm(self.head[1], h, self.head[0]).view(env.n, 2)
        u = y.double() if noise is None else y.double() + sigma * noise.double()
        u = u.clamp(-1.0, 1.0)
        a = torch.minimum(torch.maximum(self.lo + ((u + 1.0) * 0.5) * (self.hi - self.lo), self.lo), self.hi)
        keep = (~done_in).view(self.sets, self.per, 1)                # mode AFTER: the decision at a finished env is void, its row zeroed
        self.h, self.c, self.a_prev = h * keep, c * keep, a.float().view(self.sets, self.per, 2) * keep
        self.live = ~done_in
        return y, a

    def rollout(self, T):
        env = self.env
        done = env.state_field("env_int")[:, abi.EI_DONE].ne(0)
        for _ in range(T):
            _, a = self.decide(done)
            env.step(a)
            done = done | env.done.bool()

    def collect(self, T, sigma, buf):
        env, n = self.env, self.env.n
        sg = sigma.double().repeat_interleave(self.per, 0)
        done = env.state_field("env_int")[:, abi.EI_DONE].ne(0)
        for t in range(T):
            buf["obs"][t].copy_(env.policy_obs.view(n, -1))
            torch.randn(n, 2, out=buf["noise"][t])
            y, a = self.decide(done, buf["noise"][t], sg)
            buf["head"][t].copy_(y)
            buf["action"][t].copy_(a)
            env.step(a, auto_reset="next_step")
            buf["reward"][t].copy_(env.reward)
            buf["done"][t].copy_(env.done)
            buf["mission"][t].copy_(env.status[:, 0])
            done = env.done.bool()
        buf["obs"][T].copy_(env.policy_obs.view(n, -1))


def arithmetic(pol, n):
    """The least time the recurrent kernel could take: its fmaf against the f32 vector peak, its bytes against the HBM bandwidth."""
    w = pol.trunk
    fma = sum(a * b for a, b in zip(w[:-1], w[1:])) + pol.U * 4 * pol.cell + pol.cell * pol.widths[-1]
    io = n * (4 * w[0] + 16 + 8 + 2 * 4 * pol.S)                      # policy_obs row and reward in, action out, the state row in and out
    weights = 4 * pol.param_count * pol.n_sets
    return dict(fmaf_per_env_step=fma, flop_per_launch=2 * fma * n, transcendentals_per_env_step=5 * pol.cell,
                compute_bound_us=2 * fma * n / PEAK_F32_VECTOR_FLOPS * 1e6, obs_action_state_bytes=io, distinct_weight_bytes=weights,
                memory_bound_us=(io + weights) / PEAK_HBM_BYTES * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--Tc", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnn_policy_B65536.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg, pool, _, _, _ = bench.build_workload("B", 0, 0, dev)
    n, T, Tc = a.envs, a.T, a.Tc
    env = VecGame(n, device=dev, config=cfg, policy_obs=True)
    env.load_scenarios(pool)
    env.reset(shard.scenario_index(0, 0, n, pool.n))
    snap = env.snapshot()
    lo = torch.tensor(cfg.action_low, dtype=torch.float64, device=dev)
    hi = torch.tensor(cfg.action_high, dtype=torch.float64, device=dev)
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    buf = dict(obs=torch.empty(Tc + 1, n, WIDTHS[0], dtype=f32, device=dev), head=torch.empty(Tc, n, 2, dtype=f32, device=dev),
               noise=torch.empty(Tc, n, 2, dtype=f32, device=dev), action=torch.empty(Tc, n, 2, dtype=f64, device=dev),
               reward=torch.empty(Tc, n, dtype=f64, device=dev), done=torch.empty(Tc, n, dtype=u8, device=dev),
               mission=torch.empty(Tc, n, dtype=u8, device=dev))
    noise = torch.empty(Tc, n, 2, dtype=f32, device=dev)
    result = dict(workload="B", envs=n, widths=WIDTHS, cell=CELL, prev_action=True, prev_reward=True, T=T, T_collect=Tc, rounds=a.rounds,
                  method="device events around a window that ends in a device synchronise; every window from the same snapshot and a zeroed "
                         "policy state; the variants alternated; median (min .. max) of the windows")
    for n_sets in (1, 1024):
        g = torch.Generator(device="cpu")
        g.manual_seed(n_sets)
        count = abi.rnn_param_count(WIDTHS, CELL, 3)
        params = (torch.randn(n_sets, count, generator=g) * 0.1).to(dev)
        sigma = torch.full((n_sets, 2), 0.3, dtype=f32, device=dev)
        pol = rnn.RecurrentPolicy(env, WIDTHS, CELL, n_sets=n_sets, params=params)
        traj = [None]

        def fresh():
            env.restore(snap, slot_stats=True)
            pol.reset_state()
            return TorchLoop(env, pol, lo, hi)

        def collect():
            torch.randn(Tc, n, 2, out=noise)
            traj[0] = env.collect_rnn(pol, Tc, noise, sigma, out=traj[0])

        fresh().rollout(20)                                            # warm-up of every shape the windows use
        fresh().collect(Tc, sigma, buf)
        fresh(), env.rollout_rnn(pol, 20)
        fresh(), collect()
        times = dict(rollout_rnn=[], torch_loop=[], act=[], collect_rnn=[], torch_collect=[])
        for _ in range(a.rounds):
            fresh()
            times["rollout_rnn"].append(timed(lambda: env.rollout_rnn(pol, T), T))
            loop = fresh()
            times["torch_loop"].append(timed(lambda: loop.rollout(T), T))
            times["act"].append(timed(lambda: [pol.act() for _ in range(200)], 200))
            fresh()
            times["collect_rnn"].append(timed(collect, Tc))
            loop = fresh()
            times["torch_collect"].append(timed(lambda: loop.collect(Tc, sigma, buf), Tc))
        r = dict(ms_per_step={k: spread(v) for k, v in times.items()},
                 bar_rollout_slowest_below_torch_fastest=bool(max(times["rollout_rnn"]) < min(times["torch_loop"])),
                 bar_collect_slowest_below_torch_fastest=bool(max(times["collect_rnn"]) < min(times["torch_collect"])))
        r["arithmetic"] = ar = arithmetic(pol, n)
        act_us = statistics.median(times["act"]) * 1e3
        bound = max(ar["compute_bound_us"], ar["memory_bound_us"])
        r["act_kernel"] = dict(us_per_launch=act_us, tflops=ar["flop_per_launch"] / act_us / 1e6, share_of_f32_vector_peak=ar["compute_bound_us"] / act_us,
                               bound="compute" if bound == ar["compute_bound_us"] else "memory", share_of_bound=bound / act_us,
                               note="200 back-to-back launches between two device events: launch gaps included")
        result["sets_%d" % n_sets] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    env.close()


if __name__ == "__main__":
    main()
