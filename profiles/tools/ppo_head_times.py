#!/usr/bin/env python3
"""What the loss head of a PPO epoch costs on a recorded trajectory: float32 heads [T = 32, 65,536, 2] (2.10 M rows, random normals, about
3 % of the rows FTL_TR_VOID), one set of weights and 1,024 sets of 64 rows a block, from device events:
  (a) ms per mlp.ppo_head call (ftl_ppo_head: four launches) into reused outputs: dhead, dvalue, dlog_std and the stats table;
  (b) ms for the same gradients from torch ops under autograd in float32, as INTEGRATION.md wrote the loss head before ppo_loss: from
      `head` and `value` tensors that require grad to head.grad, value.grad and log_std.grad -- one set with boolean-mask indexing, 1,024
      sets with views [T, 1024, 64(, 2)] and masked per-member means;
  (c) ms per mlp.ppo_loss(...).backward(), the autograd form of (a), for information.
Protocol of DESIGN.md 8.20: a warm-up of every shape, then `rounds` windows of `reps` calls each between two device events, the variants
alternated, median (min .. max) of the windows.  Also the largest difference between the gradients of (a) and (b).  Writes one JSON
document.
usage: ppo_head_times.py [--rows N] [--blocks B] [--reps R] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from continiousenvironment_follower_leader_amd import abi, mlp  # noqa: E402
from mlp_forward_times import spread  # noqa: E402
from mlp_policy_times import timed  # noqa: E402

HALF_LOG_2PI = 0.9189385332


def torch_head(head, value, log_std, z, logp_old, adv, ret, m, n_sets):
    """(b): the loss of INTEGRATION.md's example under autograd; leaves head.grad, value.grad and log_std.grad."""
    head.grad = value.grad = log_std.grad = None
    if n_sets == 1:
        sigma = log_std.exp()
        logp = (-0.5 * ((z - head) / sigma) ** 2 - sigma.log() - HALF_LOG_2PI).sum(-1)
        ratio = (logp - logp_old).exp()
        a = (adv - adv[m].mean()) / (adv[m].std() + 1e-8)
        loss = (-torch.min(ratio * a, ratio.clamp(0.8, 1.2) * a) + 0.5 * 0.5 * (value - ret) ** 2)[m].mean()
    else:
        T, S = head.shape[0], n_sets
        mf = m.view(T, S, -1).float()
        cnt = mf.sum((0, 2))
        av = adv.view(T, S, -1)
        mean = ((av * mf).sum((0, 2)) / cnt)[None, :, None]
        std = ((((av - mean) ** 2) * mf).sum((0, 2)) / (cnt - 1)).sqrt()[None, :, None]
        a = (av - mean) / (std + 1e-8)
        sigma = log_std.exp()                                  # [S, 1, 2]
        logp = (-0.5 * ((z.view(T, S, -1, 2) - head.view(T, S, -1, 2)) / sigma) ** 2 - sigma.log() - HALF_LOG_2PI).sum(-1)
        ratio = (logp - logp_old.view(T, S, -1)).exp()
        rows = -torch.min(ratio * a, ratio.clamp(0.8, 1.2) * a) + 0.5 * 0.5 * (value.view(T, S, -1) - ret.view(T, S, -1)) ** 2
        loss = ((rows * mf).sum((0, 2)) / cnt).sum()
    loss.backward()
    return head.grad, value.grad, log_std.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_head_B65536.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T, N, A = a.blocks, a.rows, 2
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    head_old, noise, adv, ret = rnd(T, N, A), rnd(T, N, A), rnd(T, N), rnd(T, N)
    head_new = head_old + 0.1 * rnd(T, N, A)
    value_new = ret + 0.3 * rnd(T, N)
    kind = torch.where(torch.rand(T, N, generator=g) < 0.03, abi.FTL_TR_VOID, abi.FTL_TR_STEP).to(torch.uint8).to(dev)
    m = kind != abi.FTL_TR_VOID
    result = dict(rows=[T, N, A], void_fraction=float((~m).float().mean()), reps_per_window=a.reps, rounds=a.rounds, segment_rows=abi.FTL_PPO_SEG,
                  method="device events around a window of `reps` calls that ends in a device synchronise; every shape warmed up first; the "
                         "variants alternated; median (min .. max) of the windows, ms per call",
                  not_measured="the four kernels on their own (no profiler run), other row counts, head width 1, a call without the value part, "
                               "other segment lengths")
    for n_sets in (1, 1024):
        log_std_old = (-1.0 + 0.2 * torch.randn(n_sets, A, generator=g)).to(dev)
        log_std = (log_std_old + 0.05 * torch.randn(n_sets, A, generator=g).to(dev)).requires_grad_()
        sigma_old = log_std_old.exp()
        traj = mlp.Trajectory(None, head_old, None, None, kind, noise, sigma_old)
        out = mlp.PpoHead(torch.empty_like(head_new), torch.empty_like(value_new), torch.empty(n_sets, A, device=dev),
                          torch.empty(n_sets, abi.FTL_PPO_STATS, dtype=torch.float64, device=dev))
        # (b)'s inputs, as the example prepares them once per iteration
        so = sigma_old if n_sets == 1 else sigma_old.repeat_interleave(N // n_sets, 0)
        z = head_old + so * noise
        logp_old = (-0.5 * noise ** 2 - so.log() - HALF_LOG_2PI).sum(-1)
        th, tv = head_new.clone().requires_grad_(), value_new.clone().requires_grad_()
        tl = (log_std.detach().clone() if n_sets == 1 else log_std.detach().clone().view(n_sets, 1, A)).requires_grad_()
        hl, vl = head_new.clone().requires_grad_(), value_new.clone().requires_grad_()

        def fa():
            ls = log_std.detach()
            return mlp.ppo_head(head_new, head_old, noise, sigma_old, ls.exp(), adv, ret, kind, value_new, ls - log_std_old, out=out)

        def fb():
            return torch_head(th, tv, tl, z, logp_old, adv, ret, m, n_sets)

        def fc():
            hl.grad = vl.grad = log_std.grad = None
            mlp.ppo_loss(traj, hl, log_std, adv, ret, vl, log_std_old).backward()

        fa(), fb(), fc(), fa(), fb(), fc()                       # warm-up of every shape
        torch.cuda.synchronize()
        ra, (gh, gv, gl) = fa(), fb()
        diff = dict(dhead=float((ra.dhead - gh).abs().max()), dvalue=float((ra.dvalue - gv).abs().max()),
                    dlog_std=float((ra.dlog_std - gl.view(n_sets, A)).abs().max()), max_abs_dhead=float(gh.abs().max()))
        times = dict(ppo_head=[], torch=[], ppo_loss_backward=[])
        for _ in range(a.rounds):
            times["ppo_head"].append(timed(lambda: [fa() for _ in range(a.reps)], a.reps))
            times["torch"].append(timed(lambda: [fb() for _ in range(a.reps)], a.reps))
            times["ppo_loss_backward"].append(timed(lambda: [fc() for _ in range(a.reps)], a.reps))
        med = statistics.median(times["ppo_head"])
        result["sets_%d" % n_sets] = dict(
            ms_per_call={k: spread(v) for k, v in times.items()},
            bar_ppo_head_slowest_below_torch_fastest=bool(max(times["ppo_head"]) < min(times["torch"])),
            max_abs_difference_of_the_gradients=diff,
            # 3 x 8 + 3 x 4 + 1 bytes read, 8 + 4 written a row; the advantages and kinds are read twice (the moments pass)
            ppo_head_gbytes_per_s_of_54_bytes_a_row=54 * T * N / med / 1e6)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
