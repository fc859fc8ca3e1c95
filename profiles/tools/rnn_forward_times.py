#!/usr/bin/env python3
"""What a recurrent net on a recorded sequence costs: records of 32 blocks (the actor's replay, head 2, previous action and reward) and
33 blocks (a critic with memory, head 1, previous reward) x 65,536 rows of 180 floats, the net 180-64-64 with a 64-unit cell, one set
of weights and 1,024 sets of 64 rows, random kinds (a quarter VOID), from device events:
  (a) ms per call of rnn.forward (ftl_rnn_forward, one launch) into preallocated buffers;
  (b) ms for the torch loop of INTEGRATION.md's recurrent example under no_grad on the same tensors: per block the trunk, the cell, the
      head and the zero rule.  One set: addmm for the trunk and torch.nn.LSTMCell (torch's fused cell); 1,024 sets: baddbmm on views of
      the same parameter tensor and the gates written out with sigmoid / tanh.
Protocol of DESIGN.md 8.16 / 8.20: a warm-up of every shape, then `rounds` windows of `reps` calls each between two device events that
end in a device synchronise, the variants alternated, median (min .. max) of the windows.  Also the largest difference between the two
results.  Writes one JSON document.
usage: rnn_forward_times.py [--rows N] [--reps R] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from continiousenvironment_follower_leader_amd import abi, rnn  # noqa: E402
from mlp_policy_times import layer_views, timed  # noqa: E402

TRUNK, CELL, W0 = (180, 64, 64), 64, 180


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), windows=v)


def views(params, widths, flags):
    """(trunk layers, W_g, b_g, W_y, b_y) of a [sets, count] tensor in the layout of ftl_rnn."""
    P, R, U, S = abi.rnn_widths(widths, CELL, flags)
    A = widths[-1]
    off = abi.mlp_param_count(widths[:-1])
    Wg = params[:, off:off + U * 4 * CELL].view(-1, U, 4 * CELL); off += U * 4 * CELL
    bg = params[:, off:off + 4 * CELL]; off += 4 * CELL
    Wy = params[:, off:off + CELL * A].view(-1, CELL, A); off += CELL * A
    return layer_views(params, widths[:-1]), Wg, bg, Wy, params[:, off:off + A]


def torch_loop(rec, v, n_sets, P, out, lstm=None):
    """(b): the heads ``out`` [B, N, A] of the record with torch ops, the state zeroed after every VOID row."""
    layers, Wg, bg, Wy, by = v
    obs, action, reward, kind = rec
    B, N = obs.shape[:2]
    C = CELL
    with torch.no_grad():
        h = torch.zeros(N, C, device=obs.device)
        c = torch.zeros(N, C, device=obs.device)
        a_prev = torch.zeros(N, P, device=obs.device)
        live = torch.zeros(N, 1, device=obs.device)
        r_prev = torch.zeros(N, 1, device=obs.device)
        per = N // n_sets
        for t in range(B):
            if n_sets == 1:
                x = obs[t]
                for W, b in layers:
                    x = torch.relu(torch.addmm(b[0], x, W[0]))
                h, c = lstm(torch.cat([x, a_prev, r_prev], 1), (h, c))
                torch.addmm(by[0], h, Wy[0], out=out[t])
            else:
                x = obs[t].view(n_sets, per, -1)
                for W, b in layers:
                    x = torch.relu(torch.baddbmm(b[:, None, :], x, W))
                u = torch.cat([x, a_prev.view(n_sets, per, -1), r_prev.view(n_sets, per, 1), h.view(n_sets, per, C)], 2)
                z = torch.baddbmm(bg[:, None, :], u, Wg).view(N, 4 * C)
                c = torch.sigmoid(z[:, C:2 * C]) * c + torch.sigmoid(z[:, :C]) * torch.tanh(z[:, 2 * C:3 * C])
                h = torch.sigmoid(z[:, 3 * C:]) * torch.tanh(c)
                torch.baddbmm(by[:, None, :], h.view(n_sets, per, C), Wy, out=out[t].view(n_sets, per, -1))
            if t + 1 < B:
                keep = (kind[t] != abi.FTL_TR_VOID)[:, None].float()
                h, c, live = h * keep, c * keep, keep
                if P:
                    a_prev = action[t].float() * keep
                r_prev = reward[t].float()[:, None] * keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnn_forward_B65536.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, T = a.rows, 32
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    obs = torch.empty(T + 1, N, W0, dtype=torch.float32, device=dev)
    for t in range(T + 1):
        obs[t].copy_(torch.randn(N, W0, generator=g))
    action = torch.randn(T, N, 2, generator=g, dtype=torch.float64).to(dev)
    reward = torch.randn(T, N, generator=g, dtype=torch.float64).to(dev)
    kind = torch.randint(0, 4, (T, N), generator=g, dtype=torch.uint8).to(dev)
    result = dict(rows=N, trunk=TRUNK, cell=CELL, reps_per_window=a.reps, rounds=a.rounds,
                  method="device events around a window of `reps` calls that ends in a device synchronise; every shape warmed up first; the "
                         "variants alternated; median (min .. max) of the windows, ms per call",
                  reference_ms_per_decision_of_ftl_rnn_kernel=dict(sets_1=0.336, sets_1024=0.407))
    for name, A, flags, B in (("actor_head2_B32", 2, 3, T), ("critic_head1_B33", 1, 2, T + 1)):
        widths = TRUNK + (A,)
        P, R, U, S = abi.rnn_widths(widths, CELL, flags)
        count = abi.rnn_param_count(widths, CELL, flags)
        ya, yb = torch.empty(B, N, A, dtype=torch.float32, device=dev), torch.empty(B, N, A, dtype=torch.float32, device=dev)
        x = obs[:B]
        for n_sets in (1, 1024):
            params = (torch.randn(n_sets, count, generator=g) * 0.1).to(dev)
            v = views(params, widths, flags)
            lstm = None
            if n_sets == 1:
                lstm = torch.nn.LSTMCell(U - CELL, CELL).to(dev)
                with torch.no_grad():
                    lstm.weight_ih.copy_(v[1][0, :U - CELL].t()), lstm.weight_hh.copy_(v[1][0, U - CELL:].t())
                    lstm.bias_ih.copy_(v[2][0]), lstm.bias_hh.zero_()

            def fa():
                rnn.forward(widths, CELL, params, x, action if P else None, reward, kind, None, None, bool(P), True, out=ya)

            def fb():
                torch_loop((x, action, reward, kind), v, n_sets, P, yb, lstm)

            fa(), fb(), fa(), fb()                                       # warm-up of every shape
            torch.cuda.synchronize()
            diff = float((ya - yb).abs().max())
            times = dict(forward=[], torch=[])
            for _ in range(a.rounds):
                times["forward"].append(timed(lambda: [fa() for _ in range(a.reps)], a.reps))
                times["torch"].append(timed(lambda: [fb() for _ in range(a.reps)], a.reps))
            med = statistics.median(times["forward"])
            result["%s_sets_%d" % (name, n_sets)] = dict(
                blocks=B, head=A, flags=flags, ms_per_call={k: spread(w) for k, w in times.items()},
                forward_ms_per_block=med / B, torch_ms_per_block=statistics.median(times["torch"]) / B,
                bar_forward_slowest_below_torch_fastest=bool(max(times["forward"]) < min(times["torch"])),
                max_abs_difference_of_the_heads=diff)
            del params, v, lstm
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
