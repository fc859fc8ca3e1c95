#!/usr/bin/env python3
"""What the gradient of a recurrent net on a recorded trajectory costs: float32 rows [T = 32, 65,536, 180] (2.10 M rows, random normals)
with a quarter of the kinds VOID, random recorded actions and rewards and a random head gradient; the net 180-64-64 with a 64-unit cell,
head 2 fed the last action and reward (the actor) and head 1 fed the last reward (the critic), one set of weights and 1,024 sets of 64
rows a block, from device events:
  (a) ms per forward + backward through rnn.Net (ftl_rnn_forward, then ftl_rnn_backward: three launches), params.grad freshly written;
  (b) ms for the same gradient from torch autograd in float32 through the replay a user writes without (a): one set -- addmm trunk and
      torch.nn.LSTMCell on all rows of a block, block after block; 1,024 sets -- a baddbmm chain per block (trunk, gate product, head) on
      views of one parameter tensor, the cell lines written out.
Protocol of DESIGN.md 8.21 / 8.22: a warm-up of every shape, then `rounds` windows of `reps` calls each between two device events, the
variants alternated, median (min .. max) of the windows.  Also torch.cuda.max_memory_allocated above the inputs during one call of each,
the cached workspace of (a), and the largest difference between the two gradients.  Writes one JSON document.
usage: rnn_backward_times.py [--rows N] [--blocks B] [--reps R] [--rounds R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from continiousenvironment_follower_leader_amd import abi, mlp, rnn  # noqa: E402
from mlp_forward_times import peak_above, spread  # noqa: E402
from mlp_policy_times import layer_views, timed  # noqa: E402

VOID = abi.FTL_TR_VOID


def views(params, widths, cell, flags):
    """The views of a [sets, count] tensor in the layout of ftl_rnn: trunk layers, (W_g, b_g), (W_y, b_y)."""
    U = abi.rnn_widths(widths, cell, flags)[2]
    off, A = abi.mlp_param_count(widths[:-1]), widths[-1]
    Wg, bg = params[:, off:off + U * 4 * cell].view(-1, U, 4 * cell), params[:, off + U * 4 * cell:off + (U + 1) * 4 * cell]
    off += (U + 1) * 4 * cell
    return layer_views(params, widths[:-1]), (Wg, bg), (params[:, off:off + cell * A].view(-1, cell, A), params[:, off + cell * A:off + (cell + 1) * A])


def replay_modules(seq, mods, dy, cell, P, R):
    """(b), one set: the replay of the integration guide's earlier form -- nn.Sequential trunk, nn.LSTMCell, nn.Linear -- under autograd."""
    trunk, lstm, head = mods
    obs, action, reward, kind = seq
    N = obs.shape[1]
    h = c = torch.zeros(N, cell, device=obs.device)
    a_prev, live = torch.zeros(N, P, device=obs.device), torch.zeros(N, 1, device=obs.device)
    for q in (q for m in mods for q in m.parameters()):
        q.grad = None
    loss = 0.0
    for t in range(obs.shape[0]):
        parts = [trunk(obs[t]), a_prev]
        if R:
            parts.append((reward[t - 1].float()[:, None] * (live != 0)) if t else torch.zeros(N, 1, device=obs.device))
        h, c = lstm(torch.cat(parts, 1), (h, c))
        loss = loss + (head(h) * dy[t]).sum()
        if t + 1 < obs.shape[0]:
            keep = (kind[t] != VOID)[:, None].float()
            h, c, live = h * keep, c * keep, keep
            if P:
                a_prev = action[t].float().view(N, -1)[:, :P] * keep
    loss.backward()
    lins = [m for m in trunk if isinstance(m, torch.nn.Linear)]
    g = [torch.cat([lin.weight.grad.t().reshape(-1), lin.bias.grad]) for lin in lins]
    g += [torch.cat([lstm.weight_ih.grad.t(), lstm.weight_hh.grad.t()]).reshape(-1), lstm.bias_ih.grad,
          torch.cat([head.weight.grad.t().reshape(-1), head.bias.grad])]
    return torch.cat(g)[None]


def replay_population(seq, params, v, dy, cell, P, R, n_sets):
    """(b), a population: per block a baddbmm chain over the sets' weights, the cell lines written out, under autograd."""
    layers, (Wg, bg), (Wy, by) = v
    obs, action, reward, kind = seq
    N, per = obs.shape[1], obs.shape[1] // n_sets
    params.grad = None
    h = c = torch.zeros(n_sets, per, cell, device=obs.device)
    a_prev, live = torch.zeros(n_sets, per, P, device=obs.device), torch.zeros(n_sets, per, 1, device=obs.device)
    loss = 0.0
    for t in range(obs.shape[0]):
        x = obs[t].view(n_sets, per, -1)
        for W, b in layers:
            x = torch.relu(torch.baddbmm(b[:, None, :], x, W))
        parts = [x, a_prev]
        if R:
            parts.append((reward[t - 1].float().view(n_sets, per, 1) * (live != 0)) if t else torch.zeros(n_sets, per, 1, device=obs.device))
        z = torch.baddbmm(bg[:, None, :], torch.cat(parts + [h], 2), Wg)
        i, f, g, o = z.split(cell, 2)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        loss = loss + (torch.baddbmm(by[:, None, :], h, Wy) * dy[t].view(n_sets, per, -1)).sum()
        if t + 1 < obs.shape[0]:
            keep = (kind[t] != VOID).view(n_sets, per, 1).float()
            h, c, live = h * keep, c * keep, keep
            if P:
                a_prev = action[t].float().view(n_sets, per, -1)[:, :, :P] * keep
    loss.backward()
    return params.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnn_backward_B65536.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, N, W0, cell = a.blocks, a.rows, 180, 64
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    obs = torch.empty(B, N, W0, dtype=torch.float32, device=dev)
    for t in range(B):
        obs[t].copy_(torch.randn(N, W0, generator=g))
    kind = (torch.rand(B - 1, N, generator=g) < 0.25).to(torch.uint8).mul_(VOID).to(dev)
    reward = torch.randn(B - 1, N, generator=g, dtype=torch.float64).to(dev)
    result = dict(rows=[B, N, W0], cell=cell, void_fraction=float((kind == VOID).float().mean()), reps_per_window=a.reps, rounds=a.rounds,
                  span_pairs=abi.FTL_RNN_BWD_SPAN,
                  method="device events around a window of `reps` calls that ends in a device synchronise; every shape warmed up first; the "
                         "variants alternated; median (min .. max) of the windows, ms per call of forward + backward",
                  not_measured="the stored-gates form of the reverse sweep (only the recompute form exists), the kernels on their own (no profiler "
                               "run), other row counts, block counts and nets, the optimizer step")
    for A, flags in ((2, abi.FTL_RNN_PREV_ACTION | abi.FTL_RNN_PREV_REWARD), (1, abi.FTL_RNN_PREV_REWARD)):
        widths = (W0, 64, 64, A)
        P, R, U, S = abi.rnn_widths(widths, cell, flags)
        count = abi.rnn_param_count(widths, cell, flags)
        action = torch.randn(B - 1, N, 2, generator=g, dtype=torch.float64).to(dev) if A == 2 else None
        dy = torch.empty(B, N, A, dtype=torch.float32, device=dev)
        for t in range(B):
            dy[t].copy_(torch.randn(N, A, generator=g))
        seq = (obs, action, reward, kind)
        for n_sets in (1, 1024):
            start = torch.randn(n_sets, count, generator=g) * 0.1
            net = rnn.Net(widths, cell, n_sets=n_sets, prev_action=bool(P), prev_reward=bool(R), params=start.to(dev))
            tparams = start.to(dev).requires_grad_()
            v = views(tparams, widths, cell, flags)
            mods = None
            if n_sets == 1:
                trunk = torch.nn.Sequential(torch.nn.Linear(W0, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU()).to(dev)
                lstm, head = torch.nn.LSTMCell(U - cell, cell).to(dev), torch.nn.Linear(cell, A).to(dev)
                with torch.no_grad():
                    for lin, (W, b) in zip(trunk[::2], v[0]):
                        lin.weight.copy_(W[0].t()), lin.bias.copy_(b[0])
                    lstm.weight_ih.copy_(v[1][0][0, :U - cell].t()), lstm.weight_hh.copy_(v[1][0][0, U - cell:].t())
                    lstm.bias_ih.copy_(v[1][1][0]), lstm.bias_hh.zero_()
                    head.weight.copy_(v[2][0][0].t()), head.bias.copy_(v[2][1][0])
                mods = (trunk, lstm, head)

            def fa():
                net.params.grad = None
                net(seq).backward(dy)
                return net.params.grad

            def fb():
                return replay_modules(seq, mods, dy, cell, P, R) if n_sets == 1 else replay_population(seq, tparams, v, dy, cell, P, R, n_sets)

            fa(), fb(), fa(), fb()                                   # warm-up of every shape
            torch.cuda.synchronize()
            ga, gb = fa(), fb()
            diff, scale = float((ga - gb).abs().max()), float(gb.abs().max())
            del ga, gb
            mem = dict(net=peak_above(fa), torch=peak_above(fb))
            workspace = max(t.numel() * 4 for key, t in mlp._WORKSPACE.items() if key[0] == "rnn_backward")
            times = dict(net=[], torch=[])
            for _ in range(a.rounds):
                times["net"].append(timed(lambda: [fa() for _ in range(a.reps)], a.reps))
                times["torch"].append(timed(lambda: [fb() for _ in range(a.reps)], a.reps))
            result["180-64-64-c%d-%d_sets_%d" % (cell, A, n_sets)] = dict(
                ms_per_call={k: spread(t) for k, t in times.items()},
                bar_net_slowest_below_torch_fastest=bool(max(times["net"]) < min(times["torch"])),
                peak_bytes_above_inputs=mem, cached_workspace_bytes=workspace, max_abs_difference_of_the_gradients=diff, max_abs_gradient=scale)
            print(json.dumps({k: result[k] for k in list(result)[-1:]}), flush=True)
            del net, tparams, v, mods
            mlp._WORKSPACE.clear()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
