#!/usr/bin/env python3
"""What a critic's values on a recorded trajectory cost: float32 rows [T+1 = 33, 65,536, 180] (2.16 M rows, random normals), the net
180-64-64-1 with ReLU and with tanh hidden layers, one set of weights and 1,024 sets of 64 rows a block, from device events:
  (a) ms per call of mlp.forward (ftl_mlp_forward, one launch) into a preallocated [33, 65536, 1] buffer;
  (b) ms for the same values with torch under no_grad, as a user writes them without it: one set -- addmm over all 2.16 M rows, the
      activation, addmm, the activation, addmm; 1,024 sets -- per block baddbmm of [1024, 64, 180] with the sets' weights (a batched
      product over all blocks at once would have to copy either the rows or 33 copies of the weights), the activation, ..., into the
      same preallocated buffer.
Protocol of DESIGN.md 8.16: a warm-up of every shape, then `rounds` windows of `reps` calls each between two device events, the
variants alternated, median (min .. max) of the windows.  Also torch.cuda.max_memory_allocated above the inputs and the output buffer
during one call of each, and the largest difference between the two results.  Writes one JSON document.
usage: mlp_forward_times.py [--rows N] [--blocks B] [--reps R] [--rounds R] [--out PATH]"""
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
from mlp_policy_times import PEAK_F32_VECTOR_FLOPS, PEAK_HBM_BYTES, layer_views, timed  # noqa: E402

WIDTHS = (180, 64, 64, 1)
ACT = dict(relu=torch.relu, tanh=torch.tanh)


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), windows=v)


def torch_values(x, layers, n_sets, act, out):
    """(b): ``out`` [B, N, 1] from rows ``x`` [B, N, 180] with torch ops on views of the same parameter tensor."""
    f = ACT[act]
    with torch.no_grad():
        if n_sets == 1:
            h = x.view(-1, WIDTHS[0])
            for l, (W, b) in enumerate(layers):
                if l + 1 < len(layers):
                    h = f(torch.addmm(b[0], h, W[0]))
                else:
                    torch.addmm(b[0], h, W[0], out=out.view(-1, 1))
            return out
        per = x.shape[1] // n_sets
        for t in range(x.shape[0]):
            h = x[t].view(n_sets, per, WIDTHS[0])
            for l, (W, b) in enumerate(layers):
                if l + 1 < len(layers):
                    h = f(torch.baddbmm(b[:, None, :], h, W))
                else:
                    torch.baddbmm(b[:, None, :], h, W, out=out[t].view(n_sets, per, 1))
        return out


def peak_above(fn):
    """Bytes torch's allocator held at most during ``fn()`` above what it held before (inputs and output buffers exist already)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=33)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_forward_B65536.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, N = a.blocks, a.rows
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    x = torch.empty(B, N, WIDTHS[0], dtype=torch.float32, device=dev)
    for t in range(B):
        x[t].copy_(torch.randn(N, WIDTHS[0], generator=g))
    ya, yb = torch.empty(B, N, 1, dtype=torch.float32, device=dev), torch.empty(B, N, 1, dtype=torch.float32, device=dev)
    count = abi.mlp_param_count(WIDTHS)
    fma = sum(p * q for p, q in zip(WIDTHS[:-1], WIDTHS[1:]))
    rows = B * N
    result = dict(rows=[B, N, WIDTHS[0]], widths=WIDTHS, reps_per_window=a.reps, rounds=a.rounds,
                  method="device events around a window of `reps` calls that ends in a device synchronise; every shape warmed up first; the "
                         "variants alternated; median (min .. max) of the windows, ms per call",
                  arithmetic=dict(fmaf_per_row=fma, flop_per_call=2 * fma * rows, compute_bound_ms=2 * fma * rows / PEAK_F32_VECTOR_FLOPS * 1e3,
                                  row_bytes_in_and_out=rows * 4 * (WIDTHS[0] + 1), memory_bound_ms=rows * 4 * (WIDTHS[0] + 1) / PEAK_HBM_BYTES * 1e3,
                                  hidden_activation_bytes_per_layer_if_materialised=rows * 64 * 4))
    for act in ("relu", "tanh"):
        for n_sets in (1, 1024):
            params = (torch.randn(n_sets, count, generator=g) * 0.1).to(dev)
            layers = layer_views(params, WIDTHS)

            def fa():
                mlp.forward(WIDTHS, params, x, act, out=ya)

            def fb():
                torch_values(x, layers, n_sets, act, yb)

            fa(), fb(), fa(), fb()                                       # warm-up of every shape
            torch.cuda.synchronize()
            diff = float((ya - yb).abs().max())
            mem = dict(forward=peak_above(fa), torch=peak_above(fb))
            times = dict(forward=[], torch=[])
            for _ in range(a.rounds):
                times["forward"].append(timed(lambda: [fa() for _ in range(a.reps)], a.reps))
                times["torch"].append(timed(lambda: [fb() for _ in range(a.reps)], a.reps))
            med = statistics.median(times["forward"])
            bound = max(result["arithmetic"]["compute_bound_ms"], result["arithmetic"]["memory_bound_ms"])
            result["%s_sets_%d" % (act, n_sets)] = dict(
                ms_per_call={k: spread(v) for k, v in times.items()},
                bar_forward_slowest_below_torch_fastest=bool(max(times["forward"]) < min(times["torch"])),
                peak_bytes_above_inputs_and_outputs=mem, max_abs_difference_of_the_values=diff,
                forward_tflops=2 * fma * rows / med / 1e9, forward_share_of_bound=bound / med,
                bound="compute" if bound == result["arithmetic"]["compute_bound_ms"] else "memory")
            del params, layers
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
