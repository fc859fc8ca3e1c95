#!/usr/bin/env python3
"""What the gradient of a net on a recorded trajectory costs: float32 rows [T = 32, 65,536, 180] (2.10 M rows, random normals) with a
random head gradient dy, the nets 180-64-64-2 and 180-64-64-1 with ReLU and with tanh hidden layers, one set of weights and 1,024 sets of
64 rows a block, from device events:
  (a) ms per forward + backward through mlp.Net (ftl_mlp_forward, then ftl_mlp_backward: three launches), params.grad freshly written;
  (b) ms for the same gradient from torch autograd in float32, as a user writes it without (a): one set -- the nn.Sequential of
      mlp.torch_module on all 2.10 M rows; 1,024 sets -- per block a baddbmm chain of [1024, 64, 180] rows with the sets' weights under
      autograd, the blocks' gradients accumulated by autograd.
Protocol of DESIGN.md 8.20: a warm-up of every shape, then `rounds` windows of `reps` calls each between two device events, the variants
alternated, median (min .. max) of the windows.  Also torch.cuda.max_memory_allocated above the inputs during one call of each, and the
largest difference between the two gradients.  Writes one JSON document.
usage: mlp_backward_times.py [--rows N] [--blocks B] [--reps R] [--rounds R] [--out PATH]"""
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
from mlp_forward_times import peak_above, spread  # noqa: E402
from mlp_policy_times import PEAK_F32_VECTOR_FLOPS, layer_views, timed  # noqa: E402

ACT = dict(relu=torch.relu, tanh=torch.tanh)


def torch_grad(x, dy, module, layers, params, n_sets, act):
    """(b): d sum(dy * head) / d params with torch autograd; returns the gradient in the layout of ``params``."""
    if n_sets == 1:
        for q in module.parameters():
            q.grad = None
        module(x.view(-1, x.shape[-1])).backward(dy.view(-1, dy.shape[-1]))
        return torch.cat([torch.cat([lin.weight.grad.t().reshape(-1), lin.bias.grad]) for lin in module[::2]])[None]
    params.grad = None
    f, per = ACT[act], x.shape[1] // n_sets
    for t in range(x.shape[0]):
        h = x[t].view(n_sets, per, -1)
        for l, (W, b) in enumerate(layers):
            h = torch.baddbmm(b[:, None, :], h, W)
            if l + 1 < len(layers):
                h = f(h)
        h.backward(dy[t].view(n_sets, per, -1))
    return params.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_backward_B65536.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, N, W0 = a.blocks, a.rows, 180
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    x = torch.empty(B, N, W0, dtype=torch.float32, device=dev)
    for t in range(B):
        x[t].copy_(torch.randn(N, W0, generator=g))
    rows = B * N
    result = dict(rows=[B, N, W0], reps_per_window=a.reps, rounds=a.rounds, span_tiles=abi.FTL_MLP_BWD_SPAN,
                  method="device events around a window of `reps` calls that ends in a device synchronise; every shape warmed up first; the "
                         "variants alternated; median (min .. max) of the windows, ms per call of forward + backward",
                  not_measured="the kernels on their own (no profiler run), other row counts, wider nets, the optimizer step")
    for widths in ((W0, 64, 64, 2), (W0, 64, 64, 1)):
        count = abi.mlp_param_count(widths)
        fma = sum(p * q for p, q in zip(widths[:-1], widths[1:]))
        dy = torch.empty(B, N, widths[-1], dtype=torch.float32, device=dev)
        for t in range(B):
            dy[t].copy_(torch.randn(N, widths[-1], generator=g))
        for act in ("relu", "tanh"):
            for n_sets in (1, 1024):
                start = torch.randn(n_sets, count, generator=g) * 0.1
                net = mlp.Net(widths, n_sets=n_sets, activation=act, params=start.to(dev))
                tparams = start.to(dev).requires_grad_()
                layers = layer_views(tparams, widths)
                module = mlp.torch_module(widths, act, start[0]).to(dev) if n_sets == 1 else None

                def fa():
                    net.params.grad = None
                    net(x).backward(dy)
                    return net.params.grad

                def fb():
                    return torch_grad(x, dy, module, layers, tparams, n_sets, act)

                fa(), fb(), fa(), fb()                                   # warm-up of every shape
                torch.cuda.synchronize()
                ga, gb = fa(), fb()
                diff, scale = float((ga - gb).abs().max()), float(gb.abs().max())
                del ga, gb
                mem = dict(net=peak_above(fa), torch=peak_above(fb))
                times = dict(net=[], torch=[])
                for _ in range(a.rounds):
                    times["net"].append(timed(lambda: [fa() for _ in range(a.reps)], a.reps))
                    times["torch"].append(timed(lambda: [fb() for _ in range(a.reps)], a.reps))
                med = statistics.median(times["net"])
                result["%s_%s_sets_%d" % ("-".join(map(str, widths)), act, n_sets)] = dict(
                    ms_per_call={k: spread(v) for k, v in times.items()},
                    bar_net_slowest_below_torch_fastest=bool(max(times["net"]) < min(times["torch"])),
                    peak_bytes_above_inputs=mem, max_abs_difference_of_the_gradients=diff, max_abs_gradient=scale,
                    # forward, recomputed hidden layers, delta products and weight gradients: about 4 x the forward's products, less the head's recomputation
                    net_tflops_of_6_flop_per_weight_and_row=6 * fma * rows / med / 1e9,
                    compute_bound_ms_of_that=6 * fma * rows / PEAK_F32_VECTOR_FLOPS * 1e3)
                del net, tparams, layers, module
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
