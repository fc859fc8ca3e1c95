"""Cost of a step under the scenario sampler on config B (tests/golden/pool_B.npz): device events around `--calls` calls of
``step(policy(obs), auto_reset=MODE)``, the chase rule on ``obs_num`` as the policy (computed on the device inside the timed loop), one
batch of `--envs` envs with the final buffers, after `--age` untimed calls (bench.py's ageing: the timed windows see the steady-state mix
of episode ages).  MODE "sample" attaches a sampler over the whole pool with weights 1 .. count, a third of them zero; MODE "queue" a
queue long enough not to drain; MODE "same_step" is the yardstick.  One process measures one mode, `--reps` windows of it; `--root`
picks the source tree, so that the same tool times "same_step" and "queue" on a checkout of the parent commit (which has no sampler).
MODE "scan" times ``ftl_sampler_refresh`` alone at `--counts` weights (device events around `--calls` launches).  Prints one JSON line.

usage: python profiles/tools/sampler_speed.py --mode sample|queue|same_step|scan [--root TREE] [--envs 65536] [--calls 400] [--age 300]
       [--reps 3] [--counts 1105,70001]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["sample", "queue", "same_step", "scan"], required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--counts", default="1105,70001")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from golden_util import GOLDEN, config_for
    from continiousenvironment_follower_leader_amd import _lib
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool, VecGame
    z = np.load(GOLDEN + "/pool_B.npz")
    meta = json.loads(str(z["meta"]))
    cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()))
    n = args.envs if args.mode != "scan" else 64
    env = VecGame(n, config=cfg, final_obs=True)
    env.load_scenarios(ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0"))
    res = dict(tool="sampler_speed", config="B", mode=args.mode, tag=args.tag, device=torch.cuda.get_device_name(0))

    if args.mode == "scan":
        from continiousenvironment_follower_leader_amd import ScenarioSampler
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        res["scan_us"] = {}
        for count in [int(c) for c in args.counts.split(",")]:
            s = ScenarioSampler(count, device="cuda:0")
            s.set_raw_weights(torch.arange(1, count + 1, dtype=torch.int64))
            c = s.c_struct()          # (straight through the C-ABI: a window larger than the pool may be refreshed, not sampled from)
            _lib.check(env.lib.ftl_set_scenario_sampler(env.h, C.byref(c)), env.lib)
            for _ in range(20):
                _lib.check(env.lib.ftl_sampler_refresh(env.h, stream), env.lib)
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    _lib.check(env.lib.ftl_sampler_refresh(env.h, stream), env.lib)
                b.record()
                torch.cuda.synchronize()
                times.append(round(a.elapsed_time(b) / args.calls * 1e3, 3))
            assert int(s.cdf[-1]) == count * (count + 1) // 2
            res["scan_us"][str(count)] = times      # per launch, back to back on one stream (launch gaps included)
        print(json.dumps(res))
        return

    ms, mr, md = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed, cfg.c.min_distance

    def chase(x):
        x = x.double()
        dx, dy = x[:, 0] - x[:, 5], x[:, 1] - x[:, 6]
        want = torch.remainder(torch.rad2deg(torch.atan2(dy, dx)), 360.0)
        err = torch.remainder(want - x[:, 8] + 540.0, 360.0) - 180.0
        dist = torch.sqrt(dx * dx + dy * dy)
        v = torch.where(dist > md * 2.4, torch.full_like(dist, ms), torch.where(dist < md * 1.5, torch.zeros_like(dist), torch.full_like(dist, 0.9 * ms)))
        return torch.stack([v, torch.clamp(err * 0.3, -mr, mr)], 1).contiguous()

    q = smp = None
    if args.mode == "queue":
        q = env.set_episode_queue((torch.arange(n * 16) % env.pool.n).to(torch.int32))
        env.reset_from_queue()
    elif args.mode == "sample":
        from continiousenvironment_follower_leader_amd import ScenarioSampler
        smp = ScenarioSampler(env.pool.n, device="cuda:0")
        w = torch.arange(1, env.pool.n + 1, dtype=torch.int64)
        w[1::3] = 0
        smp.set_raw_weights(w)
        env.set_scenario_sampler(smp)
        env.reset_from_sampler()
    else:
        env.reset(torch.arange(n, dtype=torch.int32) % env.pool.n)
    for _ in range(args.age):
        env.step(chase(env.obs_num), auto_reset=args.mode)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            env.step(chase(env.obs_num), auto_reset=args.mode)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / args.calls)
    m = env.episode_metrics().cpu().tolist()
    best = min(times)
    res.update(n_envs=n, calls=args.calls, age=args.age, ms_per_call=[round(t, 5) for t in times], ms_per_call_min=round(best, 5),
               steps_per_s=[round(n / t * 1e3) for t in times], episodes_ended=int(m[0]), calls_total=args.age + args.reps * args.calls)
    if q is not None:
        res["queue_len"], res["queue_head"] = q.n, int(q.head)
        assert int(q.head) < q.n, "the queue drained inside the timed region"
    if smp is not None:
        t = smp.table()
        res["table_episodes"], res["scenarios_visited"] = int(t["episodes"].sum()), int((t["episodes"] > 0).sum())
        assert int(t["episodes"][1::3].sum()) == 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
