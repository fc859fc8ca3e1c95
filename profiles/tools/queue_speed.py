"""Cost of a step under the episode queue on config B (tests/golden/pool_B.npz): device events around `--calls` calls of
``step(policy(obs), auto_reset=MODE)`` after warm-up, the chase rule on ``obs_num`` as the policy (computed on the device inside the timed
loop), one batch of `--envs` envs with the final buffers.  MODE "queue" attaches a queue long enough not to drain; MODE "same_step" is
the yardstick.  One process measures one mode, `--reps` windows of it; `--root` picks the source tree, so that the same tool times
"same_step" on a checkout of the parent commit (which has no queue).  Prints one JSON line.

usage: python profiles/tools/queue_speed.py --mode queue|same_step [--root TREE] [--envs 65536] [--calls 400] [--warmup 50] [--reps 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["queue", "same_step"], required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from golden_util import GOLDEN, config_for
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool, VecGame
    z = np.load(GOLDEN + "/pool_B.npz")
    meta = json.loads(str(z["meta"]))
    cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()))
    n = args.envs
    env = VecGame(n, config=cfg, final_obs=True)
    env.load_scenarios(ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0"))
    ms, mr, md = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed, cfg.c.min_distance

    def chase(x):
        x = x.double()
        dx, dy = x[:, 0] - x[:, 5], x[:, 1] - x[:, 6]
        want = torch.remainder(torch.rad2deg(torch.atan2(dy, dx)), 360.0)
        err = torch.remainder(want - x[:, 8] + 540.0, 360.0) - 180.0
        dist = torch.sqrt(dx * dx + dy * dy)
        v = torch.where(dist > md * 2.4, torch.full_like(dist, ms), torch.where(dist < md * 1.5, torch.zeros_like(dist), torch.full_like(dist, 0.9 * ms)))
        return torch.stack([v, torch.clamp(err * 0.3, -mr, mr)], 1).contiguous()

    scen = torch.arange(n, dtype=torch.int32) % env.pool.n
    total = args.warmup + args.reps * args.calls
    if args.mode == "queue":
        q = env.set_episode_queue((torch.arange(n * 8) % env.pool.n).to(torch.int32))
        env.reset_from_queue()
    else:
        q = None
        env.reset(scen)
    for _ in range(args.warmup):
        env.step(chase(env.obs_num), auto_reset=args.mode)
    torch.cuda.synchronize()
    times, ended = [], 0
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cnt = torch.zeros((), dtype=torch.int64, device="cuda:0")
        a.record()
        for _ in range(args.calls):
            env.step(chase(env.obs_num), auto_reset=args.mode)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / args.calls)
        ended += int(cnt)
    m = env.episode_metrics().cpu().tolist()
    res = dict(tool="queue_speed", config="B", mode=args.mode, n_envs=n, calls=args.calls, warmup=args.warmup,
               ms_per_call=[round(t, 5) for t in times], ms_per_call_min=round(min(times), 5), episodes_ended=int(m[0]), calls_total=total,
               device=torch.cuda.get_device_name(0))
    if q is not None:
        res["queue_len"], res["queue_finished"], res["queue_head"] = q.n, int(q.finished()), int(q.head)
        assert int(q.head) < q.n, "the queue drained inside the timed region"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
