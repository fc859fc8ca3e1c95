"""ftl_render throughput on config B (tests/golden/pool_B.npz): device-event time per render() call, averaged over a synchronised loop
after warm-up, for (a) 64 envs full size at scale 1 and (b) 1,024 envs at scale 8, rendered from a 65,536-env batch mid-episode.
Prints one JSON line.  --frames DIR also writes one scale-1 frame and a 4 x 4 grid of scale-4 thumbnails (PNG when PIL imports,
.npy otherwise).

usage: python profiles/tools/render_speed.py [--envs 65536] [--iters 50] [--frames DIR]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def save(path, img):
    try:
        from PIL import Image
        Image.fromarray(img).save(path + ".png")
    except ImportError:
        np.save(path + ".npy", img)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--frames", default=None)
    args = ap.parse_args()
    from golden_util import GOLDEN, config_for
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool, VecGame
    z = np.load(GOLDEN + "/pool_B.npz")
    meta = json.loads(str(z["meta"]))
    cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()))
    n = args.envs
    env = VecGame(n, config=cfg)
    env.load_scenarios(ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0"))
    env.reset(torch.arange(n, dtype=torch.int32) % env.pool.n)
    g = torch.Generator(device="cpu").manual_seed(0)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    for _ in range(args.steps):      # mid-episode: green zones, corridors and trajectories of some length
        v = (0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)) * ms
        w = torch.clamp(torch.randn(n, generator=g, dtype=torch.float64) * 0.3 * mr, -mr, mr)
        env.step(torch.stack([v, w], 1).contiguous().cuda(), auto_reset=True)
    torch.cuda.synchronize()
    ids64 = torch.arange(0, 64 * (n // 64), n // 64, dtype=torch.int32, device="cuda:0")[:64]
    ids1k = torch.arange(0, 1024 * max(n // 1024, 1), max(n // 1024, 1), dtype=torch.int32, device="cuda:0")[:1024] % n
    out64 = torch.empty(64, cfg.c.height, cfg.c.width, 3, dtype=torch.uint8, device="cuda:0")
    out1k = torch.empty(1024, (cfg.c.height + 7) // 8, (cfg.c.width + 7) // 8, 3, dtype=torch.uint8, device="cuda:0")
    ms64 = timed(lambda: env.render(ids64, scale=1.0, out=out64), args.iters)
    ms1k = timed(lambda: env.render(ids1k, scale=8.0, out=out1k), args.iters)
    res = dict(tool="render_speed", config="B", n_envs=n, steps_before=args.steps,
               full64_ms=round(ms64, 4), full64_target_ms=3.0, full64_mpix_s=round(64 * cfg.c.width * cfg.c.height / ms64 / 1e3, 1),
               thumb1024_s8_ms=round(ms1k, 4), thumb1024_target_ms=1.0, iters=args.iters, device=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if args.frames:
        os.makedirs(args.frames, exist_ok=True)
        save(os.path.join(args.frames, "frame_B_scale1"), env.render([int(ids64[0])], scale=1.0)[0].cpu().numpy())
        th = env.render(ids1k[:16], scale=4.0).cpu().numpy()
        h, w = th.shape[1:3]
        grid = np.full((4 * h + 3 * 4, 4 * w + 3 * 4, 3), 255, np.uint8)
        for i in range(16):
            r, c = divmod(i, 4)
            grid[r * (h + 4):r * (h + 4) + h, c * (w + 4):c * (w + 4) + w] = th[i]
        save(os.path.join(args.frames, "thumbs_B_scale4_4x4"), grid)
    env.close()


if __name__ == "__main__":
    main()
