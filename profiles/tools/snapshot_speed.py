"""ftl_pack_envs / ftl_unpack_envs speed on config B (tests/golden/pool_B.npz): device-event time per call, averaged over a
synchronised loop after warm-up, from a 65,536-env batch mid-episode.  Measured in the same process: a torch device-to-device copy_
of the same byte count (the yardstick of a full-batch pack), the full-batch unpack, and the search case -- one env cloned into 4,096
slots -- both as the two kernels alone and as the whole VecGame.clone call (host id checks included).  Prints one JSON line.

usage: python profiles/tools/snapshot_speed.py [--envs 65536] [--iters 30] [--clones 4096]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--clones", type=int, default=4096)
    args = ap.parse_args()
    from golden_util import GOLDEN, config_for
    from continiousenvironment_follower_leader_amd import _lib, abi
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
    for _ in range(args.steps):      # mid-episode state (the copy does not depend on it; the numbers are for a realistic batch)
        v = (0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)) * ms
        w = torch.clamp(torch.randn(n, generator=g, dtype=torch.float64) * 0.3 * mr, -mr, mr)
        env.step(torch.stack([v, w], 1).contiguous().cuda(), auto_reset=True)
    torch.cuda.synchronize()
    lib, B = env.lib, env.env_bytes
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    rows = torch.empty(n, B, dtype=torch.uint8, device="cuda:0")
    nbytes = n * B
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0"), torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    src.fill_(1)

    def pack():
        _lib.check(lib.ftl_pack_envs(env.h, ids.data_ptr(), n, rows.data_ptr(), stream()), lib)

    def unpack():
        _lib.check(lib.ftl_unpack_envs(env.h, rows.data_ptr(), ids.data_ptr(), n, abi.FTL_ENV_SLOT_STATS, stream()), lib)

    res = dict(tool="snapshot_speed", config="B", n_envs=n, env_bytes=B, bytes=nbytes, steps_before=args.steps, iters=args.iters)
    # interleaved A / B / A / B rounds: the three figures see the same clocks
    t_pack, t_copy, t_unpack = [], [], []
    for _ in range(3):
        t_pack.append(timed(pack, args.iters))
        t_copy.append(timed(lambda: dst.copy_(src), args.iters))
        t_unpack.append(timed(unpack, args.iters))
    res["pack_ms"] = round(min(t_pack), 4)
    res["torch_copy_ms"] = round(min(t_copy), 4)
    res["unpack_ms"] = round(min(t_unpack), 4)
    res["pack_over_copy"] = round(min(t_pack) / min(t_copy), 3)
    res["pack_over_copy_target"] = 1.2
    res["pack_read_write_tb_s"] = round(2 * nbytes / (min(t_pack) * 1e-3) / 1e12, 3)
    res["copy_read_write_tb_s"] = round(2 * nbytes / (min(t_copy) * 1e-3) / 1e12, 3)
    # search case: env 0 into slots 1 .. K
    k = args.clones
    one = torch.zeros(k, dtype=torch.int32, device="cuda:0")
    dsts = torch.arange(1, k + 1, dtype=torch.int32, device="cuda:0")
    tmp = torch.empty(k, B, dtype=torch.uint8, device="cuda:0")

    def clone_kernels():
        _lib.check(lib.ftl_pack_envs(env.h, one.data_ptr(), k, tmp.data_ptr(), stream()), lib)
        _lib.check(lib.ftl_unpack_envs(env.h, tmp.data_ptr(), dsts.data_ptr(), k, 0, stream()), lib)

    res["clone_1_to_%d_kernels_ms" % k] = round(timed(clone_kernels, args.iters), 4)
    src_ids, dst_ids = np.zeros(k, np.int64), np.arange(1, k + 1)
    env.clone(src_ids, dst_ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        env.clone(src_ids, dst_ids)
    torch.cuda.synchronize()
    res["clone_1_to_%d_vecgame_ms" % k] = round((time.perf_counter() - t0) * 1e3 / args.iters, 4)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
