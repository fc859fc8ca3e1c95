"""Scenario supply: how fast fresh worlds can be made, and what they cost the step rate (DESIGN row f2).

Writes ONE JSON record (stdout, and --out FILE):
  generator: usable worlds/s of ftl_generate_scenarios_device alone on configs B and D (--gen-seeds seeds per launch, the best of
             --gen-reps launches, HIP events), beside the host generator's rate (ftl_generate_scenarios on --host-threads threads) in the
             same run;
  stepping:  env-steps/s of PipelinedVecGame(--envs, parts=2) on config B three ways in one process -- the fixed 1,280-world pool, the host
             ScenarioRing (2 x --host-half), a DeviceScenarioRing (--segments x --segment) -- with the worlds that went live and the resets
             (episodes ended) inside the timed region, and resets per world.
Usage: python profiles/tools/scenario_supply.py [--out FILE]"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from golden_util import GOLDEN, config_for, load_episode  # noqa: E402
from continiousenvironment_follower_leader_amd import abi  # noqa: E402
from continiousenvironment_follower_leader_amd.scenario import (DeviceScenarioRing, ScenarioRing, _DeviceGenerator,  # noqa: E402
                                                                generate_scenarios)
from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, ScenarioPool  # noqa: E402


def cfg_b(route_len=None, **over):
    z = np.load(os.path.join(GOLDEN, "pool_B.npz"))
    meta = json.loads(str(z["meta"]))
    return config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=route_len or int(z["route_len"].max()), **over)


def cfg_d():
    _, m = load_episode("D_s2_chase")
    return config_for(m, scen_route_len=256)


def gen_rate(cfg, n, reps, host_threads, host_n, device):
    g = _DeviceGenerator(cfg, n, device)
    best = None
    for r in range(reps + 1):                 # launch 0: warm-up (code object load, first touch of the workspace)
        seeds = torch.arange(r * n, (r + 1) * n, dtype=torch.int64, device=device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = g.run(seeds)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        usable = int(out["usable"].sum())
        if r > 0 and (best is None or usable / ms > best[0] / best[1]):
            best = (usable, ms)
    t0 = time.perf_counter()
    h = generate_scenarios(cfg, np.arange(10 ** 7, 10 ** 7 + host_n), n_threads=host_threads)
    th = time.perf_counter() - t0
    return dict(seeds_per_launch=n, device_ms=round(best[1], 3), device_usable=best[0],
                device_usable_per_s=round(best[0] / best[1] * 1e3), host_threads=host_threads, host_seeds=host_n,
                host_s=round(th, 3), host_usable_per_s=round(int(h["usable"].sum()) / th),
                speedup=round((best[0] / best[1] * 1e3) / (int(h["usable"].sum()) / th), 2))


def stepping(mode, a, device):
    cfg = cfg_b()                 # one config for the three modes (route_cap = the fixed pool's longest route, at least 128)
    n = a.envs
    env = PipelinedVecGame(n, parts=2, device=device, config=cfg)
    ring = None
    if mode == "fixed":
        pool = ScenarioPool.from_npz(cfg, os.path.join(GOLDEN, "pool_B.npz"), device)
        env.load_scenarios(pool)
        env.reset((torch.arange(n) % pool.n).to(torch.int32))
    elif mode == "host_ring":
        threads = max(1, min(len(os.sched_getaffinity(0)), 16) - 2)
        ring = ScenarioRing(cfg, a.host_half, device, itertools.count(1000003), n_threads=threads)
        ring.attach(env)
        env.reset((torch.arange(n) % a.host_half).to(torch.int32))
    else:
        ring = DeviceScenarioRing(cfg, a.segment, device, segments=a.segments, seed_base=1000003)
        ring.attach(env)
        env.reset((torch.arange(n) % a.segment).to(torch.int32))
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    acts = [torch.stack([(0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)) * ms,
                         torch.clamp(torch.randn(n, generator=g, dtype=torch.float64) * 0.2 * mr, -mr, mr)], 1).to(device) for _ in range(8)]
    k = 0
    for _ in range(a.age):
        if ring is not None:
            ring.poll(env, k)
        env.step(acts[k % 8], auto_reset=True)
        k += 1
    env.join()
    torch.cuda.synchronize()
    ep0 = int(env.state_field("env_int")[:, abi.EI_EPISODES].sum())
    gen0 = ring.generated if ring is not None else 0
    swaps0 = ring.swaps if ring is not None else 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.steps):
        if ring is not None:
            ring.poll(env, k)
        env.step(acts[k % 8], auto_reset=True)
        k += 1
    env.join()
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev_s = e0.elapsed_time(e1) / 1e3
    resets = int(env.state_field("env_int")[:, abi.EI_EPISODES].sum()) - ep0
    worlds = (ring.generated - gen0) if ring is not None else 0
    err = env.error_report()
    rec = dict(mode=mode, envs=n, steps=a.steps, env_steps_per_s=round(n * a.steps / dev_s), wall_env_steps_per_s=round(n * a.steps / wall),
               resets=resets, worlds=worlds, window_moves=(ring.swaps - swaps0) if ring is not None else 0,
               resets_per_world=round(resets / worlds, 2) if worlds else None, errors=list(err))
    if mode == "host_ring":
        rec["ring"] = "ScenarioRing 2 x %d" % a.host_half
        ring.close()
    elif mode == "device_ring":
        rec["ring"] = "DeviceScenarioRing %d x %d, horizon %d steps, %d generator launches in all" % (a.segments, a.segment, ring.horizon, ring.launches)
        rec["seeds_per_world"] = round(ring.seeds_used / max(ring.generated, 1), 3)
        ring.close()
    env.close()
    del env, ring
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--gen-seeds", type=int, default=16384)
    ap.add_argument("--gen-reps", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-seeds", type=int, default=8192)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--age", type=int, default=600)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--host-half", type=int, default=16384)
    ap.add_argument("--segment", type=int, default=65536)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--skip-stepping", action="store_true")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    rec = dict(tool="profiles/tools/scenario_supply.py", device=torch.cuda.get_device_name(0),
               generator=dict(B=gen_rate(cfg_b(), a.gen_seeds, a.gen_reps, a.host_threads, a.host_seeds, device),
                              D=gen_rate(cfg_d(), a.gen_seeds, a.gen_reps, a.host_threads, a.host_seeds // 2, device)))
    if not a.skip_stepping:
        rec["stepping"] = [stepping(m, a, device) for m in ("fixed", "host_ring", "device_ring")]
        f = rec["stepping"][0]["env_steps_per_s"]
        for r in rec["stepping"]:
            r["vs_fixed"] = round(r["env_steps_per_s"] / f, 4)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
