"""What a step costs without its sensor half, on config B (tests/golden/pool_B.npz) with the aged population bench.py uses: one process,
two batch sizes -- 65,536 envs as two pipelined parts and 8,192 envs as one batch --, and per size `--reps` alternating blocks of

  step     `--steps` ordinary steps with auto-reset (what bench.py times)
  blind    the same steps with ``sensors=False``
  rollout  ``rollout`` with T = 8 (seven blind steps and one that scans, no auto-reset inside), each followed by ONE blind auto-reset step
           that restarts the envs the rollout left done, so that the population stays the aged one: 9 env-steps per iteration, all timed
  scan     `--steps` calls of ``scan()`` alone

Every block ends in a device synchronise and is timed on the host around it; a block's figure is milliseconds per step (per scan) of the
WHOLE batch.  Writes medians, minima, maxima and every block to `--out` and prints the same JSON.

usage: python profiles/tools/scan_on_demand_ab.py [--steps 200] [--reps 5] [--age 300] [--out profiles/scan_on_demand_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
T_ROLLOUT = 8


def make_actions(cfg, n, n_sets, seed, device):
    """bench.py's synthetic policy output: v ~ U[0.5, 1] * max_speed, w ~ N(0, 0.2 * max_rot) clipped to the action box, float64."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed
    v = (0.5 + 0.5 * torch.rand(n_sets, n, generator=g, dtype=torch.float64)) * ms
    w = torch.clamp(torch.randn(n_sets, n, generator=g, dtype=torch.float64) * (0.2 * mr), -mr, mr)
    return torch.stack([v, w], dim=-1).contiguous().to(device)


def measure(n, parts, steps, reps, age, seed, device):
    from golden_util import GOLDEN, config_for
    from continiousenvironment_follower_leader_amd import shard
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, ScenarioPool, VecGame
    z = np.load(os.path.join(GOLDEN, "pool_B.npz"))
    meta = json.loads(str(z["meta"]))
    cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()))
    pool = ScenarioPool.from_npz(cfg, os.path.join(GOLDEN, "pool_B.npz"), device)
    env = PipelinedVecGame(n, parts=parts, device=device, config=cfg) if parts > 1 else VecGame(n, device=device, config=cfg)
    env.load_scenarios(pool)
    env.reset(shard.scenario_index(seed, 0, n, pool.n))
    n_sets = 16
    acts = make_actions(cfg, n, n_sets, seed * 7919, device)
    seqs = [torch.stack([acts[(s + t) % n_sets] for t in range(T_ROLLOUT)]).contiguous() for s in range(n_sets)]
    k = [0]

    def nxt():
        k[0] += 1
        return k[0] % n_sets

    def block_step(sensors):
        for _ in range(steps):
            env.step(acts[nxt()], auto_reset=True, sensors=sensors)
        return steps

    def block_rollout():
        its = max(steps // (T_ROLLOUT + 1), 1)
        for _ in range(its):
            env.rollout(seqs[nxt()])
            env.step(acts[nxt()], auto_reset=True, sensors=False)
        return its * (T_ROLLOUT + 1)

    def block_scan():
        for _ in range(steps):
            env.scan()
        return steps

    modes = (("step", lambda: block_step(True)), ("blind", lambda: block_step(False)), ("rollout", block_rollout), ("scan", block_scan))

    def sync():
        if parts > 1:
            env.join()
        torch.cuda.synchronize()

    for _ in range(age):                       # ageing: untimed, as bench.py
        env.step(acts[nxt()], auto_reset=True)
    for _, run in modes:                       # every path once before it is timed (allocations of the first rollout, ...)
        run()
    sync()
    blocks = {name: [] for name, _ in modes}
    for _ in range(reps):
        for name, run in modes:
            sync()
            t0 = time.perf_counter()
            cnt = run()
            sync()
            blocks[name].append((time.perf_counter() - t0) * 1e3 / cnt)
    res = dict(n_envs=n, parts=parts, error_report=list(env.error_report()))
    for name, ms in blocks.items():
        med = statistics.median(ms)
        res[name] = dict(ms_per_step=[round(v, 5) for v in ms], median=round(med, 5), min=round(min(ms), 5), max=round(max(ms), 5),
                         menv_steps_per_s=round(n / med / 1e3, 1))
    res["blind_over_step"] = round(res["blind"]["median"] / res["step"]["median"], 4)
    res["rollout_over_step"] = round(res["rollout"]["median"] / res["step"]["median"], 4)
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_on_demand_ab.json"))
    a = ap.parse_args()
    if a.steps < 200 or a.reps < 1:
        ap.error("--steps must be at least 200 and --reps at least 1")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    device = torch.device("cuda", 0)
    res = dict(tool="scan_on_demand_ab", config="B", steps_per_block=a.steps, reps=a.reps, age_steps=a.age, rollout_T=T_ROLLOUT,
               unit="milliseconds per step (per scan) of the whole batch, host time around a block that ends in a device synchronise",
               device=torch.cuda.get_device_name(0), sizes=[measure(n, parts, a.steps, a.reps, a.age, a.seed, device) for n, parts in ((65536, 2), (8192, 1))])
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
