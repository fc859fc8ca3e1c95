#!/usr/bin/env python3
"""What the guided search costs and what it buys, beside the action search and the baseline follower, on bench.py's workload B (the
captured pool) on one GPU.  Measured, not asserted.

Cost: n real envs 8 baseline steps into their episodes, K candidates, horizon T, hold, tail 0 / 8 / 32, iters 1 and 3 -- milliseconds per
``GuidedSearch.act()`` as the median of ``--blocks`` blocks of ``--reps`` calls, each block ending in a device synchronise; beside it
``ActionSearch.act()`` at the same n, K, T measured the same way in the same process (copied into a checkout of the parent commit the
script runs there too, ``--only cost``, and reports that column alone: the class it measures does not exist there), and the milliseconds
of the guided fan-out kernel alone (device events around ``ftl_guided_fanout``) times the rounds, as a share of the call.

Quality: one fixed list of ``--scenarios`` scenarios (``(7 i) mod P``) played once each with ``evaluate(policy, sensors=False)`` on
``--slots`` slots, gamma 1, by ``BaselineFollower``, ``ActionSearch`` and ``GuidedSearch`` at tail 0 / 8 / 32 (iters 1; tail 8 also with
iters 3): mean return, successes, crashes, mean frames.  ``--config F`` plays the same table on the golden config F (speed regimes, random
frames per step; a generated pool) with ``own_stream`` False and True, where the two differ.

Writes one JSON file (default profiles/guided_search_ab.json) and prints it.
usage: guided_search_ab.py [--envs 1024] [--K 64] [--T 8] [--hold 2] [--blocks 5] [--reps 4] [--scenarios 256] [--slots 256]
                           [--only cost|quality|f] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (build_workload: the workload bench.py measures)
from continiousenvironment_follower_leader_amd import _lib, abi, shard  # noqa: E402
from continiousenvironment_follower_leader_amd.baseline import BaselineFollower  # noqa: E402
from continiousenvironment_follower_leader_amd.search import ActionSearch  # noqa: E402
from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool, VecGame  # noqa: E402

try:
    from continiousenvironment_follower_leader_amd.search import GuidedSearch  # noqa: E402
except ImportError:                                            # the parent commit's tree: the ActionSearch column only
    GuidedSearch = None

TAILS = (0, 8, 32)


def _blocks(fn, a):
    ms = []
    for _ in range(a.blocks):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / a.reps)
    return dict(ms=statistics.median(ms), ms_blocks=ms)


def cost(cfg, pool, dev, a):
    env = VecGame(a.envs, device=dev, config=cfg)
    env.load_scenarios(pool)
    env.reset(shard.scenario_index(0, 0, a.envs, pool.n))
    follower = BaselineFollower(env)
    for _ in range(8):                                         # under way, on the baseline's actions
        env.step(follower.act(), sensors=False)
    rows = follower.state.clone()
    out = {}
    for iters in (1, 3):
        s = ActionSearch(env, a.K, a.T, hold=a.hold, iters=iters)
        s.act()
        torch.cuda.synchronize()
        out["action_search_iters_%d" % iters] = _blocks(s.act, a)
        s.close()
        if GuidedSearch is None:
            continue
        for tail in TAILS:
            g = GuidedSearch(env, a.K, a.T, tail, hold=a.hold, iters=iters)

            def act():
                g.follower.state.copy_(rows)                   # every call decides from the same follower rows (a 1 MB device copy)
                g.act()
            act()
            torch.cuda.synchronize()
            r = _blocks(act, a)
            st, fan = env._stream(), []
            for _ in range(a.blocks * a.reps):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                _lib.check(g.lib.ftl_guided_fanout(env.h, g.clones.h, a.K, env._out_ref, g.clones._out_ref, g.follower.state.data_ptr(),
                                                   a.envs * g.row, g.clone_state.data_ptr(), a.envs * a.K * g.row, g.cap, st), g.lib)
                ev1.record()
                torch.cuda.synchronize()
                fan.append(ev0.elapsed_time(ev1))
            r.update(fanout_ms=statistics.median(fan) * iters, fanout_share=statistics.median(fan) * iters / r["ms"], blind_steps=iters * (a.T + tail),
                     clones=a.envs * a.K, best_ret_mean=float(g.best_ret.mean()), best_k_nonzero=int(g.best_k.ne(0).sum()))
            out["guided_tail_%d_iters_%d" % (tail, iters)] = r
            g.close()
    env.close()
    return out


def quality(cfg, pool, dev, a, owns=(False,)):
    scen = (torch.arange(a.scenarios) * 7) % pool.n

    def play(make):
        env = VecGame(a.slots, device=dev, config=cfg)
        env.load_scenarios(pool)
        policy = make(env)
        t0 = time.perf_counter()
        recs = env.evaluate(policy, scen, sensors=False)
        sec = time.perf_counter() - t0
        if hasattr(policy, "close"):
            policy.close()
        env.close()
        return dict(mean_return=float(recs["ret"].mean()), success=int((recs["status"][:, 0] == abi.MISSION.index("success")).sum()),
                    crash=int((recs["status"][:, 1] == abi.AGENT.index("crash")).sum()), mean_frames=float(recs["frames"].mean()),
                    seconds=sec)
    out = dict(scenarios=a.scenarios, slots=a.slots, pool=pool.n, baseline=play(BaselineFollower))
    for own in owns:
        tag = "_own_stream" if own else ""
        out["action_search_iters_1" + tag] = play(lambda env: ActionSearch(env, a.K, a.T, hold=a.hold, iters=1, own_stream=own))
        if GuidedSearch is None:
            continue
        for tail, iters in [(t, 1) for t in TAILS] + [(8, 3)]:
            out["guided_tail_%d_iters_%d%s" % (tail, iters, tag)] = play(
                lambda env: GuidedSearch(env, a.K, a.T, tail, hold=a.hold, iters=iters, own_stream=own))
    return out


def config_f(dev):
    """The golden config F (speed regimes, random frames per step) and a generated pool of 64 seeds, as the GPU tests build them."""
    from golden_util import config_for, load_episode
    _, meta = load_episode("F_s1_chase")
    cfg = config_for(meta, scen_route_len=256)
    return cfg, ScenarioPool.generate(cfg, np.arange(64), str(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--T", type=int, default=8)
    ap.add_argument("--hold", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--scenarios", type=int, default=256)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_search_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg, pool, _, _, _ = bench.build_workload("B", 0, 0, dev)
    result = dict(workload="B", device=torch.cuda.get_device_name(dev), envs=a.envs, K=a.K, T=a.T, hold=a.hold, gamma=1.0, spread=1.0, decay=0.5,
                  library=os.environ.get("FTL_LIB", "this tree"))
    if a.only in ("", "cost"):
        result["cost"] = cost(cfg, pool, dev, a)
    if a.only in ("", "quality"):
        result["quality"] = quality(cfg, pool, dev, a)
    if a.only in ("", "f"):
        fcfg, fpool = config_f(dev)
        result["quality_config_F"] = quality(fcfg, fpool, dev, a, owns=(False, True))
    text = json.dumps(result, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
