"""Worlds per second of the two scenario generators on config B, this tree against another build of the library, interleaved.

One child process per (library, round): `--rounds` rounds of both libraries, the order swapped from round to round; a child warms up, then times
--reps launches of ftl_generate_scenarios_device (HIP events around the launch) and --reps calls of ftl_generate_scenarios on --threads threads
(host clock), each over the same --seeds seeds of config B, and prints one JSON line.  The driver prints every line and, per library and
generator, all values with min / median / max.  Also compares the status bytes of the two libraries.
Usage: python profiles/tools/scenario_planner_cap_ab.py --other variants_parent.so [--out FILE]      (profiles/tools/build_ref_variant.sh)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def child(a):
    import hashlib
    import numpy as np
    import torch
    from golden_util import GOLDEN, config_for
    from continiousenvironment_follower_leader_amd.scenario import _DeviceGenerator, generate_scenarios
    z = np.load(os.path.join(GOLDEN, "pool_B.npz"))
    cfg = config_for(dict(kwargs=json.loads(str(z["meta"]))["kwargs"], post=None), scen_route_len=int(z["route_len"].max()))
    n = a.seeds
    g = _DeviceGenerator(cfg, n, "cuda:0")
    seeds = torch.arange(n, dtype=torch.int64, device="cuda:0")
    dev, usable = [], 0
    for r in range(a.reps + 2):                      # two warm-up launches (code object load, first touch of the workspace)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = g.run(seeds)
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            dev.append(n / (e0.elapsed_time(e1) * 1e-3))
    status = out["status"].cpu().numpy()
    usable = int(out["usable"].sum())
    host = []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        h = generate_scenarios(cfg, np.arange(n), n_threads=a.threads)
        if r >= 1:
            host.append(n / (time.perf_counter() - t0))
    assert np.array_equal(h["status"], status)
    print(json.dumps(dict(lib=a.child, seeds=n, usable=usable, status_sha1=hashlib.sha1(status.tobytes()).hexdigest()[:16],
                          device_worlds_per_s=[round(x) for x in dev], host_worlds_per_s=[round(x) for x in host], host_threads=a.threads)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None, help="the library to compare with (a build of another revision)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--seeds", type=int, default=16384)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    libs = [("other", os.path.abspath(a.other))] if a.other else []
    libs.append(("tree", None))
    recs = {k: [] for k, _ in libs}
    for rnd in range(a.rounds):
        for name, path in (libs if rnd % 2 == 0 else libs[::-1]):
            env = dict(os.environ)
            if path:
                env["FTL_LIB"] = path
            else:
                env.pop("FTL_LIB", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--seeds", str(a.seeds),
                                "--threads", str(a.threads)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                say("round %d %s: exit status %d\n%s" % (rnd, name, r.returncode, r.stderr[-2000:]))
                return 1                                  # nothing more is started on the GPU after a failed child
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            recs[name].append(rec)
            say("round %d %s" % (rnd, json.dumps(rec)))
    for key in ("device_worlds_per_s", "host_worlds_per_s"):
        for name, _ in libs:
            v = sorted(x for rec in recs[name] for x in rec[key])
            say("%-20s %-5s n=%d min %d median %d max %d" % (key, name, len(v), v[0], v[len(v) // 2], v[-1]))
        for name, _ in libs:                             # per process: the medians, whose spread is the run-to-run spread
            m = [sorted(rec[key])[len(rec[key]) // 2] for rec in recs[name]]
            say("%-20s %-5s per-process medians %s" % (key, name, m))
    say("status bytes: " + ", ".join("%s %s (%d usable)" % (n, recs[n][0]["status_sha1"], recs[n][0]["usable"]) for n, _ in libs))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
