"""ftl_rays_kernel on the crafted worlds of tests/ray_edge_cases.py, HIP against the oracle: the merged and split source layout of phase 1
and more static rects inside the reach box than one, two and three wavefronts hold (group A), table lengths and class runs that end on the
last lane of a chunk (B), the follower in, on and next to rects under 12 to 256 rays in the mask and the list form, with windows of 16
pairs and with a second pass (C), every bearing under every heading (D), rects at the class-cull boxes (E), the corridor copy on both
sides of its cap (F), 1023 rays and the largest static list ftl_create accepts (G).  tests/test_ray_edges_host.py shows on the oracle
alone that each case has the shape it is built for, pins the oracle to the reference's own sensor classes there and asserts the margin
condition that makes a corner waiver impossible on these worlds -- so every case here demands that WAIVERS["corner"] does not move.
Tolerance, hitboxes and the shared counters are those of tests/test_gpu_configs.py::_compare_with_oracle."""
import numpy as np
import pytest
import torch

import ray_edge_cases as X
from continiousenvironment_follower_leader_amd import abi
from oracle_batch import OracleBatch
from test_gpu_configs import WAIVERS, _compare_with_oracle, _vec

pytestmark = pytest.mark.gpu

OUTS = ("obs_num", "lasers", "target", "reward", "done", "status")
SWITCHES = ("FTL_RAYS_ONE_PASS", "FTL_DEBUG_PAIR_WINDOW", "FTL_RAYS_CLASS_CULL", "FTL_DEBUG_CORR_LDS_CAP")


def _state_bytes(env):
    return env.state[env._state_off:env._state_off + env.lib.ftl_state_bytes(env.h)]


def _same(a, b, tag):
    for name in OUTS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (tag, name)
    assert torch.equal(_state_bytes(a), _state_bytes(b)), (tag, "state")


def _make(monkeypatch, n, cfg, pool, switches):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    env = _vec(n, cfg, pool)
    for k in switches:
        monkeypatch.delenv(k)
    return env


def _run(monkeypatch, case, look=None):
    """The case on the device against the oracle batch at the reset and after every step, and against each twin run bit for bit."""
    cfg, n, scen = case["cfg"], case["n"], case["scen"]
    pool = X.scenario_pool(cfg, scen, "cuda:0")
    env = _make(monkeypatch, n, cfg, pool, {})
    twins = [_make(monkeypatch, n, cfg, pool, sw) for sw in case["twins"]]
    idx = np.arange(n)
    ora = OracleBatch(cfg, n, env_id_base=0)         # env e draws from stream e, as on the device and in the case's trace
    ora.reset(scen, idx)
    before = WAIVERS["corner"]
    for e in [env] + twins:
        e.reset(torch.from_numpy(idx.astype(np.int32)))

    def check(tag, t):
        _compare_with_oracle(env, ora, cfg, (case["name"], tag))
        assert np.array_equal(ora.lasers[:, :cfg.lasers_len], np.stack([r[t]["lasers"] for r in case["trace"]])), (case["name"], tag, "the trace")
        for sw, tw in zip(case["twins"], twins):
            _same(env, tw, (case["name"], tag, sw))
        if look is not None:
            look(env, t)
    check("reset", 0)
    for t in range(case["steps"]):
        a = case["actions"](t)
        act = torch.tensor(a, dtype=torch.float64, device="cuda:0")
        env.step(act)
        ora.step(a)
        for tw in twins:
            tw.step(act)
        check(t, t + 1)
    assert WAIVERS["corner"] == before, (case["name"], "a corner waiver on a world that keeps every corner %g px off every ray" % X.MARGIN)
    for e in [env] + twins:
        assert e.error_report() == (0, 0), case["name"]
        assert int(e.state_field("env_int")[:, abi.EI_ERROR_STICKY].abs().max()) == 0
        e.close()


@pytest.mark.parametrize("name", X.case_names())
def test_ray_edges(monkeypatch, name):
    _run(monkeypatch, X.get_case(name))


def test_largest_static_list(monkeypatch):
    """The largest n_static ftl_create accepts for a 12-ray, one-row sensor (found by asking it), as a dense disc of rects around the
    follower; one more is refused."""
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    n, message = X.largest_n_static()
    assert "64 KiB of LDS" in message
    with pytest.raises(ValueError, match="64 KiB of LDS"):
        VecGame(X.G_DENSE_ENVS, device="cuda:0", config=X.dense_config(n + 1))
    _run(monkeypatch, X.get_case("G-dense-%d" % n))


def test_1024_rays_are_refused():
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    with pytest.raises(ValueError, match="10 bits"):
        VecGame(8, device="cuda:0", config=X.too_many_rays_config())


# ---- group F: the corridor copy -----------------------------------------------------------------------------------------------------------
# (golden episode whose config is used, config overrides, FTL_DEBUG_CORR_LDS_CAP, steps, corridor_length or None): natural worlds of the host
# generator, 32 envs.  The caps come from the window lengths of these runs: config B at one frame per step resets with 12 to 22 points and
# gains one every four steps (cap 16), config E starts at 35 to 45 and passes 64 after some 80 steps.  In those two the tracker does not
# trim within the run, so every span starts at point 0.  The third run is config B with a corridor of 60 px: the tracker trims from the
# first save on, the span over the five snapshots stays at 6 to 9 points while its first point climbs from 6-16 to 21-31, so with a copy
# of 8 points spans of 7 and 8 are staged, spans of 9 are read in place, and nearly every staged span crosses a multiple of 8 -- the
# wrap of `p & cmask` in the staging loop, the table references and the fetch of phase 3.
F_ENVS = 32
F_RUNS = {"B-fps1": ("Bfps1_s3_chase", {}, 16, 40, None), "E": ("E_s3_chase", dict(rng_seed=9, env_id_base=7000), 64, 110, None),
          "B-short": ("B_s1_chase", dict(corr_cap=256), 8, 70, 60)}


def corridor_spans(env, cfg, which=1):
    """Per env what ftl_rays_kernel stages for pass `which`: (first point, one past the last point) over the windows of the valid snapshots,
    from the device's snap_win ring ([slot][pass][lo, hi]) and its snapshot counters."""
    hmax = max(l.history for l in cfg.lasers)
    sw = env.state_field("snap_win").cpu().numpy().reshape(env.n, hmax, 2, 2)
    ei = env.state_field("env_int").cpu().numpy()
    lo, hi = np.zeros(env.n, np.int64), np.zeros(env.n, np.int64)
    for e in range(env.n):
        nsnap, head = min(int(ei[e, abi.EI_SNAP_COUNT]), hmax), int(ei[e, abi.EI_SNAP_HEAD])
        slots = [(head - 1 - a) % hmax for a in range(nsnap)]
        lo[e], hi[e] = min(sw[e, s, which, 0] for s in slots), max(sw[e, s, which, 1] for s in slots)
    return lo, hi


def run_corridor_copy(monkeypatch, run, report=None):
    from golden_util import config_for, load_episode
    from aux_edge_cases import generated_scenarios
    from test_gpu_configs import _actions
    ep, over, cap, steps, corridor_length = F_RUNS[run] if isinstance(run, str) else run
    _, meta = load_episode(ep)
    if corridor_length is not None:
        kw = dict(meta["kwargs"])
        # the corridor then lies round the leader, beyond the 100 px of config B's corridor sensor: that sensor gets rays of 220 px, so that
        # readings depend on the segments the wrap touches
        kw["follower_sensors"] = {k: dict(v, corridor_length=corridor_length) if "corridor_length" in v else
                                  dict(v, laser_length=220) if v.get("react_to_safe_corridor") else dict(v) for k, v in kw["follower_sensors"].items()}
        meta = dict(meta, kwargs=kw)
    cfg = config_for(meta, scen_route_len=256, **over)
    assert cfg.c.corr_cap >= 2 * cap and all(l.after_tracker for l in cfg.lasers), (cfg.c.corr_cap, cap)
    scen = generated_scenarios(cfg, np.arange(48))[:F_ENVS]
    pool = X.scenario_pool(cfg, scen, "cuda:0")
    env = _make(monkeypatch, F_ENVS, cfg, pool, {"FTL_DEBUG_CORR_LDS_CAP": str(cap)})
    twin = _make(monkeypatch, F_ENVS, cfg, pool, {})
    idx = np.arange(F_ENVS)
    ora = OracleBatch(cfg, F_ENVS, env_id_base=over.get("env_id_base"))
    ora.reset(scen, idx)
    for e in (env, twin):
        e.reset(torch.from_numpy(idx.astype(np.int32)))
    seen = dict(staged=0, unstaged=0, wrapped=0)

    def check(tag):
        _compare_with_oracle(env, ora, cfg, ("F", run, tag))
        _same(env, twin, ("F", run, tag, "default copy"))
        lo, hi = corridor_spans(env, cfg)
        staged = hi - lo <= cap
        seen["staged"] += int(staged.sum()); seen["unstaged"] += int((~staged).sum())
        seen["wrapped"] += int((staged & (hi > lo) & (lo // cap != (hi - 1) // cap)).sum())
        if report is not None:
            report(tag, lo, hi)
    check("reset")
    for t in range(steps):
        a = _actions(cfg, F_ENVS, t, "mixed" if t % 2 else "random", seed=51)
        act = torch.tensor(a, dtype=torch.float64, device="cuda:0")
        env.step(act); twin.step(act); ora.step(a)
        check(t)
    for e in (env, twin):
        e.close()
    return seen


@pytest.mark.parametrize("run", list(F_RUNS))
def test_corridor_copy_on_both_sides_of_its_cap(monkeypatch, run):
    """A small LDS copy of the corridor ring against the oracle and, bit for bit, against the default copy: spans that fit the copy and
    spans that do not occur in the same run, and on the short corridor staged spans cross a multiple of the cap."""
    seen = run_corridor_copy(monkeypatch, run)
    print("ray_edges F-%s: env-steps staged %d, read in place %d, staged across a multiple of the cap %d" % (run, seen["staged"], seen["unstaged"], seen["wrapped"]))
    assert seen["staged"] > 0 and seen["unstaged"] > 0, seen
    if run == "B-short":
        assert seen["wrapped"] > 0, seen
