"""Phase 1 of the ray kernel culls each segment class against the reach of the sensors of the pass that react to it, and pushes nothing
of a class no sensor sees (ftl_device.hpp: cls_reach; FTL_RAYS_CLASS_CULL=0 at ftl_create restores one box of the pass's longest laser
for every class and skips nothing).  The cull only drops what phase 3 would drop for every sensor, so every output and every state
byte equals the twin's with the cull off, and the oracle's readings.
Every case: config B's world, 256 envs x 40 steps from the recorded pool (env e starts from entry 3e mod n), against the oracle batch at
reset and after every step, no error bits.  The non-vacuity counts are taken on the oracle's newest row, summed over the 40 steps."""
import numpy as np
import pytest
import torch

from golden_util import GOLDEN, config_for, load_episode
from oracle_batch import OracleBatch, pool_scenarios
from test_gpu_configs import _actions, _compare_with_oracle, _vec
from test_gpu_rays_emission import _same

pytestmark = pytest.mark.gpu

TRACKER = "LeaderPositionsTracker_v2"
ALL, OBST = "LeaderCorridor_lasers_all", "LeaderCorridor_lasers_obstacles"      # 12 rays / 100 px, 24 rays / 150 px
N, STEPS = 256, 40
SWITCHES = ("FTL_RAYS_CLASS_CULL", "FTL_RAYS_ONE_PASS", "FTL_DEBUG_PAIR_WINDOW", "FTL_DEBUG_CORR_LDS_CAP")
FLOOR = 100          # readings a non-vacuity condition asks for (the counts observed on the CPU are given with each case)
CULL_OFF = {"FTL_RAYS_CLASS_CULL": "0"}


def _b_config(reacts=None, lengths=None, order=(TRACKER, ALL, OBST)):
    """Config B's world.  `reacts`: per ray sensor (obstacles, corridor, green); `lengths`: laser_length per ray sensor; `order`: the
    keys of follower_sensors (a ray sensor listed before the tracker is scanned before it)."""
    z = np.load(GOLDEN + "/pool_B.npz")
    _, meta = load_episode("B_s1_chase")
    kw = dict(meta["kwargs"])
    src = {k: dict(v) for k, v in kw["follower_sensors"].items()}
    assert set(src) == {TRACKER, ALL, OBST} and (src[ALL]["lasers_count"], src[OBST]["lasers_count"]) == (12, 24)
    for k, (ro, rc, rg) in (reacts or {}).items():
        src[k].update(react_to_obstacles=ro, react_to_safe_corridor=rc, react_to_green_zone=rg)
    for k, length in (lengths or {}).items():
        src[k]["laser_length"] = length
    kw["follower_sensors"] = {k: src[k] for k in order}
    return config_for(dict(kwargs=kw, post=None), scen_route_len=int(z["route_len"].max()))


def _run(monkeypatch, cfg, pool, env_vars, twins, tag, seed=41, oracle_kw=None):
    """`cfg` under `env_vars` against the oracle and, bit for bit, against the same run under each dict of `twins`.  Returns per ray
    sensor (config order) the oracle's newest rows after every step: [STEPS, N, count]."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def make(vars_):
        for k, v in vars_.items():
            monkeypatch.setenv(k, v)
        e = _vec(N, cfg, pool)
        for k in vars_:
            monkeypatch.delenv(k)
        return e
    env = make(env_vars)
    others = [make(v) for v in twins]
    scen = pool_scenarios(pool)
    idx = (np.arange(N) * 3) % pool.n
    ora = OracleBatch(cfg, N, **(oracle_kw or {}))
    ora.reset(scen, idx)
    for e in [env] + others:
        e.reset(torch.from_numpy(idx.astype(np.int32)))
    _compare_with_oracle(env, ora, cfg, (tag, "reset"))
    for j, e in enumerate(others):
        _same(env, e, (tag, "reset", j))
    newest = [[] for _ in cfg.lasers]
    for t in range(STEPS):
        a = _actions(cfg, N, t, "mixed" if t % 2 else "random", seed=seed)
        act = torch.tensor(a, dtype=torch.float64, device="cuda:0")
        env.step(act)
        ora.step(a)
        _compare_with_oracle(env, ora, cfg, (tag, t))
        for j, e in enumerate(others):
            e.step(act)
            _same(env, e, (tag, t, j))
        for rows, l in zip(newest, cfg.lasers):
            at = l.out_offset + (l.history - 1) * l.width
            rows.append(ora.lasers[:, at:at + l.width].copy())
    for e in [env] + others:
        assert e.error_report() == (0, 0)
        e.close()
    return [np.stack(rows) for rows in newest]


@pytest.fixture(scope="module")
def pool_b():
    """The recorded pool of config B (scenarios do not depend on the sensors: one pool serves every variant of the config)."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    return ScenarioPool.from_npz(_b_config(), GOLDEN + "/pool_B.npz", "cuda:0")


def _hits(rows, length):
    return int((rows != np.float32(length)).sum())


def _between(rows, lo, hi):
    return int(((rows > np.float32(lo)) & (rows < np.float32(hi))).sum())


def _lengths(cfg):
    return [float(l.length) for l in cfg.lasers]


def test_config_B_mask_and_list_form(monkeypatch, pool_b):
    """Config B as shipped (mask form; corridor and caps culled at 102 px, rects at 152) against the cull off, and the list form
    (FTL_RAYS_ONE_PASS=0) with the same tables."""
    cfg = _b_config()
    rows = _run(monkeypatch, cfg, pool_b, {}, [CULL_OFF, {"FTL_RAYS_ONE_PASS": "0"}], "B")
    assert _lengths(cfg) == [100.0, 150.0]
    assert _hits(rows[0], 100) >= FLOOR and _hits(rows[1], 150) >= FLOOR


def test_roles_swapped(monkeypatch, pool_b):
    """The 100-px sensor reacts to obstacles only, the 150-px one to corridor and green only: rects are culled at 102 and the corridor at
    152 -- a reach table indexed the wrong way round loses the corridor readings beyond 102 px (observed on the CPU: 13,536 of them;
    readings other than the length: 4,820 and 235,169)."""
    cfg = _b_config(reacts={ALL: (True, False, False), OBST: (False, True, True)})
    rows = _run(monkeypatch, cfg, pool_b, {}, [CULL_OFF], "swapped")
    assert _lengths(cfg) == [100.0, 150.0]
    assert _between(rows[1], 102, 150) >= FLOOR
    assert _hits(rows[0], 100) >= FLOOR and _hits(rows[1], 150) >= FLOOR


def test_short_lasers(monkeypatch, pool_b):
    """Lengths 30 and 45: the reach boundary runs through the middle of the corridor and the rocks in every step (observed: 760 readings
    of the 45-px sensor beyond 32 px; hits: 12,227 and 881)."""
    cfg = _b_config(lengths={ALL: 30, OBST: 45})
    rows = _run(monkeypatch, cfg, pool_b, {}, [CULL_OFF], "short")
    assert _lengths(cfg) == [30.0, 45.0]
    assert _between(rows[1], 32, 45) >= FLOOR
    assert _hits(rows[0], 30) >= FLOOR and _hits(rows[1], 45) >= FLOOR


def test_a_class_nobody_sees(monkeypatch, pool_b):
    """Both sensors react to obstacles only: the corridor ring is not staged, no corridor segment and no cap is pushed (observed hits:
    4,820 and 21,974)."""
    cfg = _b_config(reacts={ALL: (True, False, False), OBST: (True, False, False)})
    rows = _run(monkeypatch, cfg, pool_b, {}, [CULL_OFF], "obstacles only")
    assert _hits(rows[0], 100) >= FLOOR and _hits(rows[1], 150) >= FLOOR


def test_per_pass_tables(monkeypatch, pool_b):
    """Sensor "all" / tracker / sensor "obstacles": two passes, the loop form.  Pass 0 stages the ring and culls the corridor at 102;
    pass 1 has no corridor class and culls rects at 152 (observed: 10,575 readings of the 150-px sensor between 102 and 150)."""
    cfg = _b_config(order=(ALL, TRACKER, OBST))
    assert [int(cfg.c.lasers[k].after_tracker) for k in range(cfg.c.n_lasers)] == [0, 1]
    rows = _run(monkeypatch, cfg, pool_b, {}, [CULL_OFF], "two passes")
    assert _lengths(cfg) == [100.0, 150.0]
    assert _between(rows[1], 102, 150) >= FLOOR
    assert _hits(rows[0], 100) >= FLOOR and _hits(rows[1], 150) >= FLOOR


def test_unstaged_corridor(monkeypatch):
    """Config E (CAPPED) with an 8-point LDS copy of the corridor: the span is not staged, phase 3 lists every segment of it and culls
    them where they are fetched; the caps are read from the ring in place and culled in phase 1 against the box of their class."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    _, meta = load_episode("E_s3_chase")
    cfg = config_for(meta, scen_route_len=256, rng_seed=9, env_id_base=7000)
    assert cfg.c.corr_cap > 128
    pool = ScenarioPool.generate(cfg, np.arange(128), "cuda:0")
    cap = {"FTL_DEBUG_CORR_LDS_CAP": "8"}
    rows = _run(monkeypatch, cfg, pool, cap, [dict(cap, **CULL_OFF)], "E unstaged", seed=33, oracle_kw=dict(env_id_base=7000))
    for r, l in zip(rows, cfg.lasers):
        assert _hits(r, l.length) >= 1, l.name
