"""GPU tests of the MLP policy population (include/ftl.h: ftl_mlp_act, ftl_rollout_mlp; ``mlp.MlpPolicy``, ``rollout_mlp``): the forward
kernel against the numpy twin (tests/mlp_numpy.py) bit for bit at every staging edge of the kernel, the three heads, the one-call
closed-loop rollout against the loop it replaces, populations against single nets, the parts of a pipelined batch, the two-stream handle
and ``evaluate``."""
import dataclasses

import numpy as np
import pytest
import torch

import mlp_numpy as M
from continiousenvironment_follower_leader_amd import abi
from golden_util import config_for, load_episode
from test_gpu_baseline import FIELDS, OUT, _fold

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUTP = OUT + ("policy_obs",)
TILE, KCH, EPW, NBLK = abi.FTL_MLP_ENV_TILE, abi.FTL_MLP_K_CHUNK, abi.FTL_MLP_ENVS_PER_WAVE, abi.FTL_MLP_NEURON_BLOCK
KLOW = abi.mlp_chunk_rows(abi.FTL_MLP_MAX_WIDTH)      # the chunk of a layer as wide as a layer gets
_POOLS = {}


def _cfg_pool(name, **over):
    """(cfg, pool of the usable scenarios among seeds 0..63) of a golden episode's config, with policy_obs sensors."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    key = (name, tuple(sorted(over.items())))
    if key not in _POOLS:
        _, meta = load_episode(name)
        cfg = config_for(meta, scen_route_len=256, **over)
        _POOLS[key] = (cfg, ScenarioPool.generate(cfg, np.arange(64), DEV))
    return _POOLS[key]


def _vec(name, n, cls=None, over=None, env_id_base=0, scen=None, **kw):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg, pool = _cfg_pool(name, **(over or {}))
    if env_id_base:
        cfg = dataclasses.replace(cfg, c=abi.Config.from_buffer_copy(cfg.c))
        cfg.c.env_id_base = env_id_base
    env = (cls or VecGame)(n, device=DEV, config=cfg, policy_obs=True, **kw)
    env.load_scenarios(pool)
    env.reset(scen)
    return env


def _policy(env, widths, n_sets=1, seed=0, scale=1.0, nasty=True):
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
    rng = np.random.default_rng(seed)
    p = M.nasty_params(rng, n_sets, widths, scale) if nasty else (rng.standard_normal((n_sets, M.param_count(widths))) * scale).astype(np.float32)
    return MlpPolicy(env, widths, params=torch.from_numpy(p).to(DEV), n_sets=n_sets), p


def _in_width(env):
    return int(env.policy_obs.shape[1] * env.policy_obs.shape[2])


def _check_act(env, widths, n_sets, seed):
    """Overwrite policy_obs with the nasty mix, act, and compare with the twin bit for bit."""
    pol, p = _policy(env, widths, n_sets, seed, scale=0.1)
    x = M.nasty_inputs(np.random.default_rng(1000 + seed), env.n, widths[0])
    env.policy_obs.copy_(torch.from_numpy(x).to(DEV).view_as(env.policy_obs))
    got = pol.act()
    assert got is pol.action
    lo, hi = M.bounds(env.cfg)
    want = M.population(p, widths, x, M.head_kind(env.cfg), lo, hi, env.n // n_sets)
    assert got.dtype == (torch.int32 if env.cfg.discrete_action_space else torch.float64) and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (widths, n_sets, int((got.cpu() != torch.from_numpy(want)).sum()))
    return got, want


# ---------------------------------------------------------------- 1. the act kernel equals the twin
def test_act_equals_the_twin():
    env = _vec("B_s1_chase", 69)
    assert _in_width(env) == 180
    a, want = _check_act(env, (180, 70, 33, 2), 3, 0)
    assert len(np.unique(want[:, 0])) > 8 and len(np.unique(want[:, 1])) > 8          # not a saturated head
    lo, hi = M.bounds(env.cfg)
    assert ((want > lo) & (want < hi)).any()
    _check_act(env, (180, 2), 3, 1)                                                    # L = 1: a linear policy
    _check_act(env, (180, 1, 256, 2), 3, 2)                                            # the narrowest and the widest layer
    _check_act(env, (180, 64, 65, 7, 2), 3, 3)                                         # four layers
    _check_act(env, (180, 33, 2), 69, 4)                                               # one env per set
    env.close()


@pytest.mark.parametrize("hidden", [(KCH - 1,), (KCH,), (KCH + 1,), (KLOW - 1, 256), (KLOW, 256), (KLOW + 1, 256), (2 * KCH + 3, 4 * KLOW + 2, 255),
                                    (2 * NBLK - 1,), (2 * NBLK,), (2 * NBLK + 1, 3), (6,)],
                         ids=lambda h: "-".join(map(str, h)))
def test_act_at_the_k_chunk_edges(hidden):
    """Hidden widths one below, at and one above the k-chunk of the layer that reads them: FTL_MLP_K_CHUNK rows for a narrow layer, the
    FTL_MLP_W_STAGE / 256 rows of the widest one (which is FTL_MLP_NEURON_BLOCK too: one block of neurons less, exact, one more); the
    input (180 = 64 + 64 + 52, or 3 * 56 + 12 before a 70-wide layer) always ends in a partial chunk; widths around two neuron blocks and
    widths that are no multiple of 4 (the k the matrix instruction leaves over)."""
    env = _vec("B_s1_chase", 37)
    _check_act(env, (180,) + hidden + (2,), 1, 10 + hidden[0])
    env.close()


@pytest.mark.parametrize("n, n_sets", [(TILE - 1, 1), (TILE, 1), (TILE + 1, 1), (2 * TILE - 2, 2), (2 * TILE, 2), (2 * TILE + 2, 2), (3 * TILE + 3, 1),
                                       (EPW - 1, 1), (EPW, 1), (EPW + 1, 1), (3, 3)])
def test_act_at_the_env_tile_edges(n, n_sets):
    """n and envs_per_set one below, at and one above FTL_MLP_ENV_TILE and FTL_MLP_ENVS_PER_WAVE; several tiles of one set."""
    env = _vec("B_s1_chase", n)
    _check_act(env, (180, 64, 64, 2), n_sets, 20 + n)
    env.close()


def test_act_on_a_wide_input():
    env = _vec("C_s1_chase", 35)
    assert _in_width(env) == 860
    _check_act(env, (860, 70, 33, 2), 5, 30)
    env.close()


@pytest.mark.parametrize("case, wrong", [(M.tie_case, M.fma_f64sum), (M.subnormal_case, M.fma_flush)], ids=["tie", "subnormal"])
def test_act_keeps_ties_and_subnormals(case, wrong):
    """Constructed rows (tests/mlp_numpy.py: tie_case, subnormal_case) whose ACTIONS change when a product is rounded twice at a tie, or
    when a float32 subnormal operand, running sum or result is flushed -- in the first layer at every lane position of the matrix
    instruction and across a k-chunk boundary, in a later layer through the matrix instruction and through the w_in % 4 rows.  The twin
    re-run with that wrong arithmetic must differ in every set, and the device must equal the exact twin."""
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
    env = _vec("B_s1_chase", 4 * M.ROWS)
    widths, p, x = case(180)
    lo, hi = M.bounds(env.cfg)
    exact = M.population(p, widths, x, M.BOX2, lo, hi, M.ROWS)
    bad = M.population(p, widths, x, M.BOX2, lo, hi, M.ROWS, fma=wrong)
    assert ((exact > lo) & (exact < hi)).all()                     # no clip hides the last bit
    differ = (exact != bad).any(1).reshape(4, M.ROWS).sum(1)
    assert (differ >= M.ROWS - 1).all(), differ                    # the rows really depend on the arithmetic under test, in every set
    pol = MlpPolicy(env, widths, params=torch.from_numpy(p).to(DEV), n_sets=4)
    env.policy_obs.copy_(torch.from_numpy(x).to(DEV).view_as(env.policy_obs))
    got = pol.act().cpu().numpy()
    print("device vs exact twin: %d of %d actions differ; vs the wrong arithmetic: %d" % ((got != exact).sum(), got.size, (got != bad).sum()))
    assert np.array_equal(got, exact), np.argwhere(got != exact)[:8]
    env.close()


# ---------------------------------------------------------------- 2. the heads
def _tie_columns(pol, p, set_, a, b, lift):
    """Make head outputs a and b of one set equal in every row, and the largest."""
    W, bias = pol.layer(len(pol.widths) - 2)
    W[set_, :, b] = W[set_, :, a]
    bias[set_, a] = bias[set_, b] = lift
    p[:] = pol.params.cpu().numpy()


def test_turn_head():
    env = _vec("Bcfs_s2_chase", 40)
    w0 = _in_width(env)
    assert env.cfg.constant_follower_speed and not env.cfg.discrete_action_space
    a, want = _check_act(env, (w0, 33, 1), 2, 40)
    assert tuple(a.shape) == (40,) and len(np.unique(want)) > 8
    before = env.state_field("env_int")[:, abi.EI_STEP_COUNT].clone()
    env.step(a)                                                                        # the result feeds step() unchanged
    assert bool(env.state_field("env_int")[:, abi.EI_STEP_COUNT].gt(before).all())
    env.close()


def test_discrete_head():
    env = _vec("B_s1_chase", 40, over=dict(discrete_action_space=True))
    a, want = _check_act(env, (180, 33, 5), 2, 41)
    assert len(np.unique(want)) >= 3
    # rows whose two largest outputs are equal: the first of them wins
    pol, p = _policy(env, (180, 33, 5), 2, 42, scale=0.1)
    _tie_columns(pol, p, 0, 1, 3, 1.0e6)
    _tie_columns(pol, p, 1, 2, 4, 1.0e6)
    x = env.policy_obs.cpu().numpy().reshape(40, 180)
    y = np.concatenate([M.raw_forward(p[s], pol.widths, x[20 * s:20 * s + 20]) for s in range(2)])
    assert np.array_equal(y[:20, 1], y[:20, 3]) and np.array_equal(y[20:, 2], y[20:, 4]) and (y.argmax(1) == np.repeat([1, 2], 20)).all()
    got = pol.act()
    assert got.cpu().tolist() == [1] * 20 + [2] * 20
    assert torch.equal(got.cpu(), torch.from_numpy(M.discrete_head(y)))
    before = env.state_field("env_int")[:, abi.EI_STEP_COUNT].clone()
    env.step(got)
    assert bool(env.state_field("env_int")[:, abi.EI_STEP_COUNT].gt(before).all())
    env.close()


# ---------------------------------------------------------------- 3. one call = the loop it replaces
def _capture(env, r):
    return dict(out={k: getattr(env, k).clone() for k in OUTP}, ro=[x.clone() for x in r[:3]], state={k: env.state_field(k).clone() for k in FIELDS},
                acts=r[3].clone() if len(r) > 3 else None)


def _same(env, ro, one, what, outputs=True):
    if outputs:
        for k in OUTP:
            assert torch.equal(getattr(env, k), one["out"][k]), (what, k)
    for x, y, k in zip(ro, one["ro"], ("ret", "steps", "status")):
        assert torch.equal(x, y), (what, k)
    for k in FIELDS:
        assert torch.equal(env.state_field(k), one["state"][k]), (what, k)


def test_rollout_is_the_loop():
    n, T, gamma = 69, 12, 0.97
    env = _vec("B_s1_chase", n)
    pol, _ = _policy(env, (180, 70, 33, 2), 3, 50, scale=0.1, nasty=False)
    for t in range(5):                                             # envs under way ...
        env.step(pol.act())
    env.reset(mask=(torch.arange(n) % 5 == 0).to(torch.uint8).to(DEV))      # ... and every fifth env freshly reset
    steps0 = env.state_field("env_int")[:, abi.EI_STEP_COUNT]
    assert 0 < int(steps0.eq(0).sum()) < n
    snap = env.snapshot()

    r = env.rollout_mlp(pol, T, gamma=gamma, record=True)
    assert len(r) == 4 and r[0] is env.rollout_ret and tuple(r[3].shape) == (T, n, 2) and r[3].dtype == torch.float64
    one = _capture(env, r)
    assert bool(one["ro"][1].eq(T).any()) and bool(one["ro"][0].ne(0).any())
    acts = one["acts"]
    assert bool((acts[1:] != acts[:-1]).any()) and bool((acts[:, 1:] != acts[:, :-1]).any())      # the loop really is closed
    assert int((acts[:, :, 1].std(0) > 0).sum()) > n // 2

    env.restore(snap, slot_stats=True)
    played = []

    def step(t):
        played.append(pol.act().clone())
        env.step(played[-1])
    ro = _fold(env, T, gamma, step)
    _same(env, ro, one, "loop")
    assert torch.equal(torch.stack(played), acts)

    env.restore(snap, slot_stats=True)                             # the open-loop rollout of what was recorded
    r2 = env.rollout(acts, gamma=gamma)
    _same(env, r2, one, "rollout", outputs=False)

    env.restore(snap, slot_stats=True)                             # without a record: the handle's scratch, the same result
    r3 = env.rollout_mlp(pol, T, gamma=gamma)
    assert len(r3) == 3
    _same(env, r3, one, "no record")
    fit = pol.fitness()
    assert tuple(fit.shape) == (3,) and torch.equal(fit, one["ro"][0].view(3, -1).mean(1))
    with pytest.raises(ValueError):
        env.rollout_mlp(pol, 0)
    with pytest.raises(ValueError):
        env.rollout_mlp(object(), 3)
    env.close()


# ---------------------------------------------------------------- 4. a population is its members
def test_population_equals_its_members():
    n, sets, T = 69, 3, 6
    per = n // sets
    widths = (180, 70, 33, 2)
    env = _vec("B_s1_chase", n)
    pol, p = _policy(env, widths, sets, 60, scale=0.1, nasty=False)
    a_all = pol.act().clone()
    r = env.rollout_mlp(pol, T, gamma=0.95, record=True)
    ret_all, acts_all = r[0].clone(), r[3].clone()
    assert len(set(ret_all.cpu().tolist())) > 1 and bool((acts_all[1:] != acts_all[:-1]).any())
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
    for s in range(sets):
        sub = _vec("B_s1_chase", per, env_id_base=per * s, scen=(torch.arange(per) + per * s) % env.pool.n)
        ps = MlpPolicy(sub, widths, params=torch.from_numpy(p[s:s + 1].copy()).to(DEV))
        assert torch.equal(ps.act(), a_all[per * s:per * (s + 1)]), s
        rs = sub.rollout_mlp(ps, T, gamma=0.95, record=True)
        assert torch.equal(rs[0], ret_all[per * s:per * (s + 1)]), s
        assert torch.equal(rs[3], acts_all[:, per * s:per * (s + 1)]), s
        sub.close()
    assert not torch.equal(a_all[:per], a_all[per:2 * per])
    # three identical sets are one set
    env.reset()
    same = MlpPolicy(env, widths, params=torch.from_numpy(np.repeat(p[1:2], sets, 0)).to(DEV), n_sets=sets)
    single = MlpPolicy(env, widths, params=torch.from_numpy(p[1:2].copy()).to(DEV))
    assert torch.equal(same.act(), single.act())
    env.close()


# ---------------------------------------------------------------- 5. pipelined: a set straddles the part boundary
def test_pipelined_matches_vec_game():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    n, sets = 1045, 5
    a, p = _vec("B_s1_chase", n), _vec("B_s1_chase", n, cls=PipelinedVecGame, parts=2)
    lo1 = p.shards[1].lo
    assert lo1 % (n // sets) != 0 and (lo1 - 1) // (n // sets) == lo1 // (n // sets)           # set 2 lies in both parts
    pa, params = _policy(a, (180, 70, 33, 2), sets, 70, scale=0.1, nasty=False)
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
    pp = MlpPolicy(p, (180, 70, 33, 2), params=torch.from_numpy(params).to(DEV), n_sets=sets)
    for env, pol in ((a, pa), (p, pp)):
        env.step(pol.act())                                        # the policy form on both, once
    p.join()
    assert torch.equal(pa.action, pp.action)
    for k in OUTP:
        assert torch.equal(getattr(a, k), getattr(p, k)), ("step", k)
    ra, rp = a.rollout_mlp(pa, 8, gamma=0.9, record=True), p.rollout_mlp(pp, 8, gamma=0.9, record=True)
    p.join()
    for x, y in zip(ra, rp):
        assert torch.equal(x, y)
    assert bool(ra[1].eq(8).any())
    for k in OUTP:
        assert torch.equal(getattr(a, k), getattr(p, k)), k
    for k in FIELDS:
        assert torch.equal(a.state_field(k), p.state_field(k)), k
    assert torch.equal(pa.fitness(), pp.fitness())
    a.close(), p.close()


# ---------------------------------------------------------------- 6. the handle's own two-stream mode
def test_rollout_on_a_two_stream_handle(monkeypatch):
    """Config F from 8,192 envs on steps on two streams: the act kernel of step t has to wait for the sensor kernels of both halves of
    step t - 1, and the halves of step t for it."""
    monkeypatch.setenv("FTL_SPLIT", "1")
    n, T, gamma = 8192 + 37, 4, 0.9
    env = _vec("F_s1_chase", n)
    assert _in_width(env) == 360
    pol, _ = _policy(env, (360, 32, 2), 1, 80, scale=0.1, nasty=False)
    env.step(pol.act())
    snap = env.snapshot()
    one = _capture(env, env.rollout_mlp(pol, T, gamma=gamma, record=True))
    env.restore(snap, slot_stats=True)
    played = []

    def step(t):
        played.append(pol.act().clone())
        env.step(played[-1])
    ro = _fold(env, T, gamma, step)
    _same(env, ro, one, "loop")
    assert torch.equal(torch.stack(played), one["acts"])
    assert bool(one["ro"][1].eq(T).any())
    env.close()


# ---------------------------------------------------------------- 7. the policy's score per scenario, whatever the batch size
def test_evaluate_is_independent_of_the_batch_size():
    recs = []
    for n in (32, 96):
        env = _vec("B_s1_chase", n)
        pol, _ = _policy(env, (180, 70, 33, 2), 1, 90, scale=0.1, nasty=False)
        scen = torch.arange(96) % env.pool.n
        recs.append(env.evaluate(pol, scen))
        env.close()
    r0, r1 = recs
    assert len(r0) == len(r1) == 96 and (r0["state"] == 2).all() and (r1["state"] == 2).all()
    for col in ("scenario", "frames", "calls", "status", "errors", "flags", "ret", "stream"):
        assert np.array_equal(r0[col], r1[col]), col
    assert len(set(r0["ret"].tolist())) > 1 and len(set(r0["frames"].tolist())) > 1, "every episode went the same way"
    assert (r0["errors"] == 0).all()
