"""GPU tests of the action search (include/ftl.h: ftl_search, ftl_search_begin / _sample / _select, ftl_unpack_envs_from;
``search.ActionSearch``): the three kernels against their numpy twin, the fan-out against the packed rows, the one call against the sequence
it replaces, and the properties the header states -- the real batch is only read, the clones are the envs' exact future, the candidates
follow an env's stream and not its slot.  Exact equality throughout.

Sizes: config B, 5 real envs stepped 50 times apart (one cloned from another, so its stream word is not 0; one at step count 0; one done), K = 1, 7,
64, 70 candidates (below, at and above one wavefront), T = 3 steps with hold = 2, two rounds."""
import ctypes as C

import numpy as np
import pytest
import torch

import search_numpy
from continiousenvironment_follower_leader_amd import _lib, abi
from golden_util import config_for, load_episode

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, T, HOLD, ITERS = 5, 3, 2, 2
KS = (1, 7, 64, 70)
FRESH, DONE, CLONE = 3, 4, 1       # the env at step count 0, the env that is done, the env that runs on env 0's stream
OUT = ("obs_num", "target", "reward", "done", "status", "lasers")

_POOL = []


def _cfg_pool():
    """(cfg, pool of seeds 0..63) of config B, as tests/test_gpu_baseline.py builds it."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    if not _POOL:
        _, meta = load_episode("B_s1_chase")
        cfg = config_for(meta, scen_route_len=256)
        _POOL.append((cfg, ScenarioPool.generate(cfg, np.arange(64), DEV)))
    return _POOL[0]


def _vec(n):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    cfg, pool = _cfg_pool()
    env = VecGame(n, device=DEV, config=cfg)
    env.load_scenarios(pool)
    env.reset()
    return env


PREP_STEPS = 50         # far enough for the slower followers to reach the edge of the leader's box: there the candidates' returns differ


def _prepared(n=N):
    """``n`` envs a few steps into different episodes: env CLONE a copy of env 0 (on env 0's stream) that then went its own way, env FRESH
    reset again (step count 0), env DONE with its done word set as a finished episode leaves it."""
    env = _vec(n)
    f = env.cfg.c.follower
    env.clone([0], [CLONE])
    e = torch.arange(n, dtype=torch.float64, device=DEV)
    for t in range(PREP_STEPS):
        a = torch.stack([f.max_speed * (1.0 - 0.15 * (e % 4)), f.max_rotation_speed * ((e + t) % 3 - 1.0)], 1).contiguous()
        env.step(a, sensors=False)
    env.reset(mask=(torch.arange(n) == FRESH).to(torch.uint8).to(DEV))
    ei = env.state_field("env_int")
    ei[DONE, abi.EI_DONE] = 1
    env.done[DONE] = 1
    env.scan()
    steps = ei[:, abi.EI_STEP_COUNT].tolist()
    assert steps[FRESH] == 0 and all(s > 0 for i, s in enumerate(steps) if i != FRESH)
    assert ei[:, abi.EI_DONE].tolist() == [1 if i == DONE else 0 for i in range(n)]
    return env


def _search(env, K, **kw):
    from continiousenvironment_follower_leader_amd.search import ActionSearch
    return ActionSearch(env, K, T, **dict(dict(hold=HOLD, iters=ITERS, gamma=0.97, seed=11), **kw))


def _streams(env):
    """The absolute stream id of every env: what a packed row carries at FTL_EI_STREAM."""
    w = env.state_field("env_int")[:, abi.EI_STREAM].cpu().numpy().astype(np.int64)
    return int(env.cfg.c.env_id_base) + np.arange(env.n) + w


def _plan(env, seed=0):
    """A float64 [T, n, 2] plan inside the Box, the same for the same seed."""
    lo, hi = search_numpy.box(env.cfg)
    return torch.from_numpy(lo + np.random.default_rng(seed).random((T, env.n, 2)) * (hi - lo)).to(DEV)


def _pack(s):
    _lib.check(s.lib.ftl_pack_envs(s.batch.h, s.env_ids.data_ptr(), s.n, s.rows.data_ptr(), s.batch._stream()), s.lib)


def _row_word(env, which):
    off, per, dt, st = C.c_size_t(), C.c_size_t(), C.c_int32(), C.c_size_t()
    _lib.check(env.lib.ftl_state_field(env.h, b"env_int", C.byref(off), C.byref(per), C.byref(dt), C.byref(st)), env.lib)
    return off.value // 4 + which


# ---------------------------------------------------------------- 1. the sample kernel
@pytest.mark.parametrize("K", KS)
def test_sample_equals_the_twin(K):
    env = _prepared()
    s = _search(env, K)
    lo, hi = search_numpy.box(env.cfg)
    streams = _streams(env)
    assert streams[CLONE] == streams[0] and len(set(streams.tolist())) == N - 1
    _pack(s)
    call, it, rad = 3, 1, s.radius(1)
    assert rad == 0.5
    flat = _plan(env)[:1].expand(T, N, 2).clone()            # one action at every step, and env CLONE plans what env 0 plans
    flat[:, CLONE] = flat[:, 0]
    for plan in (_plan(env), flat):
        s.nominal.copy_(plan)
        s.cand.fill_(float("nan"))
        _lib.check(s.lib.ftl_search_sample(env.h, s.rows.data_ptr(), N, C.byref(s.params), call, it, rad, s.nominal.data_ptr(), s.cand.data_ptr(),
                                           env._stream()), s.lib)
        cand = s.cand.cpu().numpy()
        want = search_numpy.sample(plan.cpu().numpy(), streams, 11, call, it, K, HOLD, rad, lo, hi)
        assert np.array_equal(cand, want)
        assert np.array_equal(cand[:, ::K], plan.cpu().numpy())                 # k = 0 is the nominal, exactly
        assert (cand >= lo).all() and (cand <= hi).all()
        assert torch.equal(s.nominal, plan)
        if K > 1:
            clipped = (cand == lo) | (cand == hi)
            assert clipped.any() and not clipped.all()                          # the Box cuts some candidates, not all
    # (the flat plan) steps 0 and 1 share a hold block and so their draws, step 2 starts the next block; the two envs on one stream
    # draw the same candidates
    c = cand.reshape(T, N, K, 2)
    assert np.array_equal(c[0], c[1]) and np.array_equal(c[:, CLONE], c[:, 0])
    if K > 1:
        assert not np.array_equal(c[0], c[2]) and not np.array_equal(c[:, 2] - c[:, 2, :1], c[:, 0] - c[:, 0, :1])
    env.close(), s.close()


# ---------------------------------------------------------------- 2. the select kernel
def _ret_cases(K, rng):
    last = K - 1
    rows = []
    r = np.zeros(K); r[[K // 3, K // 2, last]] = 1.0; rows.append(r)                       # ties at several k
    r = np.full(K, -3.0); r[[0, last]] = 2.5; rows.append(r)                               # the maximum at k = 0 (and again at the end)
    r = np.full(K, -3.0); r[last] = -1.0; rows.append(r)                                   # at K - 1
    r = rng.random(K); r[min(63, last)] = 7.0; rows.append(r)                              # at lane 63
    r = rng.random(K); r[min(64, last)] = 7.0; rows.append(r)                              # at lane 0 of the second pass
    r = rng.random(K); r[[min(63, last), min(64, last)]] = 7.0; rows.append(r)             # both: the lower one
    rows.append(np.full(K, -2.0))                                                          # all equal
    r = np.zeros(K); r[0::2] = -0.0; rows.append(r)                                        # -0.0 first, then 0.0: k = 0
    r = np.zeros(K); r[1::2] = -0.0; r[last] = -4.0 if K > 2 else r[last]; rows.append(r)  # 0.0 first
    rows.append(rng.integers(0, 4, K).astype(np.float64))                                  # many duplicates
    rows.append(-rng.random(K) * 1e300)
    return np.concatenate(rows)


@pytest.mark.parametrize("K,Ts", [(1, 3), (7, 3), (64, 3), (70, 3), (70, 67), (200, 2)])
def test_select_equals_the_twin(K, Ts):
    env = _vec(1)
    rng = np.random.default_rng(K)
    ret = _ret_cases(K, rng)
    n = len(ret) // K
    assert n == 11                                                                         # three workgroups of four wavefronts, the last one partial
    cand = rng.random((Ts, n * K, 2))
    d = lambda a: torch.from_numpy(a).to(DEV)
    ret_d, cand_d, nominal = d(ret), d(cand), torch.full((Ts, n, 2), -1.0, dtype=torch.float64, device=DEV)
    best_k, best_ret = torch.full((n,), -7, dtype=torch.int32, device=DEV), torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    _lib.check(env.lib.ftl_search_select(env.h, ret_d.data_ptr(), n, K, Ts, cand_d.data_ptr(), nominal.data_ptr(), best_k.data_ptr(),
                                         best_ret.data_ptr(), env._stream()), env.lib)
    wk, wr, wn = search_numpy.select(ret, K, cand, np.full((Ts, n, 2), -1.0))
    assert np.array_equal(best_k.cpu().numpy(), wk)
    assert np.array_equal(best_ret.cpu().numpy().view(np.int64), wr.view(np.int64))        # bit for bit: the sign of a zero too
    assert np.array_equal(nominal.cpu().numpy(), wn)
    assert wk[6] == 0 and wk[7] == 0 and wk[8] == 0 and wk[1] == 0 and wk[2] == K - 1 and wk[5] == min(63, K - 1)
    assert torch.equal(ret_d, d(ret)) and torch.equal(cand_d, d(cand))
    env.close()


# ---------------------------------------------------------------- 3. the fan-out
@pytest.mark.parametrize("K", KS)
def test_fan_out(K):
    env = _prepared()
    s = _search(env, K)
    s._follow_pool()
    cl, nk = s.clones, N * K
    _pack(s)
    rows, blob = s.rows.clone(), cl.state.clone()
    back = torch.empty(nk, env.env_bytes, dtype=torch.uint8, device=DEV)
    w_stream = _row_word(env, abi.EI_STREAM)
    for flags in (0, abi.FTL_ENV_OWN_STREAM):
        cl.state.copy_(blob)                                                               # fresh slots: stream word 0
        _lib.check(s.lib.ftl_unpack_envs_from(cl.h, s.rows.data_ptr(), s.row_ids.data_ptr(), s.env_ids.data_ptr(), nk, flags, env._stream()), s.lib)
        _lib.check(s.lib.ftl_pack_envs(cl.h, s.env_ids.data_ptr(), nk, back.data_ptr(), env._stream()), s.lib)
        assert torch.equal(s.rows, rows)
        src = rows[s.row_ids.long()]
        if not flags:
            assert torch.equal(back, src)                                                  # every clone packs to its source's row
            continue
        a, b = back.view(torch.int32), src.view(torch.int32)
        diff = (a != b).nonzero()
        assert set(diff[:, 1].tolist()) <= {w_stream}                                      # only the stream word differs ...
        own = int(cl.cfg.c.env_id_base) + torch.arange(nk, device=DEV, dtype=torch.int32)
        assert torch.equal(a[:, w_stream], own)                                            # ... and it is the slot's own stream
        assert K == 1 or len(diff) > 0
    env.close(), s.close()


# ---------------------------------------------------------------- 4. one call = the sequence it replaces
@pytest.mark.parametrize("K,own", [(1, False), (7, False), (64, False), (70, False), (7, True)])
def test_search_is_the_sequence(K, own):
    env = _prepared()
    s = _search(env, K, own_stream=own)
    s._follow_pool()
    cl, nk, lib, st = s.clones, N * K, s.lib, env._stream()
    blob, plan = cl.state.clone(), _plan(env, 1)
    for call, warm in ((0, True), (4, True), (4, False)):
        s.warm = warm
        cl.state.copy_(blob)
        s.nominal.copy_(plan)
        s.act(call=call)
        names = ("rows", "nominal", "cand", "action", "best_k", "best_ret", "ret")
        one = {k: getattr(s, k).clone() for k in names}
        one.update(state=cl.state.clone(), steps=cl.rollout_steps.clone(), status=cl.rollout_status.clone(), **{"o_" + k: getattr(cl, k).clone() for k in OUT})
        assert one["ret"].ne(0).any() and one["steps"].eq(T).any()

        cl.state.copy_(blob)
        s.nominal.copy_(plan)
        for k in names[2:]:
            getattr(s, k).fill_(-5)
        s.rows.fill_(0)
        _pack(s)
        _lib.check(lib.ftl_search_begin(env.h, s.rows.data_ptr(), N, T, call, int(warm), s.nominal.data_ptr(), st), lib)
        for it in range(ITERS):
            _lib.check(lib.ftl_search_sample(env.h, s.rows.data_ptr(), N, C.byref(s.params), call, it, s.radius(it), s.nominal.data_ptr(),
                                             s.cand.data_ptr(), st), lib)
            _lib.check(lib.ftl_unpack_envs_from(cl.h, s.rows.data_ptr(), s.row_ids.data_ptr(), s.env_ids.data_ptr(), nk,
                                                abi.FTL_ENV_OWN_STREAM if own else 0, st), lib)
            cl.rollout(s.cand, gamma=0.97, sensors=False)
            _lib.check(lib.ftl_search_select(cl.h, s.ret.data_ptr(), N, K, T, s.cand.data_ptr(), s.nominal.data_ptr(), s.best_k.data_ptr(),
                                             s.best_ret.data_ptr(), st), lib)
        s.action.copy_(s.nominal[0])
        for k in names:
            assert torch.equal(getattr(s, k), one[k]), (call, warm, k)
        assert torch.equal(cl.state, one["state"]), (call, warm, "state")
        assert torch.equal(cl.rollout_steps, one["steps"]) and torch.equal(cl.rollout_status, one["status"])
        for k in OUT:
            assert torch.equal(getattr(cl, k), one["o_" + k]), (call, warm, k)
    env.close(), s.close()


# ---------------------------------------------------------------- 5, 6, 10. the real batch is only read; the clones are its exact future
@pytest.mark.parametrize("gamma", [1.0, 0.97])
@pytest.mark.parametrize("K", KS)
def test_best_ret_is_the_real_return(K, gamma):
    env = _prepared()
    s1, s2 = _search(env, K, iters=1, gamma=gamma), _search(env, K, iters=2, gamma=gamma)
    snap = env.snapshot()
    blob, outs = env.state.clone(), {k: getattr(env, k).clone() for k in OUT}
    plan = _plan(env, 3)
    for s in (s1, s2):
        s.nominal.copy_(plan)
        a = s.act(call=6)
        assert a is s.action and a.dtype == torch.float64 and tuple(a.shape) == (N, 2)
        assert torch.equal(a, s.nominal[0])
    assert torch.equal(env.state, blob)                                                    # 5. state and outputs byte for byte
    for k in OUT:
        assert torch.equal(getattr(env, k), outs[k]), k
    steps = env.state_field("env_int")[:, abi.EI_STEP_COUNT].cpu().numpy()
    start = torch.from_numpy(search_numpy.begin(steps, plan.cpu().numpy(), 6, True, env.cfg.c.follower.max_speed)).to(DEV)
    assert torch.equal(start[:, FRESH, 0], torch.full((T,), env.cfg.c.follower.max_speed, dtype=torch.float64, device=DEV))

    rets = []
    for actions in (start, s1.nominal, s2.nominal):                                        # 6. played on the real batch
        rets.append(env.rollout(actions.clone(), gamma=gamma, sensors=False)[0].clone())
        assert env.rollout_steps.tolist() == [0 if i == DONE else T for i in range(N)]
        env.restore(snap, slot_stats=True)
    alone, r1, r2 = rets
    assert torch.equal(r1, s1.best_ret) and torch.equal(r2, s2.best_ret)
    assert bool((s1.best_ret >= alone).all()) and bool((s2.best_ret >= s1.best_ret).all())
    print("K = %d gamma = %g: nominal %s, round 1 %s, round 2 %s" % (K, gamma, alone.tolist(), r1.tolist(), r2.tolist()))
    if K == 1:
        assert torch.equal(s2.nominal, start) and torch.equal(r2, alone)
    else:                                                                                  # (the test has teeth: a candidate beat the plan)
        assert bool((s1.best_ret > alone).any()) and bool(s1.best_k.ne(0).any())
    for s in (s1, s2):                                                                     # 10. the done env
        assert int(s.best_k[DONE]) == 0 and float(s.best_ret[DONE]) == 0.0
        assert torch.equal(s.action[DONE], start[0, DONE])
        assert bool(s.ret[DONE * K:(DONE + 1) * K].eq(0).all())
        assert bool((s.best_k >= 0).all()) and bool((s.best_k < K).all())
        s.close()
    env.close()


# ---------------------------------------------------------------- 7. the candidates follow the env, not its slot
@pytest.mark.parametrize("K", [7, 70])
def test_slot_independence(K):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    a = _prepared()
    cfg, pool = _cfg_pool()
    b = VecGame(9, device=DEV, config=cfg)
    b.load_scenarios(pool)
    b.reset()
    src, dst = 2, 6
    b.restore(a.snapshot([src]), env_ids=[dst])
    assert _streams(b)[dst] == _streams(a)[src] != int(cfg.c.env_id_base) + dst
    sa, sb = _search(a, K), _search(b, K)
    sa.act(call=0), sb.act(call=0)
    assert torch.equal(sa.cand[:, src * K:(src + 1) * K], sb.cand[:, dst * K:(dst + 1) * K])
    assert not torch.equal(sa.cand[:, src * K:(src + 1) * K], sb.cand[:, (dst - 1) * K:dst * K])       # (env dst - 1 runs on its own stream)
    for k in ("best_k", "best_ret", "action"):
        assert torch.equal(getattr(sa, k)[src], getattr(sb, k)[dst]), k
    assert torch.equal(sa.nominal[:, src], sb.nominal[:, dst])
    a.close(), b.close(), sa.close(), sb.close()


# ---------------------------------------------------------------- 8. where a call starts from
def test_begin_rule():
    env = _prepared()
    s = _search(env, 7)
    speed = env.cfg.c.follower.max_speed
    steps = env.state_field("env_int")[:, abi.EI_STEP_COUNT].cpu().numpy()
    plan = _plan(env, 3)
    _pack(s)
    for call, warm in ((0, 1), (0, 0), (1, 1), (1, 0), (2 ** 40, 1)):
        s.nominal.copy_(plan)
        _lib.check(s.lib.ftl_search_begin(env.h, s.rows.data_ptr(), N, T, call, warm, s.nominal.data_ptr(), env._stream()), s.lib)
        got = s.nominal.cpu().numpy()
        assert np.array_equal(got, search_numpy.begin(steps, plan.cpu().numpy(), call, bool(warm), speed)), (call, warm)
        default = np.broadcast_to([speed, 0.0], (T, 2))
        assert np.array_equal(got[:, FRESH], default)
        for e in range(N):
            if e == FRESH:
                continue
            if call == 0 or not warm:
                assert np.array_equal(got[:, e], default)
            else:                                                                          # shifted by one step, the last step kept
                assert np.array_equal(got[:-1, e], plan[1:, e].cpu().numpy()) and np.array_equal(got[-1, e], plan[-1, e].cpu().numpy())
    # the same call from the same plan gives the same result; another call counter draws other candidates
    res = []
    for call in (5, 5, 6):
        s.nominal.copy_(plan)
        s.act(call=call)
        res.append({k: getattr(s, k).clone() for k in ("cand", "nominal", "action", "best_k", "best_ret")})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    assert not torch.equal(res[0]["cand"], res[2]["cand"])
    # the counter of act() itself: 0, 1, 2, ...; a call without warm starts from the default whatever the plan holds
    assert s.calls == 0
    s.act(), s.act()
    assert s.calls == 2
    cold = _search(env, 7, iters=1, warm=False)
    cold.nominal.copy_(plan)
    cold.act(call=9)
    assert torch.equal(cold.cand[:, ::7], torch.tensor([speed, 0.0], dtype=torch.float64, device=DEV).expand(T, N, 2))
    env.close(), s.close(), cold.close()


# ---------------------------------------------------------------- 9. the search as the policy of evaluate()
def test_evaluate_equals_the_hand_written_loop():
    scen = torch.tensor([3, 9, 17, 20, 33, 41])
    env = _vec(4)
    s = _search(env, 7)
    recs = env.evaluate(s, scen, sensors=False)
    assert env.queue is None and len(recs) == 6 and (recs["state"] == 2).all()
    env.close(), s.close()

    env = _vec(4)
    s = _search(env, 7)
    q = env.set_episode_queue(scen)
    env.reset_from_queue()
    calls = 0
    while True:
        env.step(s.act(), auto_reset="queue", sensors=False)
        calls += 1
        if calls % 16 == 0 and int(q.finished()) == q.n:
            break
        assert calls < 2 * (env.cfg.c.max_steps // env.cfg.c.frames_per_step + 2) + 16
    mine = q.records()
    env.set_episode_queue(None)
    for col in ("state", "scenario", "env", "frames", "calls", "status", "errors", "flags", "ret", "stream"):
        assert np.array_equal(recs[col], mine[col]), col
    assert len(set(recs["ret"].tolist())) > 1
    env.close(), s.close()


# ---------------------------------------------------------------- the wrapper's refusals that need a device
def test_pool_rules():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    env = _prepared()
    s = _search(env, 7)
    s.act()
    env.pool.version += 1                                                                  # what ScenarioPool.write / a moving ring does
    try:
        with pytest.raises(ValueError, match="written since"):
            s.act()
    finally:
        env.pool.version -= 1
    s.act()
    cfg, pool = _cfg_pool()
    p = PipelinedVecGame(8, parts=2, device=DEV, config=cfg)
    with pytest.raises(ValueError, match="pipelined"):
        _search(p, 7)
    p.close(), env.close(), s.close()
