"""GPU tests of the episode queue (include/ftl.h: ftl_set_episode_queue, ftl_queue_start, FTL_STEP_QUEUE_RESET; ``VecGame.set_episode_queue``,
``reset_from_queue``, ``step(a, auto_reset="queue")``, ``evaluate``).

The oracle is the behaviour the library had before the queue: a FRESH ``VecGame(Q, env_id_base=S0)`` reset with ``scen_idx = queue`` and
stepped WITHOUT auto-reset until every env is done; for each env the state's reward sum (overall_reward), step_count, the status row and
the error word are read at the call that raised its done, together with the observation rows that call returned.  A world that is done at
reset (an empty route: the only world ``reset`` leaves done) has frames 0, calls 0, return 0, status 0/0/0 and the DONE_AT_RESET flag; its
error word and terminal rows are those of its first call.  Policies are pure functions of an env's own observation row, so the same episode
gets the same actions in whichever slot of whichever batch it runs.  Every comparison is exact equality."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from continiousenvironment_follower_leader_amd import _lib, abi
from golden_util import GOLDEN, config_for, load_episode

pytestmark = pytest.mark.gpu

Q = 600
S0 = 1000                    # stream id of entry 0
COLS = ("scenario", "frames", "calls", "status", "errors", "flags", "ret", "stream")
OBS = ("obs_num", "lasers", "target")


@pytest.fixture(autouse=True, params=["4 lanes per env", "8 lanes per env"])
def lanes_per_env(request, monkeypatch):
    """Both forms of the frame kernel (FTL_DEBUG_G8 at ftl_create, as tests/test_gpu_parity.py)."""
    monkeypatch.setenv("FTL_DEBUG_G8", "0" if request.param.startswith("4") else "1")
    return request.param


_POOLS, _ORACLES = {}, {}


def _cfg_pool(name):
    """(cfg, pool) with episodes of a few calls: B the headline world (B400: with 40 calls to the time limit), E random speed / acceleration regimes, F random frames per step
    (and the regimes), T the v1 tracker kernel."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    if name not in _POOLS:
        if name in ("B", "B400"):
            z = np.load(GOLDEN + "/pool_B.npz")
            meta = json.loads(str(z["meta"]))
            cfg = config_for(dict(kwargs=meta["kwargs"], post=None), scen_route_len=int(z["route_len"].max()),
                             max_steps=400 if name == "B400" else 60, warm_start=10)
            pool = ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0", limit=128)
        else:
            ep = {"E": "E_s3_chase", "F": "F_s7_chase", "T": "T_s3_chase"}[name]
            _, meta = load_episode(ep)
            over = {"E": dict(max_steps=80, warm_start=10, rng_seed=7), "F": dict(max_steps=150, warm_start=10, rng_seed=4),
                    "T": dict(max_steps=60, warm_start=10)}[name]
            cfg = config_for(meta, scen_route_len=256, **over)
            pool = ScenarioPool.generate(cfg, np.arange(131), "cuda:0")
        _POOLS[name] = (cfg, pool)
    return _POOLS[name]


def _with_base(cfg, base):
    ck = dataclasses.replace(cfg, c=abi.Config.from_buffer_copy(cfg.c))
    ck.c.env_id_base = base
    return ck


def _vec(cfg, pool, n, base=0, **kw):
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    env = VecGame(n, device="cuda:0", config=_with_base(cfg, base), **kw)
    env.load_scenarios(pool)
    return env


def _queue_scen(pool, q=Q):
    """Q entries that walk a part of the pool several times: the same scenario comes back under different stream ids."""
    return ((torch.arange(q) * 7 + 3) % min(pool.n, 97)).to(torch.int32)


# ---------------------------------------------------------------- policies: action = f(the env's own observation row)
def _policy(kind, cfg):
    ms, mr, md = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed, cfg.c.min_distance
    dev = torch.device("cuda:0")
    if kind == "chase":
        def chase(obs):
            x = obs[0].double()
            dx, dy = x[:, 0] - x[:, 5], x[:, 1] - x[:, 6]
            want = torch.remainder(torch.rad2deg(torch.atan2(dy, dx)), 360.0)
            err = torch.remainder(want - x[:, 8] + 540.0, 360.0) - 180.0
            w = torch.clamp(err * 0.3, -mr, mr)
            dist = torch.sqrt(dx * dx + dy * dy)
            v = torch.where(dist > md * 2.4, torch.full_like(dist, ms), torch.where(dist < md * 1.5, torch.zeros_like(dist), torch.full_like(dist, 0.9 * ms)))
            return torch.stack([v, w], 1).contiguous()
        return chase
    if kind == "constant":
        return lambda obs: torch.tensor([0.7 * ms, 0.15 * mr], dtype=torch.float64, device=dev).repeat(obs[0].shape[0], 1).contiguous()
    g = torch.Generator(device="cpu").manual_seed(3)
    v = (0.4 + 0.6 * torch.rand(4093, generator=g, dtype=torch.float64)) * ms
    w = torch.clamp(torch.randn(4093, generator=g, dtype=torch.float64) * 0.4 * mr, -mr, mr)
    table = torch.stack([v, w], 1).to(dev)
    k1 = (torch.arange(abi.FTL_OBS_NUM, device=dev) * 2 + 1) * 2654435761
    k2 = (torch.arange(max(cfg.lasers_len, 1), device=dev) * 2 + 1) * 40503

    def hashed(obs):                                   # exact integer arithmetic over the bytes of the row
        h = (obs[0].view(torch.int32).long() * k1).sum(1) + (obs[1].view(torch.int32).long() * k2).sum(1)
        return table[torch.remainder(h, 4093)].contiguous()
    return hashed


# ---------------------------------------------------------------- the oracle
def _oracle(name, kind, lanes, pool_key=None, cfg_pool=None, scen=None):
    key = (name, kind, lanes, pool_key)
    if key in _ORACLES:
        return _ORACLES[key]
    cfg, pool = cfg_pool or _cfg_pool(name)
    scen = _queue_scen(pool) if scen is None else scen
    n = int(scen.numel())
    env = _vec(cfg, pool, n, base=S0)
    pol = _policy(kind, cfg)
    env.reset(scen)
    dev = env.device
    at_reset = env.done.bool().clone()
    seen = torch.zeros(n, dtype=torch.bool, device=dev)
    o = dict(frames=torch.zeros(n, dtype=torch.int32, device=dev), calls=torch.zeros(n, dtype=torch.int32, device=dev),
             status=torch.zeros(n, 3, dtype=torch.int32, device=dev), errors=torch.zeros(n, dtype=torch.int32, device=dev),
             ret=torch.zeros(n, dtype=torch.float64, device=dev))
    term = {k: torch.zeros_like(getattr(env, k)) for k in OBS}
    limit = cfg.c.max_steps // (cfg.c.rand_fps_lo if cfg.c.rand_fps_hi > 0 else cfg.c.frames_per_step) + 3
    for t in range(limit):
        env.step(pol((env.obs_num, env.lasers)))
        new = env.done.bool() & ~seen
        ei, ed = env.state_field("env_int"), env.state_field("env_dbl")
        live = new & ~at_reset
        o["frames"] = torch.where(live, ei[:, abi.EI_STEP_COUNT], o["frames"])
        o["calls"] = torch.where(live, torch.full_like(o["calls"], t + 1), o["calls"])
        o["status"] = torch.where(live[:, None], env.status.int(), o["status"])
        o["ret"] = torch.where(live, ed[:, abi.ED_OVERALL_REWARD], o["ret"])
        o["errors"] = torch.where(new, ei[:, abi.EI_ERROR], o["errors"])
        for k in OBS:
            term[k] = torch.where(new.reshape(-1, *[1] * (term[k].dim() - 1)), getattr(env, k), term[k])
        seen |= new
        if bool(seen.all()):
            break
    assert bool(seen.all()), "the oracle batch did not finish"
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["errors"] = out["errors"].astype(np.uint32)
    out["scenario"] = scen.numpy().astype(np.int32)
    out["flags"] = at_reset.cpu().numpy().astype(np.uint32) * abi.FTL_EPISODE_DONE_AT_RESET
    out["stream"] = S0 + np.arange(n, dtype=np.int64)
    out["term"] = {k: v.cpu() for k, v in term.items()}
    env.close()
    _ORACLES[key] = out
    return out


def _same_table(rec, ora, what):
    assert (rec["state"] == 2).all(), what
    for c in COLS:
        bad = np.nonzero((rec[c] != ora[c]).reshape(len(rec), -1).any(1))[0]
        assert bad.size == 0, (what, c, bad[:8], rec[c][bad[:4]], ora[c][bad[:4]])


def _drain(env, q, pol, per_call=None):
    """Step a started queue until it is drained; per_call(t) runs after every call.  No hand-out order needs more calls than ``evaluate``'s
    default ``max_calls``: ceil(Q / n) rounds of the longest episode."""
    c = env.cfg.c
    cap = -(-q.n // env.n) * (c.max_steps // (c.rand_fps_lo if c.rand_fps_hi > 0 else c.frames_per_step) + 2) + 8
    t = 0
    while True:
        env.step(pol((env.obs_num, env.lasers)), auto_reset="queue")
        if per_call:
            per_call(t)
        t += 1
        if t % 8 == 0 and int(q.finished()) == q.n:
            return t
        assert t < cap, "the queue did not drain"


# ---------------------------------------------------------------- 1. exactly once, slot-independent
@pytest.mark.parametrize("name, kind", [("B", "chase"), ("B", "hashed"), ("B", "constant"), ("E", "chase"), ("E", "hashed"), ("F", "chase"),
                                        ("F", "hashed"), ("T", "chase"), ("T", "constant")])
def test_every_entry_once_and_slot_independent(name, kind, lanes_per_env):
    cfg, pool = _cfg_pool(name)
    ora = _oracle(name, kind, lanes_per_env)
    scen = _queue_scen(pool)
    assert len(set(scen.tolist())) < Q            # repeats of a scenario under different stream ids
    for n in (1, 7, 64, 256):
        final = n in (7, 256)                     # with and without the final buffers; with them the terminal rows are compared too
        env = _vec(cfg, pool, n, base=3, final_obs=final)      # (a base of its own: the stream word holds a non-trivial offset)
        q = env.set_episode_queue(scen, stream_base=S0)
        env.reset_from_queue()
        term = {k: torch.zeros_like(ora["term"][k], device="cuda:0") for k in OBS}
        before = [env.ticket.clone()]

        def keep_terminal_rows(t):                # (device work only: row `ticket` of the table <- the final row of its slot)
            ended = env.ended.bool()
            tk = before[0][ended].long()
            for k in OBS:
                term[k][tk] = getattr(env, "final_" + k)[ended]
            before[0] = env.ticket.clone()
        _drain(env, q, _policy(kind, cfg), keep_terminal_rows if final else None)
        rec = q.records()
        _same_table(rec, ora, (name, kind, n))
        if final:
            for k in OBS:
                assert torch.equal(term[k].cpu(), ora["term"][k]), (name, kind, n, k)
        assert ((rec["env"] >= 0) & (rec["env"] < n)).all()
        assert int(q.remaining()) == 0 and int(q.head) >= Q
        env.close()
    if name in ("E", "F"):                        # the case is worth something: episodes of one scenario differ between streams
        by, by_obs = {}, {}
        for i, (s, f, r) in enumerate(zip(ora["scenario"], ora["frames"], ora["ret"])):
            by.setdefault(int(s), set()).add((int(f), float(r)))
            by_obs.setdefault(int(s), set()).add(ora["term"]["obs_num"][i].numpy().tobytes())
        differ, differ_obs = sum(len(v) > 1 for v in by.values()), sum(len(v) > 1 for v in by_obs.values())
        print("%s / %s: of %d scenarios, %d gave different (frames, return) and %d different terminal rows on different streams"
              % (name, kind, len(by), differ, differ_obs))
        assert differ_obs > len(by) // 2 and (name == "E" or differ > 0)


# ---------------------------------------------------------------- 2. deterministic hand-out
def test_hand_out_is_deterministic_and_in_slot_order():
    cfg, pool = _cfg_pool("B")
    scen, pol = _queue_scen(pool), _policy("hashed", cfg)
    runs = []
    for _ in range(2):
        env = _vec(cfg, pool, 64, final_obs=True)
        q = env.set_episode_queue(scen, stream_base=S0)
        env.reset_from_queue()
        assert torch.equal(env.ticket.cpu(), torch.arange(64, dtype=torch.int32))
        masks, head = [], [64]

        def check(t):
            masks.append((env.ended.cpu().clone(), env.restarted.cpu().clone()))
            if t < 50:                            # the entries taken in this call: consecutive from the old head, ascending in slot order
                took = env.ticket.cpu()[env.restarted.cpu().bool()]
                assert torch.equal(took, torch.arange(head[0], head[0] + took.numel(), dtype=torch.int32)), t
                assert not bool((env.restarted.cpu().bool() & ~env.ended.cpu().bool()).any())
                head[0] = min(head[0] + int(env.ended.sum()), 10 ** 9)
                assert int(q.head) == head[0]
        _drain(env, q, pol, check)
        runs.append((q.records(), masks))
        env.close()
    (r0, m0), (r1, m1) = runs
    assert np.array_equal(r0["env"], r1["env"]) and r0.tobytes() == r1.tobytes()
    assert len(m0) == len(m1)
    for (e0, s0), (e1, s1) in zip(m0, m1):
        assert torch.equal(e0, e1) and torch.equal(s0, s1)


# ---------------------------------------------------------------- 3. drain and park
@pytest.mark.parametrize("q_len, n", [(40, 64), (100, 64)])
def test_drain_and_park(q_len, n, lanes_per_env):
    from continiousenvironment_follower_leader_amd.vec_game import EpisodeQueue
    cfg, pool = _cfg_pool("B")
    scen = _queue_scen(pool, q_len + 8)
    ora = _oracle("B", "chase", lanes_per_env, pool_key=("park", q_len), scen=scen[:q_len])
    q = EpisodeQueue(scen, None, S0, "cuda:0", pool.n)
    sentinel = -0x0102030405060708
    q._rec[q_len:] = sentinel                     # a second table right behind the first: nothing may be written past entry Q - 1
    q.n = q_len
    env = _vec(cfg, pool, n)
    assert env.set_episode_queue(q) is q
    env.reset_from_queue()
    tk = env.ticket.cpu()
    assert torch.equal(tk[:min(q_len, n)], torch.arange(min(q_len, n), dtype=torch.int32)) and bool((tk[q_len:] == -1).all())
    assert bool(env.done[q_len:].bool().all())    # parked from the start: they step like finished envs
    pol = _policy("chase", cfg)
    _drain(env, q, pol)
    rec = q.records().copy()
    _same_table(rec, ora, ("park", q_len, n))
    assert int(q.head) >= q_len and bool((env.ticket == -1).all())
    assert bool((q._rec[q_len:] == sentinel).all())
    # one record per episode counted: no entry was recorded twice
    assert int(env.state_field("env_int")[:, abi.EI_EPISODES].sum()) == q_len
    head = int(q.head)
    for _ in range(20):
        env.step(pol((env.obs_num, env.lasers)), auto_reset="queue")
    assert q.records().tobytes() == rec.tobytes() and int(q.head) == head
    assert bool((q._rec[q_len:] == sentinel).all())
    assert float(env.episode_metrics()[abi.M_EPISODES]) == q_len
    env.close()


# ---------------------------------------------------------------- 4. done at reset
def test_done_at_reset_is_recorded_and_the_slot_moves_on(lanes_per_env):
    """Entry 0 of a hand-built pool has an empty route -- the world ``reset`` leaves done (ENV:508-510) --, entry 1 starts the follower
    inside a rock: that one is NOT done at reset, it crashes in its first frame and is an ordinary one-call episode."""
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool
    cfg, _ = _cfg_pool("B")
    pool = ScenarioPool.from_npz(cfg, GOLDEN + "/pool_B.npz", "cuda:0", limit=16)
    pool.t["route_len"][0] = 0
    pool.t["static_rects"][1, cfg.c.n_static - 1] = pool.t["robot_rect"][1, 1]      # the last rock, moved onto the follower
    scen = torch.tensor([0, 5, 1, 0, 6, 7, 0, 1, 8, 9, 0, 3], dtype=torch.int32)
    ora = _oracle("B", "chase", lanes_per_env, pool_key="hand-built", cfg_pool=(cfg, pool), scen=scen)
    for n in (1, 2, 5):
        env = _vec(cfg, pool, n)
        q = env.set_episode_queue(scen, stream_base=S0)
        env.reset_from_queue()
        assert int(env.done[0]) == 1              # slot 0 holds entry 0: done at reset
        _drain(env, q, _policy("chase", cfg))
        rec = q.records()
        _same_table(rec, ora, ("done at reset", n))
        empty = scen.numpy() == 0
        assert (rec["flags"][empty] == abi.FTL_EPISODE_DONE_AT_RESET).all() and (rec["flags"][~empty] == 0).all()
        assert (rec["frames"][empty] == 0).all() and (rec["calls"][empty] == 0).all() and (rec["ret"][empty] == 0).all()
        assert (rec["status"][empty] == 0).all()
        rock = scen.numpy() == 1
        assert (rec["calls"][rock] == 1).all() and (rec["frames"][rock] == cfg.c.frames_per_step).all()
        assert (rec["status"][rock][:, 1] == abi.AGENT.index("crash")).all()
        if n == 1:                                # the slot went on to every later entry
            assert (rec["env"] == 0).all() and (rec["state"] == 2).all()
        m = env.episode_metrics().cpu().numpy()
        assert m[abi.M_EPISODES] == len(scen) and m[abi.M_FRAMES_SUM] == rec["frames"].sum()
        env.close()


# ---------------------------------------------------------------- 5. terminal observations
@pytest.mark.parametrize("name", ["B", "E", "F"])
def test_terminal_observations(name, lanes_per_env):
    cfg, pool = _cfg_pool(name)
    ora = _oracle(name, "hashed", lanes_per_env)
    env = _vec(cfg, pool, 64, final_obs=True)
    q = env.set_episode_queue(_queue_scen(pool), stream_base=S0)
    env.reset_from_queue()
    before = [env.ticket.clone()]
    seen = [0]

    def check(t):
        ended = env.ended.bool()
        tk = before[0][ended].long().cpu()
        assert bool((tk >= 0).all())
        for k in OBS:
            assert torch.equal(getattr(env, "final_" + k)[ended].cpu(), ora["term"][k][tk]), (name, t, k)
        term, trunc = env.terminated_truncated()
        assert torch.equal(term | trunc, ended) and not bool((term & trunc).any())
        assert torch.equal(trunc, ended & (env.status[:, 0] == abi.MISSION.index("finished_by_time")))
        # a restarted slot returns the terminal reward / done / status and the new episode's observation
        assert bool(env.done[ended].bool().all())
        seen[0] += int(ended.sum())
        before[0] = env.ticket.clone()
    _drain(env, q, _policy("hashed", cfg), check)
    assert seen[0] == Q
    _same_table(q.records(), ora, (name, "final_obs"))
    env.close()


# ---------------------------------------------------------------- 6. metrics
def _metrics_tree(per_slot):
    """ftl_episode_metrics' fixed order for one block of at most 256 envs: thread t holds env t, then a halving tree."""
    sm = np.zeros((256, abi.FTL_N_METRICS))
    sm[:len(per_slot)] = per_slot
    off = 128
    while off >= 1:
        sm[:off] += sm[off:2 * off]
        off //= 2
    return sm[0]


@pytest.mark.parametrize("name", ["B", "F"])
def test_metrics_are_the_column_sums(name):
    cfg, pool = _cfg_pool(name)
    n = 64
    env = _vec(cfg, pool, n)
    q = env.set_episode_queue(_queue_scen(pool), stream_base=S0)
    env.reset_from_queue()
    _drain(env, q, _policy("chase", cfg))
    rec = q.records()
    got = env.episode_metrics().cpu().numpy()
    st, ag = rec["status"][:, 0], rec["status"][:, 1]
    counts = [len(rec), None, rec["frames"].sum(), (st == abi.MISSION.index("success")).sum(), (ag == abi.AGENT.index("crash")).sum(),
              (ag == abi.AGENT.index("low_reward")).sum(), (ag == abi.AGENT.index("too_far_from_leader")).sum(),
              (st == abi.MISSION.index("finished_by_time")).sum()]
    for k, c in enumerate(counts):
        if c is not None:
            assert got[k] == float(c), (name, k)
    # the return sum in the order the device adds it: per slot in the order its episodes ended, then ftl_episode_metrics' tree
    per_slot = np.zeros((n, abi.FTL_N_METRICS))
    for r in rec:                                 # (a slot's tickets ascend over time)
        per_slot[r["env"], abi.M_RETURN_SUM] += r["ret"]
    assert np.array_equal(env.state_field("ep_stats")[:, abi.M_RETURN_SUM].cpu().numpy(), per_slot[:, abi.M_RETURN_SUM])
    assert got[abi.M_RETURN_SUM] == _metrics_tree(per_slot)[abi.M_RETURN_SUM]
    env.close()


# ---------------------------------------------------------------- 7. pipelined batch, shared queue
@pytest.mark.parametrize("name", ["B", "F"])
def test_pipelined_parts_share_one_queue(name, lanes_per_env):
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    cfg, pool = _cfg_pool(name)
    ora = _oracle(name, "hashed", lanes_per_env)
    env = PipelinedVecGame(256, parts=2, device="cuda:0", config=cfg)
    env.load_scenarios(pool)
    rec = env.evaluate(_policy("hashed", cfg), _queue_scen(pool), stream_ids=S0 + torch.arange(Q))
    _same_table(rec, ora, (name, "pipelined"))
    assert env.queue is None and env.games[0].queue is None          # evaluate detaches
    m = env.episode_metrics().cpu().numpy()
    assert m[abi.M_EPISODES] == Q and m[abi.M_FRAMES_SUM] == rec["frames"].sum()
    env.close()


# ---------------------------------------------------------------- 8. the bias the queue removes
def test_success_share_is_the_oracles_not_the_auto_resets(lanes_per_env):
    cfg, pool = _cfg_pool("B400")
    ora = _oracle("B400", "chase", lanes_per_env)
    pol = _policy("chase", cfg)
    env = _vec(cfg, pool, 64)
    box = []

    def counting(obs):
        box.append(1)
        return pol(obs)
    rec = env.evaluate(counting, _queue_scen(pool), stream_ids=None, check_every=4)
    calls = len(box)
    ok, late = abi.MISSION.index("success"), abi.MISSION.index("finished_by_time")
    share_q = float((rec["status"][:, 0] == ok).mean())
    share_o = float((ora["status"][:, 0] == ok).mean())
    late_q = float((rec["status"][:, 0] == late).mean())
    # evaluate() numbers the streams from 0; the oracle's table was played on S0 ..: config B draws nothing, so the episodes are the same
    assert np.array_equal(rec["frames"], ora["frames"]) and np.array_equal(rec["ret"], ora["ret"])
    env.close()
    auto = _vec(cfg, pool, 64)
    auto.reset(_queue_scen(pool)[:64])
    for _ in range(calls):
        auto.step(pol((auto.obs_num, auto.lasers)), auto_reset=True)
    m = auto.episode_metrics().cpu().numpy()
    share_a = m[abi.M_SUCCESS] / max(m[abi.M_EPISODES], 1.0)
    late_a = m[abi.M_TIMEOUT] / max(m[abi.M_EPISODES], 1.0)
    print("over %d calls: success share queue %.4f (oracle %.4f, %d episodes), auto_reset=True %.4f (%d episodes); "
          "share of episodes that reach the time limit: queue %.4f, auto_reset=True %.4f"
          % (calls, share_q, share_o, Q, share_a, int(m[abi.M_EPISODES]), late_q, late_a))
    assert share_q == share_o
    assert late_q == float((ora["status"][:, 0] == late).mean())
    auto.close()


# ---------------------------------------------------------------- 9. nothing else moved
@pytest.mark.parametrize("name", ["B", "F"])
def test_old_flags_after_attach_and_detach(name):
    cfg, pool = _cfg_pool(name)
    n = 96
    a, b = _vec(cfg, pool, n, final_obs=True), _vec(cfg, pool, n, final_obs=True)
    b.set_episode_queue(_queue_scen(pool), stream_base=S0)
    b.set_episode_queue(None)
    with pytest.raises(_lib.FtlError):
        b.step(torch.zeros(n, 2, dtype=torch.float64, device="cuda:0"), auto_reset="queue")
    idx = torch.arange(n, dtype=torch.int32) % pool.n
    pol = _policy("hashed", cfg)
    for e in (a, b):
        e.reset(idx)
    for t in range(24):
        mode = (False, True, "same_step", "next_step")[(t // 6) % 4]
        act = pol((a.obs_num, a.lasers))
        a.step(act, auto_reset=mode)
        b.step(act, auto_reset=mode)
        for k in ("obs_num", "lasers", "target", "reward", "done", "status", "ended", "restarted"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (name, t, k)
    for f in ("rb_pos", "rb_dbl", "rb_int", "env_dbl", "env_int", "ep_stats", "traj", "hist", "corr"):
        assert torch.equal(a.state_field(f), b.state_field(f)), (name, f)
    assert torch.equal(a.episode_metrics(), b.episode_metrics())
    a.close()
    b.close()


# ---------------------------------------------------------------- 10. queue, sampler and same-step on one handle
def _same_rows(a, b, what):
    for k, row in a.output_rows().items():
        assert torch.equal(row, b.output_rows()[k]), (what, k)


@pytest.mark.parametrize("final", [True, False], ids=["final buffers", "no final buffers"])
def test_three_restart_sources_on_one_handle(final, lanes_per_env):
    """A sampler stays attached to batch A while A plays a queue and while it steps in the other auto-reset modes: the handle's one
    restart scratch and its two call counters serve all of them.  B (a sampler of its own, never a queue) and C (never a sampler) are
    the yardsticks.  130 envs: three populated wavefronts of the queue's kernel, the last with a partial row, and a partial workgroup of
    the sampler's.  Without the final buffers the masks of both choosers live in the handle's scratch, and same-step, which needs
    the buffers, gives its turns to the in-kernel auto-reset."""
    from test_gpu_sampler import FIELDS, _new_sampler
    cfg, pool = _cfg_pool("B")
    n, q_len = 130, 200
    pol = _policy("hashed", cfg)
    A, B, C = (_vec(cfg, pool, n, final_obs=final) for _ in range(3))
    sa, sb = _new_sampler(pool), _new_sampler(pool)
    A.set_scenario_sampler(sa)
    B.set_scenario_sampler(sb)
    A.reset_from_sampler()
    B.reset_from_sampler()
    for t in range(20):
        A.step(pol((A.obs_num, A.lasers)), auto_reset="sample")
        B.step(pol((B.obs_num, B.lasers)), auto_reset="sample")
        _same_rows(A, B, ("sample", t))
    snap = A.snapshot()
    scen, streams = _queue_scen(pool, q_len), S0 + torch.arange(q_len)
    rec_a = A.evaluate(pol, scen, stream_ids=streams)
    assert A.sampler is sa and A.queue is None
    rec_c = C.evaluate(pol, scen, stream_ids=streams)
    assert (rec_a["state"] == 2).all()
    for c in (col[0] for col in abi.RECORD_DTYPE):
        assert np.array_equal(rec_a[c], rec_c[c]), c
    A.restore(snap, slot_stats=True)
    modes = ("sample", "same_step" if final else True, "sample", True, "next_step", "sample")
    for t in range(24):
        act = pol((B.obs_num, B.lasers))
        A.step(act, auto_reset=modes[t % len(modes)])
        B.step(act, auto_reset=modes[t % len(modes)])
        _same_rows(A, B, (modes[t % len(modes)], t))
    for f in FIELDS:
        assert torch.equal(A.state_field(f), B.state_field(f)), f
    assert torch.equal(A.episode_metrics(), B.episode_metrics())
    ta, tb = sa.table(), sb.table()
    assert int(ta["episodes"].sum()) > n
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    for e in (A, B, C):
        e.close()


def test_snapshot_and_state_dict_are_refused_with_a_queue():
    cfg, pool = _cfg_pool("B")
    env = _vec(cfg, pool, 8)
    env.set_episode_queue(_queue_scen(pool, 20))
    env.reset_from_queue()
    for f in (env.snapshot, env.state_dict):
        with pytest.raises(_lib.FtlError, match="episode queue"):
            f()
    env.set_episode_queue(None)
    assert len(env.snapshot()) == 8
    env.close()
