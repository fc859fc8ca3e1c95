"""GPU tests of the tanh hidden activation of the MLP policy (include/ftl.h: ``ftl_mlp.activation`` = FTL_MLP_ACT_TANH;
``mlp.MlpPolicy(..., activation="tanh")``): the act kernel against the numpy twin (tests/mlp_tanh_numpy.py) bit for bit, the edges of
tanh32 carried to the head and the action, the closed-loop rollout and the trajectory collection against the loops they replace, the parts
of a pipelined batch, and the ReLU policy built with the argument against the one built without it."""
import numpy as np
import pytest
import torch

import mlp_numpy as M
import mlp_tanh_numpy as MT
from continiousenvironment_follower_leader_amd import abi
from test_gpu_baseline import FIELDS, _fold
from test_gpu_collect import SHORT, TRAJ, _loop, _same_batches, _sigma
from test_gpu_mlp import DEV, KCH, OUTP, _capture, _in_width, _same, _vec

pytestmark = pytest.mark.gpu

HIDDEN = [(64, 64), (15,), (17,), (KCH + 1, 255), (33, 16, 31)]
HEADS = [("B_s1_chase", None, 2), ("Bcfs_s2_chase", None, 1), ("B_s1_chase", dict(discrete_action_space=True), 5)]


def _policy(env, widths, n_sets=1, seed=0, scale=0.1, nasty=True, **kw):
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
    rng = np.random.default_rng(seed)
    p = M.nasty_params(rng, n_sets, widths, scale) if nasty else (rng.standard_normal((n_sets, M.param_count(widths))) * scale).astype(np.float32)
    return MlpPolicy(env, widths, params=torch.from_numpy(p).to(DEV), n_sets=n_sets, **kw), p


def _put(env, x):
    env.policy_obs.copy_(torch.from_numpy(x).to(DEV).view_as(env.policy_obs))


# ---------------------------------------------------------------- 1. the act kernel equals the twin
@pytest.mark.parametrize("name, over, A", HEADS, ids=["box2", "turn", "discrete"])
@pytest.mark.parametrize("n, n_sets", [(33, 3), (15, 1)])
def test_act_equals_the_twin(name, over, A, n, n_sets):
    env = _vec(name, n, over=over)
    w0 = _in_width(env)
    lo, hi = M.bounds(env.cfg)
    kind = M.head_kind(env.cfg)
    for i, hidden in enumerate(HIDDEN):
        widths = (w0,) + hidden + (A,)
        pol, p = _policy(env, widths, n_sets, 10 * A + i, activation="tanh")
        assert pol.activation == "tanh"
        x = M.nasty_inputs(np.random.default_rng(1000 + 10 * A + i), n, w0)
        _put(env, x)
        got = pol.act()
        want = MT.population(p, widths, x, kind, lo, hi, n // n_sets, activation="tanh")
        assert got.dtype == (torch.int32 if A == 5 else torch.float64) and tuple(got.shape) == want.shape
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (widths, int((got.cpu() != torch.from_numpy(want)).sum()))
        relu = MT.population(p, widths, x, kind, lo, hi, n // n_sets, activation="relu")
        if A != 5:
            assert not np.array_equal(want, relu), widths                                      # the activation reaches the action
            assert len(np.unique(want)) > n // 3                                               # (the twin's) head is not saturated all over
    env.close()


# ---------------------------------------------------------------- 2. the edges of tanh32 reach the action
def test_act_keeps_the_edges_of_tanh32():
    """Constructed rows (tests/mlp_tanh_numpy.py: edge_probes, edge_case) whose hidden pre-activations are exactly the probe values and
    whose heads are 0.5 * tanh32(+-v): zeros and the cancellation range, both sides of the first exact 1, arguments at and beside a rintf
    tie of the exponent split, 1e30 and infinity, a NaN, and a net in which every value is -0.  First the twin alone: re-run with a
    correctly rounded float64 tanh cast to float32 its heads differ in every class in which two float32 tanh can differ (tiny, one, tie
    -- at 1e30 and infinity every tanh is exactly 1, there the probes check the range), and re-run with an activation that drops the sign
    of zero the -0 net gives +0.  Then the device must equal the exact twin: the raw heads of sample() bit for bit, and the actions."""
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
    widths, p, x, classes = MT.edge_case(180)
    rows = len(classes)
    cls = np.array(classes)
    pre = MT.first_layer(p[0], widths, x[:rows])
    for r, (c, v) in enumerate(MT.edge_probes()):
        if c == "nan":
            assert np.isnan(pre[r]).all()
            continue
        qa, ja, qb, jb = MT.EDGE_INF if np.isinf(v) else MT.EDGE_UNITS[r % 3]
        want = np.zeros(MT.EDGE_H, np.float32)
        want[ja], want[jb] = v, -v
        assert np.array_equal(pre[r], want) and not np.signbit(pre[r][want == 0]).any(), (r, c, v)    # exactly the probe, nothing else
    assert np.signbit(MT.first_layer(p[1], widths, x[rows:])).all()                                    # every pre-activation of set 1 is -0
    exact = MT.population_raw(p, widths, x, rows)
    wrong = MT.population_raw(p, widths, x, rows, activation=MT.tanh_f64)
    differ = (exact[:rows].view(np.uint32) != wrong[:rows].view(np.uint32)).all(1)
    for c in ("tiny", "one", "tie"):
        assert differ[cls == c].any(), c
    print("probes whose heads tell tanh32 from a rounded float64 tanh:", {c: "%d of %d" % (differ[cls == c].sum(), (cls == c).sum()) for c in ("tiny", "one", "tie", "range")})
    assert (np.abs(exact[:rows][cls == "range"]) == 0.5).all() and np.isnan(exact[:rows][cls == "nan"]).all()
    assert (exact[rows:].view(np.uint32) == 0x80000000).all()                                          # -0 stays -0 ...
    assert (MT.population_raw(p, widths, x, rows, activation="relu")[rows:].view(np.uint32) == 0).all()     # ... only if the activation keeps it
    finite = ~np.isnan(exact).any(1)
    assert (np.abs(exact[finite]) <= 0.5).all()                                                        # inside (-1, 1): no clip hides a bit

    env = _vec("B_s1_chase", 2 * rows)
    lo, hi = M.bounds(env.cfg)
    want_a = MT.population(p, widths, x, M.BOX2, lo, hi, rows)
    assert (want_a[~finite] == lo).all()                                                               # a NaN head goes to lo
    pol = MlpPolicy(env, widths, params=torch.from_numpy(p).to(DEV), n_sets=2, activation="tanh")
    _put(env, x)
    act = pol.act().cpu().numpy().copy()
    pol.sample()
    head, act2 = pol.head.cpu().numpy(), pol.action.cpu().numpy()
    print("device vs exact twin: %d of %d heads differ; vs the float64 tanh: %d" % ((head[finite].view(np.uint32) != exact[finite].view(np.uint32)).sum(),
                                                                                  head[finite].size, (head[finite].view(np.uint32) != wrong[finite].view(np.uint32)).sum()))
    assert np.array_equal(head[finite].view(np.uint32), exact[finite].view(np.uint32)), np.argwhere(head.view(np.uint32) != exact.view(np.uint32))[:8]
    assert np.isnan(head[~finite]).all()
    assert np.array_equal(act, want_a), np.argwhere(act != want_a)[:8]
    assert np.array_equal(act2, want_a)
    env.close()


# ---------------------------------------------------------------- 3. the loops
def test_rollout_is_the_loop():
    n, T, gamma, widths = 33, 6, 0.97, (180, 70, 33, 2)
    env = _vec("B_s1_chase", n)
    pol, _ = _policy(env, widths, 3, 50, nasty=False, activation="tanh")
    for t in range(3):                                             # envs under way
        env.step(pol.act())
    snap = env.snapshot()
    r = env.rollout_mlp(pol, T, gamma=gamma, record=True)
    assert len(r) == 4 and tuple(r[3].shape) == (T, n, 2)
    one = _capture(env, r)
    acts = one["acts"]
    assert bool((acts[1:] != acts[:-1]).any()) and bool(one["ro"][1].eq(T).any())          # the loop really is closed
    env.restore(snap, slot_stats=True)
    played = []

    def step(t):
        played.append(pol.act().clone())
        env.step(played[-1])
    ro = _fold(env, T, gamma, step)
    _same(env, ro, one, "loop")
    assert torch.equal(torch.stack(played), acts)
    # and the decisions are the tanh net's: the first block against the twin on the observations the snapshot holds
    env.restore(snap, slot_stats=True)
    x = env.policy_obs.cpu().numpy().reshape(n, -1)
    lo, hi = M.bounds(env.cfg)
    want = MT.population(pol.params.cpu().numpy(), widths, x, M.BOX2, lo, hi, n // 3)
    assert np.array_equal(acts[0].cpu().numpy(), want)
    env.close()


def test_collect_is_the_loop():
    from continiousenvironment_follower_leader_amd import mlp
    n, T, sets, widths = 33, 5, 3, (180, 70, 33, 2)
    env, ref = _vec("B_s1_chase", n, over=SHORT), _vec("B_s1_chase", n, over=SHORT)
    pol, p = _policy(env, widths, sets, 500, nasty=False, activation="tanh")
    pref = mlp.MlpPolicy(ref, widths, params=torch.from_numpy(p).to(DEV), n_sets=sets, activation="tanh")
    noise = torch.from_numpy(np.random.default_rng(501).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    sigma = torch.from_numpy(_sigma(502, sets, 2)).to(DEV)
    for b, q in ((env, pol), (ref, pref)):
        b.step(q.act())                                            # the first episode of the window is one step short: it ends inside it
    tr = env.collect_mlp(pol, T, noise, sigma, auto_reset="next_step")
    want = _loop(ref, pref, T, noise, sigma, "next_step")
    for k in TRAJ:
        assert torch.equal(getattr(tr, k), want[k]), k
    _same_batches(env, ref, "collect vs loop")
    kind = tr.kind.cpu().numpy()
    for k in (abi.FTL_TR_STEP, abi.FTL_TR_TRUNCATED, abi.FTL_TR_VOID):
        assert (kind == k).any(), k                                # the window passes an episode boundary and its restart
    # the recorded heads are the tanh net's on the recorded observations
    y = MT.population_raw(p, widths, tr.obs[0].cpu().numpy(), n // sets)
    assert np.array_equal(tr.head[0].cpu().numpy().view(np.uint32), y.view(np.uint32))
    env.close(), ref.close()


def test_zero_noise_is_act():
    n, sets, widths = 33, 3, (180, 70, 33, 2)
    env = _vec("B_s1_chase", n)
    pol, p = _policy(env, widths, sets, 600, activation="tanh")
    x = M.nasty_inputs(np.random.default_rng(601), n, 180)
    _put(env, x)
    act = pol.act().clone()
    sigma = torch.from_numpy(_sigma(602, sets, 2)).to(DEV)
    for noise in (None, torch.zeros(n, 2, dtype=torch.float32, device=DEV)):
        pol.action.fill_(3.0)
        assert torch.equal(pol.sample(noise, sigma), act)
        assert torch.equal(pol.obs.cpu(), torch.from_numpy(x))
        assert np.array_equal(pol.head.cpu().numpy().view(np.uint32), MT.population_raw(p, widths, x, n // sets).view(np.uint32))
    nz = torch.from_numpy(np.random.default_rng(603).standard_normal((n, 2)).astype(np.float32)).to(DEV)
    assert not torch.equal(pol.sample(nz, sigma), act)             # and a noise that is not zero reaches the action
    env.close()


def test_pipelined_matches_vec_game():
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    n, sets, T, widths = 1045, 5, 4, (180, 70, 33, 2)
    a, p = _vec("B_s1_chase", n, over=SHORT), _vec("B_s1_chase", n, cls=PipelinedVecGame, over=SHORT, parts=2)
    lo1 = p.shards[1].lo
    assert lo1 % (n // sets) != 0 and (lo1 - 1) // (n // sets) == lo1 // (n // sets)           # set 2 lies in both parts
    pa, params = _policy(a, widths, sets, 700, nasty=False, activation="tanh")
    pp = MlpPolicy(p, widths, params=torch.from_numpy(params).to(DEV), n_sets=sets, activation="tanh")
    assert [net.activation for _, _, net in pp._parts] == [abi.FTL_MLP_ACT_TANH] * 2
    for env, pol in ((a, pa), (p, pp)):
        env.step(pol.act())
    p.join()
    assert torch.equal(pa.action, pp.action)
    ra, rp = a.rollout_mlp(pa, T, gamma=0.9, record=True), p.rollout_mlp(pp, T, gamma=0.9, record=True)
    p.join()
    for u, v in zip(ra, rp):
        assert torch.equal(u, v)
    noise = torch.from_numpy(np.random.default_rng(701).standard_normal((T, n, 2)).astype(np.float32)).to(DEV)
    sigma = torch.from_numpy(_sigma(702, sets, 2)).to(DEV)
    a.reset(), p.reset()
    ta, tp = a.collect_mlp(pa, T, noise, sigma), p.collect_mlp(pp, T, noise, sigma)
    p.join()
    for k in TRAJ:
        assert torch.equal(getattr(ta, k), getattr(tp, k)), k
    _same_batches(a, p, "pipelined")
    a.close(), p.close()


# ---------------------------------------------------------------- 4. ReLU by name is ReLU by default
def test_relu_by_name_is_the_default():
    n, sets, widths = 33, 3, (180, 70, 33, 2)
    env = _vec("B_s1_chase", n)
    named, p = _policy(env, widths, sets, 800, activation="relu")
    plain, _ = _policy(env, widths, sets, 800)
    tanh, _ = _policy(env, widths, sets, 800, activation="tanh")
    assert named.activation == plain.activation == "relu"
    x = M.nasty_inputs(np.random.default_rng(801), n, 180)
    _put(env, x)
    a, b = named.act().clone(), plain.act().clone()
    assert torch.equal(a, b)
    lo, hi = M.bounds(env.cfg)
    assert torch.equal(a.cpu(), torch.from_numpy(M.population(p, widths, x, M.BOX2, lo, hi, n // sets)))
    assert not torch.equal(tanh.act(), a)
    snap = env.snapshot()
    r1 = [t.clone() for t in env.rollout_mlp(named, 3, record=True)]
    env.restore(snap, slot_stats=True)
    r2 = env.rollout_mlp(plain, 3, record=True)
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    env.close()
