"""GPU checks of the backward pass of the recurrent net (include/ftl.h: ``ftl_rnn_backward``; ``rnn.backward``, ``rnn.Net``): the device
against the twin (tests/rnn_backward_numpy.py) bit for bit -- the nets, heads and flags of the forward tests at 1, 2 and 5 blocks, spans
and groups, the limits, the zero rule's patterns, a call chained from two, parts of a padded wider record, the edges of the gates and
the ReLU --, overwrite, reproducibility, ``rnn.Net`` under autograd, the PPO loss of INTEGRATION.md on recorded trajectories, and the
wrapper's refusals on device tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_numpy as M
import rnn_backward_numpy as RB
import rnn_numpy as R
import rnn_seq_numpy as RS
import test_rnn_backward_abi as BA
from continiousenvironment_follower_leader_amd import _lib, abi, mlp, rnn
from test_gpu_collect import SHORT
from test_gpu_mlp import DEV, TILE, _vec
from test_gpu_rnn import BOTH, NETS, _rnn

pytestmark = pytest.mark.gpu
F = np.float32
VOID = abi.FTL_TR_VOID


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), bad.size, float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64)))))


def _call(case, cell, flags, out=None, dstate_out=True, dev=None):
    """``rnn.backward`` on a case of ``test_rnn_backward_abi.gpu_case``; returns (grad, dstate_out) as device tensors."""
    rec, B, n = case["rec"], case["rec"]["obs"].shape[0], case["rec"]["obs"].shape[1]
    d = dev or {k: _dev(v) for k, v in rec.items()}
    dso = torch.full((n, 2 * cell), 7.0, dtype=torch.float32, device=DEV) if dstate_out else None
    got = rnn.backward(case["widths"], cell, _dev(case["params"]), d["obs"], _dev(case["dhead"]), d["action"] if B > 1 else None,
                       d["reward"] if B > 1 else None, d["kind"] if B > 1 else None, _dev(case["state"]), d["reward0"], bool(flags & R.PREV_ACTION),
                       bool(flags & R.PREV_REWARD), out=out, dstate_in=_dev(case["dstate_in"]), dstate_out=dso)
    return got, dso


def _check(case, cell, flags, n_sets, what):
    want, wdso = BA.twin(case, cell, flags, n_sets)
    assert np.isfinite(want).all() and (want != 0).mean() > 0.05
    got, dso = _call(case, cell, flags)
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    _same(got, want, what)
    _same(dso, wdso, (what, "dstate_out"))
    return got, want


def _small(seed, widths, cell, flags, B, n, n_sets=1, kind=None):
    """A case on a small net with a record of its own."""
    A_ = widths[-1]
    rng = np.random.default_rng(seed)
    rec = RS.record(seed + 1, B, n, widths[0], A_)
    if kind is not None:
        rec["kind"] = kind
    dy = rng.standard_normal((B, n, A_)).astype(F)
    dy[rng.random((B, n)) < 0.2] = 0.0
    return dict(widths=widths, params=RS.params(seed + 2, n_sets, widths, cell, flags), state=RS.random_state(seed + 3, n, R.dims(widths, cell, flags)[3]),
                rec=rec, dhead=dy, dstate_in=(rng.standard_normal((n, 2 * cell)) * 0.3).astype(F))


# ---------------------------------------------------------------- 1. the device equals the twin
@pytest.mark.parametrize("flags", [BOTH, 0, R.PREV_ACTION, R.PREV_REWARD], ids=["both", "none", "action", "reward"])
@pytest.mark.parametrize("w0", [180, 65])
@pytest.mark.parametrize("A", [2, 1, 5], ids=["box2", "turn", "discrete"])
@pytest.mark.parametrize("trunk, cell", NETS, ids=["c65", "c128", "c1", "c63", "c32", "c33"])
def test_gradient_equals_the_twin(trunk, cell, A, w0, flags):
    for n, n_sets in ((33, 3), (15, 1)):
        for B in (1, 2, 5):                                        # (back-propagation is not causal: every B has a twin run of its own)
            case = BA.gpu_case(trunk, cell, A, w0, n, n_sets, flags, B)
            if B == 5:
                RS.assert_patterns(case["rec"], case["state"])      # a VOID at block 0, two in a row, one followed by a non-VOID
                assert (case["dhead"] == 0).all(-1).any() and (case["dhead"][:, 1] == 0).all()
            _check(case, cell, flags, n_sets, (n, B, flags))


# ---------------------------------------------------------------- 2. spans and groups
def test_spans_of_64_and_6_pairs_a_tile():
    widths, cell, B, n = (20, 16, 2), 8, 70, 40
    assert RB.plan(B, n, n) == (2, 4)
    _check(_small(70, widths, cell, BOTH, B, n), cell, BOTH, 1, "B = 70")


def test_a_second_group_of_tiles():
    widths, cell, B, n = (20, 8, 1), 4, 3, 22 * TILE + 5
    assert RB.plan(B, n, n) == (2, 2) and abi.FTL_RNN_BWD_SPAN // B == 21 and -(-n // TILE) == 23
    _check(_small(71, widths, cell, R.PREV_REWARD, B, n), cell, R.PREV_REWARD, 1, "23 tiles in groups of 21")


@pytest.mark.parametrize("B", [64, 65])
def test_one_span_and_two_a_tile(B):
    widths, cell, n = (20, 8, 2), 4, TILE + 1
    assert RB.plan(B, n, n) == (2, 2 if B == 64 else 4)
    _check(_small(72 + B, widths, cell, BOTH, B, n), cell, BOTH, 1, B)


# ---------------------------------------------------------------- 3. the limits
def test_gradient_at_the_limits():
    """180-256-256 with FTL_RNN_MAX_CELL units, the widest head and a_prev: two full gate passes (du travels through the carry rows),
    dc_next in both register sets of a lane, 149 KiB of LDS."""
    widths, cell, n, B = (180, 256, 256, 5), abi.FTL_RNN_MAX_CELL, TILE + 1, 2
    case = _small(77, widths, cell, BOTH, B, n)
    case["params"] = RS.params(77, 1, widths, cell, BOTH, nasty=False)
    assert (case["rec"]["kind"][0] == VOID).any() and (case["rec"]["kind"][0] != VOID).any()
    _check(case, cell, BOTH, 1, "limits")


# ---------------------------------------------------------------- 4. the zero rule in the carry
def test_void_patterns_cut_the_carry():
    widths, cell, B, n = (33, 16, 2), 40, 5, 15
    kind = np.zeros((B - 1, n), np.uint8)
    kind[0, 0] = VOID                                              # a VOID at block 0
    kind[1, 1] = kind[2, 1] = VOID                                 # two in a row
    kind[1, 2], kind[2, 2] = VOID, abi.FTL_TR_STEP                 # a VOID followed by a non-VOID
    kind[3, 3] = VOID
    case = _small(81, widths, cell, BOTH, B, n, kind=kind)
    assert kind[0, 0] == VOID and (kind[1:3, 1] == VOID).all() and kind[1, 2] == VOID and kind[2, 2] != VOID and (kind[:, 4:] != VOID).all()
    got, want = _check(case, cell, BOTH, 1, "void patterns")
    wrong = BA.twin(case, cell, BOTH, 1, no_void_cut=True)[0]
    assert (_bits(wrong) != _bits(want)).any()


def test_one_call_equals_two_chained():
    """Blocks 0 .. 2 and 3 .. 4 as two calls: the second starts from the rows block 3 read (``rnn.forward``'s ``state_out``), its
    ``dstate_out`` -- zeroed where kind[2] is VOID, the seam -- is the first call's ``dstate_in``.  ``dstate_out`` of the pair equals
    the single call's bit for bit; the weight gradients are sums in another order: their sum lies within the CPU test's float32 bound."""
    (trunk, cell), A, w0, n, n_sets = NETS[0], 2, 180, 33, 3
    case = BA.gpu_case(trunk, cell, A, w0, n, n_sets, BOTH, 5, dstate=False)
    widths, rec, dy = case["widths"], case["rec"], case["dhead"]
    whole, dso_whole = _call(case, cell, BOTH)
    mid = torch.empty(n, R.dims(widths, cell, BOTH)[3], dtype=torch.float32, device=DEV)
    rnn.forward(widths, cell, _dev(case["params"]), _dev(rec["obs"]), _dev(rec["action"]), _dev(rec["reward"]), _dev(rec["kind"]), _dev(case["state"]),
                _dev(rec["reward0"]), state_out=mid, state_at=3)
    second = dict(case, rec=dict(obs=rec["obs"][3:], action=rec["action"][3:], reward=rec["reward"][3:], kind=rec["kind"][3:], reward0=rec["reward"][2]),
                  dhead=dy[3:], state=mid.cpu().numpy())
    g2, dso2 = _call(second, cell, BOTH)
    seam = rec["kind"][2] == VOID
    assert seam.any() and not seam.all() and bool((dso2[_dev(seam)] != 0).any())
    dso2[_dev(seam)] = 0
    first = dict(case, rec=dict(obs=rec["obs"][:3], action=rec["action"][:2], reward=rec["reward"][:2], kind=rec["kind"][:2], reward0=rec["reward0"]),
                 dhead=dy[:3], dstate_in=dso2.cpu().numpy())
    g1, dso1 = _call(first, cell, BOTH)
    assert torch.equal(dso1.view(torch.int32), dso_whole.view(torch.int32))
    both, one = (g1.double() + g2.double()).cpu().numpy(), whole.double().cpu().numpy()
    for s in range(n_sets):
        for sl in BA.tensors(widths, cell, BOTH):
            assert np.abs(both[s][sl] - one[s][sl]).max() <= BA.F32_BOUND * np.abs(one[s][sl]).max(), (s, sl)


# ---------------------------------------------------------------- 5. parts of a padded wider record (the C entry point itself)
def test_parts_of_a_wider_record_and_untouched_words():
    lib = _lib.load()
    (trunk, cell), A, w0, N, eps, n_sets, B, pad = NETS[3], 2, 65, 40, 16, 3, 3, 3
    widths = (w0,) + trunk + (A,)
    S, count = R.dims(widths, cell, BOTH)[3], R.param_count(widths, cell, BOTH)
    case = _small(41, widths, cell, BOTH, B, N, n_sets)
    p, rec, st0, dy = case["params"], case["rec"], case["state"], case["dhead"]
    assert (rec["kind"] == VOID).any()
    stride, sentinel = count + 5, F(12345.678)
    pp = torch.zeros(n_sets, stride, dtype=torch.float32, device=DEV)
    pp[:, :count] = _dev(p)
    state = torch.full((N, S + pad), 5.0, dtype=torch.float32, device=DEV)
    state[:, :S] = _dev(st0)
    keep = state.clone()
    t = dict(obs=_dev(rec["obs"]), action=_dev(rec["action"]), reward=_dev(rec["reward"]), kind=_dev(rec["kind"]), reward0=_dev(rec["reward0"]))
    dyd = torch.full((B, N * A + pad), float("nan"), dtype=torch.float32, device=DEV)
    dyd[:, :N * A] = _dev(dy.reshape(B, -1))
    for lo, n in ((7, 17), (24, 16), (0, 40)):                     # sets 0 and 1, both cut; set 1 cut and the cut set 2; everything
        net = abi.Rnn()
        net.params, net.set_stride, net.n_sets, net.n_layers = pp.data_ptr(), stride, n_sets, len(widths) - 2
        for l, w in enumerate(widths):
            net.width[l] = w
        net.env_first, net.envs_per_set, net.cell, net.flags = lo, eps, cell, BOTH
        net.state, net.state_stride = state.data_ptr() + lo * (S + pad) * 4, S + pad
        seq = abi.RnnSequence()
        seq.obs, seq.obs_block_bytes = t["obs"].data_ptr() + lo * w0 * 4, N * w0 * 4
        seq.action, seq.action_block_bytes = t["action"].data_ptr() + lo * 16, N * 16
        seq.reward, seq.reward_block_bytes = t["reward"].data_ptr() + lo * 8, N * 8
        seq.kind, seq.kind_block_bytes = t["kind"].data_ptr() + lo, N
        seq.reward0 = t["reward0"].data_ptr() + lo * 8
        need = lib.ftl_sizeof_rnn_backward_workspace(C.byref(net), B, n)
        assert need == RB.workspace_bytes(widths, cell, BOTH, B, n, eps, lo)
        ws = torch.full((need // 4 + 2,), 3.0, dtype=torch.float32, device=DEV)
        grad = torch.full((n_sets, stride), float(sentinel), dtype=torch.float32, device=DEV)
        dso = torch.full((N, 2 * cell), 9.0, dtype=torch.float32, device=DEV)
        g = abi.RnnGradient()
        g.dhead, g.dhead_block_bytes, g.grad = dyd.data_ptr() + lo * A * 4, (N * A + pad) * 4, grad.data_ptr()
        g.workspace, g.workspace_bytes, g.dstate_out = ws.data_ptr(), need, dso.data_ptr() + lo * 2 * cell * 4
        _lib.check(lib.ftl_rnn_backward(mlp._device_handle(torch.device(DEV)), C.byref(net), B, n, C.byref(seq), C.byref(g),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
        torch.cuda.synchronize()
        rows = slice(lo, lo + n)
        want, wdso = RB.population_grad(p, widths, cell, BOTH, rec["obs"][:, rows], dy[:, rows], st0[rows], rec["action"][:, rows], rec["reward"][:, rows],
                                        rec["kind"][:, rows], rec["reward0"][rows], eps, env_first=lo, fill=sentinel)
        touched = sorted(set((lo + np.arange(n)) // eps))
        assert (want[[s for s in range(n_sets) if s not in touched]] == sentinel).all() and (len(touched) < n_sets) == (n < N)
        _same(grad[:, :count], want, (lo, n))
        assert bool((grad[:, count:] == float(sentinel)).all())   # the stride's padding
        _same(dso[rows], wdso, (lo, n, "dstate_out"))
        rest = dso.clone()
        rest[rows] = 9.0
        assert bool((rest == 9.0).all()) and bool((ws[need // 4:] == 3.0).all())
        assert torch.equal(state, keep)                            # net->state is read, never written


# ---------------------------------------------------------------- 6. overwrite, rows left out, reproducibility
def test_overwrite_zero_rows_and_reproducibility():
    (trunk, cell), A, w0, n, n_sets = NETS[4], 2, 65, 33, 3
    case = BA.gpu_case(trunk, cell, A, w0, n, n_sets, BOTH, 5, dstate=False)
    out = torch.full(case["params"].shape, float("nan"), dtype=torch.float32, device=DEV)
    got, dso = _call(case, cell, BOTH, out=out)
    assert got is out and bool(torch.isfinite(out).all())          # every word overwritten
    again, dso2 = _call(case, cell, BOTH)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)) and torch.equal(dso.view(torch.int32), dso2.view(torch.int32))
    # a row whose dhead is zero in every block (and whose state gradient is) contributes nothing: other observations there, the same
    # gradient (up to the sign of a zero sum)
    assert (case["dhead"][:, 1] == 0).all()
    other = dict(case, rec=dict(case["rec"], obs=case["rec"]["obs"].copy()))
    other["rec"]["obs"][:, 1] = np.random.default_rng(4).random((5, w0), dtype=F) * 3
    assert torch.equal(out, _call(other, cell, BOTH)[0])
    nothing = dict(case, dhead=np.zeros_like(case["dhead"]))
    g0, d0 = _call(nothing, cell, BOTH, out=torch.full_like(out, float("nan")))
    assert bool((g0 == 0).all()) and bool((d0 == 0).all())


# ---------------------------------------------------------------- 7. the edges of the gates and the ReLU
def test_saturated_gates_and_relu_edges():
    """Gate pre-activations driven to +-100 (sig32 gives 1 and 4.5e-38, tanh32 +-1: the derivative lines run on 0, 1 and subnormal
    products) and trunk pre-activations of exactly +0, -0 and +- subnormal (columns of +-0 weights with such a bias): the select keeps
    only acc > 0.  Asserted on the inputs; the device equals the twin bit for bit."""
    widths, cell, flags, B, n = (20, 16, 2), 8, BOTH, 3, 15
    case = _small(91, widths, cell, flags, B, n)
    p = case["params"] = RS.params(93, 1, widths, cell, flags, nasty=False)
    trunk, Wg, bg, Wy, by = R.split(p[0], widths, cell, flags)
    (W1, b1), = M.layers(trunk, widths[:-1])
    sub = F(2.0 ** -140)
    for col, (w, b) in enumerate(((F(0.0), F(0.0)), (F(-0.0), F(-0.0)), (F(0.0), sub), (F(0.0), -sub))):
        W1[:, col], b1[col] = w, b
    case["rec"]["obs"] = np.random.default_rng(92).random((B, n, widths[0]), dtype=F) + F(0.5)      # positive inputs: a product with -0 is -0
    for j, v in enumerate((100.0, -100.0, 100.0, -100.0)):        # cells 0 .. 3 of i and f, g and o alternate
        bg[j], bg[cell + j], bg[2 * cell + j], bg[3 * cell + j] = v, -v, v, -v
    acc = R.chain(case["rec"]["obs"].reshape(B * n, -1), W1, b1)
    assert (acc[:, 0] == 0).all() and not np.signbit(acc[:, 0]).any() and (acc[:, 1] == 0).all() and np.signbit(acc[:, 1]).all()
    assert (acc[:, 2] == sub).all() and (acc[:, 3] == -sub).all()
    fw = RB.forward_values(RB._Arith(False, R.exp32), p[0], widths, cell, flags, case["rec"]["obs"], case["state"], case["rec"]["action"],
                           case["rec"]["reward"], case["rec"]["kind"], case["rec"]["reward0"])
    i0, g0 = np.concatenate([v["i"][:, :4] for v in fw]), np.concatenate([v["g"][:, :4] for v in fw])
    assert (i0[:, 0] == 1).all() and (0 < i0[:, 1]).all() and (i0[:, 1] < 1e-37).all() and (g0[:, 0] == 1).all() and (g0[:, 1] == -1).all()
    got, want = _check(case, cell, flags, 1, "edges")
    ge = _bits(BA.twin(case, cell, flags, 1, two_roundings=True)[0])
    assert (ge != _bits(want)).any()


# ---------------------------------------------------------------- 8. rnn.Net under autograd
def test_net_under_autograd_and_shared_storage():
    (trunk, cell), A, w0, n, n_sets = NETS[5], 2, 180, 32, 2
    env = _vec("B_s1_chase", n)
    widths = (w0,) + trunk + (A,)
    pol, p = _rnn(env, widths, cell, n_sets, 300, nasty=False)
    net = rnn.Net(widths, cell, n_sets=n_sets, params=pol.params)
    assert isinstance(net, torch.nn.Module) and [tuple(q.shape) for q in net.parameters()] == [p.shape]
    assert net.params.data_ptr() == pol.params.data_ptr()         # the policy's own tensor
    case = BA.gpu_case(trunk, cell, A, w0, n, n_sets, BOTH, 5, dstate=False)
    rec = {k: _dev(v) for k, v in case["rec"].items()}
    seq, st, dyd = (rec["obs"], rec["action"], rec["reward"], rec["kind"]), _dev(case["state"]), _dev(case["dhead"])
    y = net(seq, st, rec["reward0"])
    assert y.requires_grad and torch.equal(y, rnn.forward(widths, cell, pol.params, *seq, st, rec["reward0"]))
    y.backward(dyd)
    want = rnn.backward(widths, cell, pol.params, rec["obs"], dyd, rec["action"], rec["reward"], rec["kind"], st, rec["reward0"])
    assert torch.equal(net.params.grad.view(torch.int32), want.view(torch.int32)) and bool((want != 0).any())
    net(seq, st, rec["reward0"]).backward(dyd)                     # a second backward accumulates
    assert torch.equal(net.params.grad, want + want)
    with pytest.raises(ValueError, match="backward"):
        rnn.forward(widths, cell, net.params, *seq, st, rec["reward0"])      # forward() itself keeps refusing
    before = pol.params.clone()
    torch.optim.SGD(net.parameters(), 1e-3).step()                 # what the optimizer writes is what the policy plays next
    assert torch.allclose(pol.params, before - 1e-3 * (want + want), rtol=1e-6, atol=1e-9) and not torch.equal(pol.params, before)
    # a Trajectory of collect_rnn: obs[:-1] from state[0]
    traj = env.collect_rnn(pol, 3)
    head = net(traj, reward0=None)
    assert tuple(head.shape) == (3, n, A) and torch.equal(head, rnn.forward(widths, cell, pol.params.detach(), traj.obs[:-1], traj.action, traj.reward,
                                                                             traj.kind, traj.state[0]))
    env.close()


# ---------------------------------------------------------------- 9. the PPO loss of INTEGRATION.md on recorded trajectories
@pytest.mark.parametrize("A, T", [(2, 12), (5, 5)], ids=["box2-T12", "discrete-T5"])
def test_ppo_loss_on_collect_rnn_trajectories(A, T):
    """The recurrent PPO example: ``collect_rnn`` trajectories with VOID rows, the actor's and the critic's gradients through ``rnn.Net``
    with one loss; each equals the twin on the head gradient autograd handed down, bit for bit."""
    n, sets, cell = 2 * TILE + 2, 2, 33
    env = _vec("B_s1_chase", n, over=dict(SHORT, discrete_action_space=True) if A == 5 else SHORT)
    W0 = env.policy_obs.shape[1] * env.policy_obs.shape[2]
    wa, wc = (W0, 20, A), (W0, 16, 1)
    pol, pa = _rnn(env, wa, cell, sets, 500 + A, nasty=False)
    pc = RS.params(600 + A, sets, wc, cell, R.PREV_REWARD, nasty=False)
    crit = rnn.RecurrentCritic(wc, cell, n_sets=sets, params=_dev(pc))
    actor, value = rnn.Net(wa, cell, sets, params=pol.params), rnn.Net(wc, cell, sets, prev_action=False, params=crit.params)
    rng = np.random.default_rng(15)
    noise = _dev(rng.standard_normal((T, n, A)).astype(F))
    log_std = torch.full((1, 2), -1.0, device=DEV)
    env.step(pol.act())
    with torch.no_grad():
        r_in = env.reward.clone()
        v_state = torch.zeros(n, crit.S, device=DEV)
        traj = env.collect_rnn(pol, T, noise, None if A == 5 else log_std.exp().expand(sets, 2).contiguous())
        assert torch.equal(pol.forward(traj, r_in), traj.head)
        values, _ = crit.values(traj, v_state, r_in)
        adv, ret = mlp.gae(traj, values, gamma=0.99, lam=0.95)
        m = traj.valid
    assert bool((~m).any()) and bool(m.any())                      # VOID rows present
    heads = {}
    y = actor(traj, reward0=r_in)
    y.register_hook(lambda gr: heads.__setitem__("a", gr))
    v = value(traj, v_state, r_in)
    v.register_hook(lambda gr: heads.__setitem__("c", gr))
    if A == 5:
        logp = torch.log_softmax(y, -1).gather(-1, traj.action.long()[..., None].clamp(0, 4))[..., 0]
        logp_old = torch.log_softmax(traj.head, -1).gather(-1, traj.action.long()[..., None].clamp(0, 4))[..., 0]
    else:
        sigma = log_std.exp()
        z = traj.head + sigma * noise
        logp = (-0.5 * ((z - y) / sigma) ** 2 - sigma.log() - 0.9189385332).sum(-1)
        logp_old = (-0.5 * noise ** 2 - sigma.log() - 0.9189385332).sum(-1)
    ratio = (logp - logp_old).exp()
    a = (adv - adv[m].mean()) / (adv[m].std() + 1e-8)
    loss = (-torch.min(ratio * a, ratio.clamp(0.8, 1.2) * a) + 0.5 * (v.squeeze(-1) - ret) ** 2)[m].mean()
    loss.backward()
    assert bool((heads["a"][~m] == 0).all()) and bool((heads["c"][~m] == 0).all())       # the rows left out carry zeros
    obs, kind = traj.obs[:-1].cpu().numpy(), traj.kind.cpu().numpy()[:T - 1]
    for net_, p_, w_, flags, st, dy in ((actor, pa, wa, BOTH, traj.state[0], heads["a"]), (value, pc, wc, R.PREV_REWARD, v_state, heads["c"])):
        want, _ = RB.population_grad(p_, w_, cell, flags, obs, dy.cpu().numpy(), st.cpu().numpy(), traj.action.cpu().numpy()[:T - 1],
                                     traj.reward.cpu().numpy()[:T - 1], kind, r_in.cpu().numpy(), n // sets)
        assert bool(torch.isfinite(net_.params.grad).all()) and bool((net_.params.grad != 0).any())
        _same(net_.params.grad, want, (A, T, flags))
    env.close()


# ---------------------------------------------------------------- 10. the wrapper's refusals on device tensors
def test_wrapper_refuses_on_device_tensors():
    widths, cell, B, n = (20, 8, 2), 4, 3, 6
    S, count = abi.rnn_widths(widths, cell, BOTH)[3], abi.rnn_param_count(widths, cell, BOTH)
    z = lambda *s, dt=torch.float32, dev=DEV: torch.zeros(*s, dtype=dt, device=dev)
    good = dict(widths=widths, cell=cell, params=z(2, count), obs=z(B, n, 20), dhead=z(B, n, 2), action=z(B - 1, n, 2, dt=torch.float64),
                reward=z(B - 1, n, dt=torch.float64), kind=z(B - 1, n, dt=torch.uint8))
    g = rnn.backward(**good)
    assert tuple(g.shape) == (2, count) and not g.any()
    for over in (dict(params=z(2, count, dev="cpu")), dict(dhead=z(B, n, 2, dev="cpu")), dict(dhead=z(B, n, 3)), dict(dhead=z(B, n, 2, dt=torch.float64)),
                 dict(dhead=z(B, n, 2).requires_grad_()), dict(obs=z(B, n, 20).requires_grad_()), dict(params=z(2, count).requires_grad_()),
                 dict(out=z(2, count + 1)), dict(out=z(2, count, dev="cpu")), dict(dstate_in=z(n, 2 * cell + 1)), dict(dstate_out=z(n, 2 * cell, dev="cpu")),
                 dict(state=z(n, S + 1)), dict(kind=z(B - 2, n, dt=torch.uint8)), dict(action=z(B - 1, n, dt=torch.float64)), dict(params=z(4, count))):
        with pytest.raises(ValueError):
            rnn.backward(**dict(good, **over))
    with pytest.raises(NotImplementedError):
        rnn.backward(widths, 129, z(1, 1), z(B, n, 20), z(B, n, 2))
    wide = (20, 256, 256, 256, 2)                                  # inside ftl_rnn's limits, beyond the LDS of the backward kernel
    with pytest.raises(NotImplementedError, match="LDS"):
        rnn.backward(wide, 128, z(1, abi.rnn_param_count(wide, 128, 0)), z(1, n, 20), z(1, n, 2), prev_action=False, prev_reward=False)
    net = rnn.Net(widths, cell, n_sets=2, device=DEV)
    with pytest.raises(ValueError, match="grad"):
        net((z(B, n, 20).requires_grad_(), good["action"], good["reward"], good["kind"]))
    with pytest.raises(ValueError, match="Trajectory"):
        net(z(B, n, 20))
