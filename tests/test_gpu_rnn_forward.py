"""GPU tests of the recurrent net on a recorded sequence (include/ftl.h: ftl_rnn_forward; ``rnn.forward``, ``RecurrentPolicy.forward``,
``rnn.RecurrentCritic``): the one-launch kernel against the sequence twin (tests/rnn_seq_numpy.py) bit for bit on synthetic records that
hold every pattern the zero rule lives on, the limits, the carry from one call into the next, parts of a wider record into padded buffers,
the record of ``collect_rnn`` replayed onto its own heads and states, the critic with ``gae``, and the wrappers' refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import collect_numpy as CN
import rnn_numpy as R
import rnn_seq_numpy as RS
from continiousenvironment_follower_leader_amd import _lib, abi, mlp, rnn
from test_gpu_collect import SHORT, _sigma
from test_gpu_mlp import DEV, TILE, _vec
from test_gpu_rnn import BOTH, NETS, _eq, _rnn

pytestmark = pytest.mark.gpu

VOID = abi.FTL_TR_VOID


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call(widths, cell, flags, p, rec, state, B, state_at=None, lo=0, reward0="rec"):
    """``rnn.forward`` on blocks lo .. lo + B - 1 of a record; returns (head, h, state_out) as device tensors."""
    n, S = rec["obs"].shape[1], state.shape[1]
    head = torch.full((B, n, widths[-1]), 7.0, dtype=torch.float32, device=DEV)
    h = torch.full((B, n, cell), 7.0, dtype=torch.float32, device=DEV)
    so = torch.full((n, S), 7.0, dtype=torch.float32, device=DEV) if state_at is not None else None
    got = rnn.forward(widths, cell, _dev(p), _dev(rec["obs"][lo:lo + B]), _dev(rec["action"][lo:]), _dev(rec["reward"][lo:]), _dev(rec["kind"][lo:]),
                      _dev(state), _dev(rec["reward0"] if isinstance(reward0, str) else reward0), bool(flags & R.PREV_ACTION), bool(flags & R.PREV_REWARD),
                      out=head, h_out=h, state_out=so, state_at=state_at or 0)
    assert got is head
    return head, h, so


# ---------------------------------------------------------------- 1. the twin on synthetic records, no env
@pytest.mark.parametrize("w0", [180, 65])
@pytest.mark.parametrize("A", [2, 1, 5], ids=["box2", "turn", "discrete"])
@pytest.mark.parametrize("trunk, cell", NETS, ids=["c65", "c128", "c1", "c63", "c32", "c33"])
def test_sequence_equals_the_twin(trunk, cell, A, w0):
    for n, n_sets in ((33, 3), (15, 1)):
        for flags in (BOTH, 0, R.PREV_ACTION, R.PREV_REWARD):
            case = RS.synthetic(trunk, cell, A, w0, n, n_sets, flags)
            widths, p, st0, rec = case["widths"], case["params"], case["state"], case["rec"]
            RS.assert_patterns(rec, st0)                            # a VOID at block 0, two in a row, one followed by a non-VOID, live 0 on a non-zero row
            want = RS.forward(p, widths, cell, flags, rec["obs"], st0, rec["action"], rec["reward"], rec["kind"], rec["reward0"], n // n_sets)
            st_dev = _dev(st0)
            for B in (1, 2, 5):                                    # (the sequence is causal: a shorter call is a prefix of the twin's five blocks)
                for at in range(B):
                    head, h, so = _call(widths, cell, flags, p, rec, st0, B, at)
                    what = (n, flags, B, at)
                    assert _eq(head, want["head"][:B]), what
                    assert _eq(h, want["h"][:B]), what
                    assert _eq(so, want["read"][at]), what
            assert (want["read"][1:][rec["kind"] == VOID] == 0).all() and (want["read"][1:][rec["kind"] != VOID][:, -1] == 1).all()
            # a single block reads no record: the pointers may be left out
            got = rnn.forward(widths, cell, _dev(p), _dev(rec["obs"][:1]), state=st_dev, reward0=_dev(rec["reward0"]),
                              prev_action=bool(flags & R.PREV_ACTION), prev_reward=bool(flags & R.PREV_REWARD))
            assert _eq(got, want["head"][:1]) and _eq(st_dev, st0)


# ---------------------------------------------------------------- 2. the limits
def test_sequence_at_the_limits():
    """Three trunk layers of FTL_MLP_MAX_WIDTH, FTL_RNN_MAX_CELL units, the widest head and a_prev: the most LDS a workgroup asks for
    (125.25 KiB, above the 64 KiB a launch gets without asking), two full gate passes, c in both register sets of a lane."""
    n, cell, W = TILE + 1, abi.FTL_RNN_MAX_CELL, abi.FTL_MLP_MAX_WIDTH
    widths = (180, W, W, W, 5)
    p = RS.params(77, 1, widths, cell, BOTH, nasty=False)
    st0 = RS.random_state(79, n, R.dims(widths, cell, BOTH)[3])
    rec = RS.record(78, 2, n, 180, 5)
    assert (rec["kind"][0] == VOID).any() and (rec["kind"][0] != VOID).any()
    want = RS.forward(p, widths, cell, BOTH, rec["obs"], st0, rec["action"], rec["reward"], rec["kind"], rec["reward0"], n)
    head, h, so = _call(widths, cell, BOTH, p, rec, st0, 2, 1)
    assert _eq(head, want["head"]) and _eq(h, want["h"]) and _eq(so, want["read"][1])
    assert len(np.unique(want["head"].argmax(2))) > 1


# ---------------------------------------------------------------- 3. the carry
def test_one_call_equals_two():
    """B = 5 in one call equals blocks 0 .. 2 with state_at = 2, then blocks 2 .. 4 started from that state_out with reward0 = reward[1]."""
    (trunk, cell), A, w0, n, n_sets = NETS[0], 2, 180, 33, 3
    case = RS.synthetic(trunk, cell, A, w0, n, n_sets, BOTH)
    widths, p, st0, rec = case["widths"], case["params"], case["state"], case["rec"]
    whole, hw, _ = _call(widths, cell, BOTH, p, rec, st0, 5)
    first, h1, carry = _call(widths, cell, BOTH, p, rec, st0, 3, 2)
    second, h2, end = _call(widths, cell, BOTH, p, rec, carry.cpu().numpy(), 3, 2, lo=2, reward0=rec["reward"][1])
    assert _eq(first, whole[:3]) and _eq(second, whole[2:]) and _eq(h1, hw[:3]) and _eq(h2, hw[2:])
    _, _, end_whole = _call(widths, cell, BOTH, p, rec, st0, 5, 4)
    assert _eq(end, end_whole)
    assert (rec["kind"][1] == VOID).any() and bool((carry[_dev(rec["kind"][1] == VOID)] == 0).all())      # the carry holds wiped rows and live ones
    assert bool((carry[_dev(rec["kind"][1] != VOID)][:, -1] == 1).all())


# ---------------------------------------------------------------- 4. strides and parts (the C entry point itself)
def _raw(lib, widths, cell, flags, params, n_sets, eps, lo, n, B, t, S, pad):
    """ftl_rnn_forward on rows [lo, lo + n) of the full-width tensors ``t``: every block stride is the full tensor's, state rows are
    S + pad floats apart."""
    A, W0 = widths[-1], widths[0]
    N = t["obs"].shape[1]
    net = abi.Rnn()
    net.params, net.set_stride, net.n_sets, net.n_layers = params.data_ptr(), params.shape[1], n_sets, len(widths) - 2
    for l, w in enumerate(widths):
        net.width[l] = w
    net.env_first, net.envs_per_set, net.cell, net.flags = lo, eps, cell, flags
    net.state, net.state_stride = t["state"].data_ptr() + lo * (S + pad) * 4, S + pad
    arow = 16 if A == 2 else 8 if A == 1 else 4
    seq = abi.RnnSequence()
    seq.obs, seq.obs_block_bytes = t["obs"].data_ptr() + lo * W0 * 4, N * W0 * 4
    seq.action, seq.action_block_bytes = t["action"].data_ptr() + lo * arow, N * arow
    seq.reward, seq.reward_block_bytes = t["reward"].data_ptr() + lo * 8, N * 8
    seq.kind, seq.kind_block_bytes = t["kind"].data_ptr() + lo, N
    seq.reward0 = t["reward0"].data_ptr() + lo * 8
    NP = t["head"].shape[1]
    seq.head, seq.head_block_bytes = t["head"].data_ptr() + lo * A * 4, NP * A * 4
    seq.h, seq.h_block_bytes = t["h"].data_ptr() + lo * cell * 4, NP * cell * 4
    seq.state_out, seq.state_at = t["so"].data_ptr() + lo * S * 4, B - 1
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(lib.ftl_rnn_forward(mlp._device_handle(torch.device(DEV)), C.byref(net), B, n, C.byref(seq), stream), lib)


def test_parts_of_a_wider_record_into_padded_buffers():
    lib = _lib.load()
    (trunk, cell), A, w0, N, eps, n_sets, B, pad, NP = NETS[3], 2, 65, 40, 16, 3, 3, 3, 44
    widths = (w0,) + trunk + (A,)
    S = R.dims(widths, cell, BOTH)[3]
    p = RS.params(41, n_sets, widths, cell, BOTH)
    rec = RS.record(42, B, N, w0, A)
    st0 = RS.random_state(43, N, S)
    assert (rec["kind"] == VOID).any()
    state = torch.full((N, S + pad), 5.0, dtype=torch.float32, device=DEV)
    state[:, :S] = _dev(st0)
    keep = state.clone()
    base = dict(obs=_dev(rec["obs"]), action=_dev(rec["action"]), reward=_dev(rec["reward"]), kind=_dev(rec["kind"]), reward0=_dev(rec["reward0"]), state=state)

    def outs():
        return dict(head=torch.full((B, NP, A), 7.0, dtype=torch.float32, device=DEV), h=torch.full((B, NP, cell), 7.0, dtype=torch.float32, device=DEV),
                    so=torch.full((NP, S), 7.0, dtype=torch.float32, device=DEV))
    params = _dev(p)
    whole = outs()
    _raw(lib, widths, cell, BOTH, params, n_sets, eps, 0, N, B, dict(base, **whole), S, pad)
    assert torch.equal(state, keep)
    want = RS.forward(p, widths, cell, BOTH, rec["obs"], st0, rec["action"], rec["reward"], rec["kind"], rec["reward0"], eps)
    assert _eq(whole["head"][:, :N], want["head"]) and _eq(whole["h"][:, :N], want["h"]) and _eq(whole["so"][:N], want["read"][B - 1])
    parts = outs()
    for lo, n in ((7, 17), (24, 16)):                              # rows 7 .. 23 cross the boundary of sets 0 and 1; rows 24 .. 39 end in the cut set 2
        _raw(lib, widths, cell, BOTH, params, n_sets, eps, lo, n, B, dict(base, **parts), S, pad)
        assert torch.equal(state, keep)                            # net->state is read, never written
    for k in ("head", "h", "so"):
        rows = (slice(None), slice(7, N)) if k != "so" else (slice(7, N),)
        assert torch.equal(parts[k][rows], whole[k][rows]), k
        rest = parts[k].clone()
        rest[rows] = 7.0
        assert bool((rest == 7.0).all()) and bool((whole[k][(slice(None), slice(N, NP)) if k != "so" else slice(N, NP)] == 7.0).all()), k      # every other float survives


# ---------------------------------------------------------------- 5. the record of collect_rnn
def _replay_the_record(env, pol, T, A, join=lambda: None):
    n = env.n
    noise = torch.from_numpy(np.random.default_rng(501).standard_normal((T, n, A)).astype(np.float32)).to(DEV)
    sigma = None if A == 5 else torch.from_numpy(_sigma(502, pol.n_sets, A)).to(DEV)
    env.step(pol.act())                                             # envs under way, states live
    join()
    r_in = env.reward.clone()
    tr = env.collect_rnn(pol, T, noise, sigma, record_state=True)
    join()
    kind = tr.kind.cpu().numpy()
    for k in (abi.FTL_TR_STEP, abi.FTL_TR_TRUNCATED, abi.FTL_TR_VOID):
        assert (kind == k).any(), k
    so = torch.empty(n, pol.S, dtype=torch.float32, device=DEV)
    for t in range(T):
        head = pol.forward(tr, r_in, state_out=so, state_at=t)
        assert _eq(so, tr.state[t]), t
    assert tuple(head.shape) == (T, n, A) and _eq(head, tr.head)    # every row, VOID rows included
    assert (kind[:-1] == VOID).any() and bool((tr.head[1:][tr.kind[:-1] == VOID] != 0).any())
    if bool((r_in != 0).any()):
        assert not _eq(pol.forward(tr), tr.head)                    # the reward the first decision saw is part of the record
    return tr


def test_forward_replays_the_record():
    n, T, sets, widths, cell = 2 * TILE + 2, 12, 2, (180, 70, 33, 2), 65
    env = _vec("B_s1_chase", n, over=SHORT)
    pol, _ = _rnn(env, widths, cell, sets, 500, nasty=False)
    _replay_the_record(env, pol, T, 2)
    env.close()


def test_forward_replays_a_discrete_record():
    n, T, sets, widths, cell = 2 * TILE + 2, 5, 2, (180, 70, 33, 5), 65
    env = _vec("B_s1_chase", n, over=dict(SHORT, discrete_action_space=True))
    pol, _ = _rnn(env, widths, cell, sets, 510, nasty=False)
    _replay_the_record(env, pol, T, 5)
    env.close()


def test_forward_replays_a_pipelined_record():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    n, T, sets, widths, cell = 2 * TILE + 2, 12, 2, (180, 70, 33, 2), 65
    env = _vec("B_s1_chase", n, cls=PipelinedVecGame, over=SHORT, parts=2)
    pol, _ = _rnn(env, widths, cell, sets, 500, nasty=False)
    _replay_the_record(env, pol, T, 2, env.join)
    env.close()


# ---------------------------------------------------------------- 6. the critic
def test_critic_values_gae_and_carry():
    widths, cell, n, n_sets, T = (180, 64, 1), 32, 33, 3, 6
    flags = R.PREV_REWARD
    rec = RS.record(61, T + 1, n, 180, 2)
    p = RS.params(62, n_sets, widths, cell, flags)
    crit = rnn.RecurrentCritic(widths, cell, n_sets=n_sets, params=_dev(p))
    assert crit.device == torch.device(DEV) and crit.S == 2 * cell + 1
    traj = mlp.Trajectory(_dev(rec["obs"]), torch.zeros(T, n, 2, dtype=torch.float32, device=DEV), _dev(rec["action"]), _dev(rec["reward"]), _dev(rec["kind"]))
    st0 = RS.random_state(63, n, crit.S)
    want = RS.forward(p, widths, cell, flags, rec["obs"], st0, None, rec["reward"], rec["kind"], rec["reward0"], n // n_sets)
    values, carry = crit.values(traj, _dev(st0), _dev(rec["reward0"]))
    assert tuple(values.shape) == (T + 1, n) and _eq(values, want["head"][..., 0]) and _eq(carry, want["read"][T])
    so = torch.empty(n, crit.S, dtype=torch.float32, device=DEV)
    rnn.forward(widths, cell, crit.params, traj.obs, None, traj.reward, traj.kind, _dev(st0), _dev(rec["reward0"]), False, True, state_out=so, state_at=T)
    assert torch.equal(carry, so)
    adv, ret = mlp.gae(traj, values, 0.99, 0.95)
    wa, wr = CN.gae(rec["reward"], rec["kind"], want["head"][..., 0], 0.99, 0.95)
    assert _eq(adv, wa) and _eq(ret, wr)
    # None reads as a fresh state and a zero reward; out= reuses the pair
    zero = RS.forward(p, widths, cell, flags, rec["obs"], np.zeros_like(st0), None, rec["reward"], rec["kind"], None, n // n_sets)
    buf = (torch.full((T + 1, n), 7.0, dtype=torch.float32, device=DEV), torch.full((n, crit.S), 7.0, dtype=torch.float32, device=DEV))
    v2, c2 = crit.values(traj, out=buf)
    assert v2.data_ptr() == buf[0].data_ptr() and c2 is buf[1] and _eq(buf[0], zero["head"][..., 0]) and _eq(buf[1], zero["read"][T])
    # the views write into params: a loaded LSTMCell changes the values
    crit.load_lstm_cell(1, torch.nn.LSTMCell(crit.U - cell, cell))
    v3, _ = crit.values(traj, _dev(st0), _dev(rec["reward0"]))
    per = n // n_sets
    assert _eq(v3[:, :per], values[:, :per]) and not _eq(v3[:, per:2 * per], values[:, per:2 * per])


# ---------------------------------------------------------------- 7. the wrappers' refusals on device tensors
def test_refusals_on_device_tensors():
    widths, cell, B, n = (20, 8, 2), 4, 3, 6
    S = abi.rnn_widths(widths, cell, BOTH)[3]
    count = abi.rnn_param_count(widths, cell, BOTH)
    z = lambda *s, dt=torch.float32, dev=DEV: torch.zeros(*s, dtype=dt, device=dev)
    good = dict(widths=widths, cell=cell, params=z(2, count), obs=z(B, n, 20), action=z(B - 1, n, 2, dt=torch.float64), reward=z(B - 1, n, dt=torch.float64),
                kind=z(B - 1, n, dt=torch.uint8))
    assert tuple(rnn.forward(**good).shape) == (B, n, 2)
    for over in (dict(params=z(2, count, dev="cpu")), dict(obs=z(B, n, 20, dev="cpu")), dict(kind=z(B - 1, n, dt=torch.uint8, dev="cpu")),
                 dict(action=z(B - 1, n, 2, dt=torch.float64, dev="cpu")), dict(reward=z(B - 1, n, dt=torch.float64, dev="cpu")),
                 dict(state=z(n, S, dev="cpu")), dict(reward0=z(n, dt=torch.float64, dev="cpu")), dict(out=z(B, n, 2, dev="cpu")),
                 dict(h_out=z(B, n, cell, dev="cpu")), dict(state_out=z(n, S, dev="cpu")), dict(state_out=z(n, S), state_at=B),
                 dict(state=z(n, S + 1)), dict(out=z(B, n, 5)), dict(h_out=z(B, n, cell + 1)), dict(kind=z(B - 2, n, dt=torch.uint8)),
                 dict(action=z(B - 1, n, dt=torch.float64)), dict(obs=z(B, n, 21)), dict(params=z(4, count))):
        with pytest.raises(ValueError):
            rnn.forward(**dict(good, **over))
    with pytest.raises(NotImplementedError):
        rnn.forward(widths, 129, z(1, 1), z(B, n, 20))
    crit = rnn.RecurrentCritic((20, 8, 1), cell, device=DEV)
    traj = mlp.Trajectory(z(B, n, 20), z(B - 1, n, 2), z(B - 1, n, 2, dt=torch.float64), z(B - 1, n, dt=torch.float64), z(B - 1, n, dt=torch.uint8))
    v, carry = crit.values(traj)
    assert tuple(v.shape) == (B, n) and tuple(carry.shape) == (n, crit.S) and not v.any()
    with pytest.raises(ValueError, match="out"):
        crit.values(traj, out=(z(B - 1, n), z(n, crit.S)))
    with pytest.raises(ValueError, match="state"):
        crit.values(traj, state=z(n, crit.S + 1))
    with pytest.raises(ValueError, match="constant_follower_speed"):
        rnn.RecurrentCritic((20, 8, 1), cell, device=DEV, prev_action=True).values(traj)
    env = _vec("B_s1_chase", n)
    pol, _ = _rnn(env, (180, 8, 2), 8, 2, 1100, nasty=False)
    tr = env.collect_rnn(pol, 2)
    with pytest.raises(ValueError, match="reward0"):
        pol.forward(tr, z(n))
    with pytest.raises(ValueError, match="out"):
        pol.forward(tr, out=z(3, n, 2))
    with pytest.raises(ValueError, match="state_at"):
        pol.forward(tr, state_out=z(n, pol.S), state_at=2)
    with pytest.raises(ValueError, match="Trajectory"):
        pol.forward(tr.obs)
    env.close()
