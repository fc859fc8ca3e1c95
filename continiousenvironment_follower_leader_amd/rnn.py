"""A recurrent policy on the device, or a population of them: ``RecurrentPolicy`` is a trunk of dense ReLU layers, one LSTM cell and a
linear head on the batch's ``policy_obs`` (the reference's ``*_lstm`` architectures with ``lstm_use_prev_action`` /
``lstm_use_prev_reward``).  One decision with its state update is one launch (``ftl_rnn_act``); ``batch.rollout_rnn`` closes the loop over T
steps and ``batch.collect_rnn`` records a PPO-ready trajectory through episode boundaries, each with one call.  The arithmetic is fixed
operation by operation, ``sigmoid`` and ``tanh`` included (the ``ftl_rnn_act`` block of ``include/ftl.h``).

The state is a ``[N, S]`` float32 tensor, a row ``h | c | a_prev | live``; the device zeroes a row at the episode boundary, so that no
memory of a finished episode leaks into the next one: after the void decision at a finished env (``auto_reset`` False or "next_step"), or
before the first decision on the new episode's observation ("same_step", "queue", "sample").

A recorded sequence goes back through a recurrent net in one launch (``ftl_rnn_forward``): ``forward`` evaluates any net on recorded blocks
with the state carried from block to block and zeroed after VOID rows as ``collect_rnn`` did, ``RecurrentPolicy.forward(traj)`` is the
actor's replay -- ``traj.head`` bit for bit --, and ``RecurrentCritic`` is a head-1 net with memory whose ``values(traj)`` feed ``gae()``.
``backward`` is back-propagation through time on the same record (``ftl_rnn_backward``), and ``Net`` is the ``nn.Module`` over the two whose
parameter can be ``RecurrentPolicy.params`` or ``RecurrentCritic.params`` itself."""
import ctypes as C

import torch

from . import _lib, abi
from .mlp import MlpPolicy, Trajectory, _check_params, _device_handle, _held_params, _lead_blocks, _workspace, check_net_widths, check_widths

_BEFORE = ("same_step", "queue", "sample")


def _flags(prev_action, prev_reward):
    return (abi.FTL_RNN_PREV_ACTION if prev_action else 0) | (abi.FTL_RNN_PREV_REWARD if prev_reward else 0)


def _rnn_struct(widths, cell, flags, params, n_sets, envs_per_set, state, env_first=0):
    """The ``abi.Rnn`` of checked arguments: rows from ``env_first`` on, ``envs_per_set`` of them to a weight set; ``state`` is the
    ``[rows, S]`` tensor whose row 0 belongs to env 0."""
    S = abi.rnn_widths(widths, cell, flags)[3]
    net = abi.Rnn()
    net.params, net.set_stride, net.n_sets, net.n_layers = params.data_ptr(), abi.rnn_param_count(widths, cell, flags), n_sets, len(widths) - 2
    for l, w in enumerate(widths):
        net.width[l] = w
    net.env_first, net.envs_per_set, net.cell, net.flags = env_first, envs_per_set, cell, flags
    net.state, net.state_stride = state.data_ptr() + env_first * S * 4, S
    return net


class _RnnParams:
    """Views into ``params`` of a recurrent net (``widths``, ``trunk``, ``cell``, ``U``, ``n_sets``), shared by the policy and the critic."""

    def _hold(self, widths, cell, n_sets, prev_action, prev_reward, params, device, who, head=None):
        """The constructor body of ``RecurrentCritic`` and ``Net``: the checked shape and its derived widths, and the checked or new
        ``params`` tensor, which it returns (the critic keeps the tensor, the net wraps it); ``who`` names the class in the message."""
        self.widths, self.cell = check_rnn_widths(widths, cell)
        if head is not None and self.widths[-1] != head:
            raise ValueError("a critic's head is %d wide, not %d" % (head, self.widths[-1]))
        self.trunk = self.widths[:-1]
        self.prev_action, self.prev_reward = bool(prev_action), bool(prev_reward)
        self.flags = _flags(prev_action, prev_reward)
        self.P, self.R, self.U, self.S = abi.rnn_widths(self.widths, self.cell, self.flags)
        self.n_sets, self.param_count = int(n_sets), abi.rnn_param_count(self.widths, self.cell, self.flags)
        return _held_params(params, self.n_sets, self.param_count, device, who)

    def layer(self, l):
        """Views ``(W [n_sets, in, out], b [n_sets, out])`` of trunk layer ``l`` (0-based) in ``params``."""
        w = self.trunk
        if not 0 <= l < len(w) - 1:
            raise IndexError("trunk layer %d of %d" % (l, len(w) - 1))
        off = abi.mlp_param_count(w[:l + 1])
        nw = w[l] * w[l + 1]
        return self.params[:, off:off + nw].view(self.n_sets, w[l], w[l + 1]), self.params[:, off + nw:off + nw + w[l + 1]]

    def cell_weights(self):
        """Views ``(W_g [n_sets, U, 4C], b_g [n_sets, 4C])``: rows in the order ``x | a_prev | r_prev | h``, columns ``i | f | g | o``."""
        off, n = abi.mlp_param_count(self.trunk), self.U * 4 * self.cell
        return self.params[:, off:off + n].view(self.n_sets, self.U, 4 * self.cell), self.params[:, off + n:off + n + 4 * self.cell]

    def head_weights(self):
        """Views ``(W_y [n_sets, C, A], b_y [n_sets, A])``."""
        A = self.widths[-1]
        off = abi.mlp_param_count(self.trunk) + (self.U + 1) * 4 * self.cell
        n = self.cell * A
        return self.params[:, off:off + n].view(self.n_sets, self.cell, A), self.params[:, off + n:off + n + A]

    def load_lstm_cell(self, s, lstm):
        """Copy a ``torch.nn.LSTMCell(U - C, C)`` into set ``s``: ``weight_ih.T`` over ``weight_hh.T``, ``bias_ih + bias_hh``."""
        if lstm.input_size != self.U - self.cell or lstm.hidden_size != self.cell:
            raise ValueError("the cell takes %d inputs and has %d units, not %d and %d" % (self.U - self.cell, self.cell, lstm.input_size, lstm.hidden_size))
        W, b = self.cell_weights()
        with torch.no_grad():
            W[s, :self.U - self.cell].copy_(lstm.weight_ih.detach().t())
            W[s, self.U - self.cell:].copy_(lstm.weight_hh.detach().t())
            if lstm.bias:
                b[s].copy_((lstm.bias_ih.detach().to(torch.float32) + lstm.bias_hh.detach().to(torch.float32)))
            else:
                b[s].zero_()


class RecurrentPolicy(_RnnParams, MlpPolicy):
    """``n_sets`` recurrent nets on ``batch`` (a ``VecGame`` or a ``PipelinedVecGame`` built with ``policy_obs=True``): ``widths`` names
    the input width, the trunk's layers and the head width -- ``(180, 64, 64, 2)`` is 180 -> 64 -> 64 -> cell -> 2 --, ``cell`` the LSTM
    units; ``prev_action`` / ``prev_reward`` feed the last action (one-hot on Discrete(5)) and the last reward to the cell.  Env e uses
    set ``e // (batch.n // n_sets)``.

    ``params`` is the float32 ``[n_sets, param_count]`` device tensor of all weights (zeros unless given); ``layer(l)``,
    ``cell_weights()`` and ``head_weights()`` are views into it and ``load_lstm_cell`` copies a ``torch.nn.LSTMCell``.  ``state`` is the
    ``[N, S]`` state (zeros: every env at the start of an episode).  ``auto_reset`` names the reset discipline of the ``step`` calls that
    ``act()`` / ``sample()`` are used with: it decides where the state is zeroed.  ``act()``, ``sample()`` and the call operator return the
    persistent action tensor like ``MlpPolicy``; like ``step`` they do not join a pipelined batch."""

    _ROLLOUT, _COLLECT = "ftl_rollout_rnn", "ftl_collect_rnn"                          # (``rollout`` is ``MlpPolicy``'s)
    _COUNT_MISMATCH = "ftl_rnn_param_count disagrees with abi.rnn_param_count: library and package do not match"

    def __init__(self, batch, widths, cell, n_sets=1, params=None, prev_action=True, prev_reward=True, auto_reset="next_step"):
        widths = tuple(int(w) for w in widths)
        if len(widths) < 3:
            raise ValueError("widths must name the input width, at least one trunk layer and the head width")
        check_widths(batch.cfg, widths)                            # (the trunk and the head obey the limits of a feed-forward net one layer deeper)
        cell = int(cell)
        if cell < 1:
            raise ValueError("cell must be at least 1")
        if cell > abi.FTL_RNN_MAX_CELL:
            raise NotImplementedError("at most %d LSTM units" % abi.FTL_RNN_MAX_CELL)
        if auto_reset is not False and auto_reset != "next_step" and auto_reset not in _BEFORE:
            raise ValueError('auto_reset must be False, "next_step", "same_step", "queue" or "sample" (got %r)' % (auto_reset,))
        self.cell, self.auto_reset = cell, auto_reset
        self.flags = _flags(prev_action, prev_reward)
        self.P, self.R, self.U, self.S = abi.rnn_widths(widths, cell, self.flags)
        self.widths, self.trunk = widths, widths[:-1]
        self.param_count = abi.rnn_param_count(widths, cell, self.flags)
        self._bind(batch, n_sets, params)

    def _buffers(self):
        self.state = torch.zeros(self.n, self.S, dtype=torch.float32, device=self.device)
        self.head = torch.zeros(self.n, self.widths[-1], dtype=torch.float32, device=self.device)
        self.obs = torch.zeros(self.n, self.widths[0], dtype=torch.float32, device=self.device)

    def _lib_param_count(self):
        return self.lib.ftl_rnn_param_count((C.c_int32 * len(self.widths))(*self.widths), len(self.widths) - 2, self.cell, self.flags)

    def _net(self, env_first):
        return _rnn_struct(self.widths, self.cell, self.flags, self.params, self.n_sets, self.envs_per_set, self.state, env_first)

    def reset_state(self, env_ids=None):
        """Zero the state of every env, or of ``env_ids``: the rows of a fresh episode (after a ``batch.reset`` of those envs)."""
        if env_ids is None:
            self.state.zero_()
        else:
            self.state[torch.as_tensor(env_ids, device=self.device).long()] = 0

    # ------------------------------------------------------------------ decisions
    def _mode(self):
        return abi.FTL_RNN_ZERO_ON_OUT_DONE if self.auto_reset in _BEFORE else 0

    def act(self):
        """One deterministic decision of every env with its state update (``ftl_rnn_act``, one launch per part); returns ``action``."""
        return self.sample()

    def sample(self, noise=None, sigma=None, state_rec=None):
        """One decision of every env with its state update: ``noise`` / ``sigma`` as ``MlpPolicy.sample`` takes them (None: the
        deterministic map); the raw head and the observation rows are kept in ``self.head`` and ``self.obs``; ``state_rec`` (float32
        ``[N, S]``, optional) receives the state rows as the decision read them.  Returns ``action``."""
        self.batch._need_pool()
        self._check_noise(noise, sigma)
        if state_rec is not None and (not torch.is_tensor(state_rec) or state_rec.dtype != torch.float32 or tuple(state_rec.shape) != (self.n, self.S)
                                      or state_rec.device != self.device or not state_rec.is_contiguous()):
            raise ValueError("state_rec must be a contiguous float32 [N, %d] tensor on the batch's device" % self.S)
        A, W0, S = self.widths[-1], self.widths[0], self.S
        ap, hp, op = self.action.data_ptr(), self.head.data_ptr(), self.obs.data_ptr()
        for (g, lo, net), s in zip(self._parts, self._streams(noise)):
            _lib.check(self.lib.ftl_rnn_act(g.h, g._out_ref, C.byref(net), (noise.data_ptr() + lo * A * 4) if noise is not None else None,
                                            sigma.data_ptr() if sigma is not None else None, hp + lo * A * 4, op + lo * W0 * 4,
                                            (state_rec.data_ptr() + lo * S * 4) if state_rec is not None else None,
                                            ap + lo * self.row, self._mode(), s), self.lib)
        self._keep = (noise, sigma, state_rec)
        return self.action

    def collect(self, T, noise=None, sigma=None, auto_reset="next_step", out=None, record_state=False):
        """``batch.collect_rnn(self, ...)``."""
        return self._collect(T, noise, sigma, auto_reset, out, record_state)

    def _state_blocks(self, T, record_state):
        return dict(state=((T if record_state else 1, self.n, self.S), torch.float32))

    def _collect_struct(self, out, lo):
        rb = abi.RnnCollectBuffers()
        rb.state, rb.state_step_bytes, rb.state_steps = out.state.data_ptr() + lo * self.S * 4, self.n * self.S * 4, int(out.state.shape[0])
        return rb, rb.b

    def forward(self, traj, reward0=None, **outs):
        """The policy's own net -- its sets and its flags -- replayed on a trajectory its ``collect`` recorded, in one launch (the
        module's ``forward`` on ``traj.obs[:-1]`` from ``traj.state[0]``, with ``traj.action`` / ``reward`` / ``kind``): float32
        ``[T, N, A]``, which is ``traj.head`` bit for bit when ``reward0`` is ``batch.reward`` as it stood before the ``collect`` call (float64
        ``[N]``; None reads as zeros, right for envs that had not stepped yet).  ``outs`` are ``out``, ``h_out``, ``state_out`` and
        ``state_at`` of ``forward``: ``state_out`` at ``state_at=t`` is ``traj.state[t]`` of a ``record_state=True`` trajectory.  The launch
        goes to the current stream, not to the parts' streams: on a pipelined batch ``join()`` first."""
        if not isinstance(traj, Trajectory) or not torch.is_tensor(getattr(traj, "state", None)):
            raise ValueError("traj must be a Trajectory of collect_rnn (with its state blocks)")
        if not torch.is_tensor(traj.obs) or traj.obs.dim() != 3 or traj.obs.shape[0] < 2 or traj.obs.shape[1] != self.n:
            raise ValueError("traj.obs must be a [T + 1, N, H * W] tensor with the batch's N = %d rows a block" % self.n)
        return forward(self.widths, self.cell, self.params, traj.obs[:-1], traj.action, traj.reward, traj.kind, traj.state[0], reward0,
                       bool(self.flags & abi.FTL_RNN_PREV_ACTION), bool(self.flags & abi.FTL_RNN_PREV_REWARD), **outs)


def check_rnn_widths(widths, cell):
    """``(widths, cell)`` as ints inside the limits of ``ftl_rnn`` alone (no config): ``ValueError`` for a malformed net,
    ``NotImplementedError`` beyond the limits."""
    widths = tuple(int(w) for w in widths)
    if len(widths) < 3:
        raise ValueError("widths must name the input width, at least one trunk layer and the head width")
    widths = check_net_widths(widths)
    if widths[-1] not in (1, 2, 5):
        raise ValueError("the head width must be 2 (Box(2)), 1 (Box(1) turn) or 5 (Discrete(5)), not %d" % widths[-1])
    cell = int(cell)
    if cell < 1:
        raise ValueError("cell must be at least 1")
    if cell > abi.FTL_RNN_MAX_CELL:
        raise NotImplementedError("at most %d LSTM units" % abi.FTL_RNN_MAX_CELL)
    return widths, cell


def _is(t, dtype, shape, device):
    return torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.device == device and t.is_contiguous()


def _check_sequence(widths, cell, params, obs, action, reward, kind, state, reward0, prev_action, prev_reward, grad_msg):
    """The checks ``forward`` and ``backward`` share, in ``forward``'s order; returns ``(widths, cell, flags, count, n_sets, B, N, dev)``."""
    widths, cell = check_rnn_widths(widths, cell)
    A, W0 = widths[-1], widths[0]
    flags = _flags(prev_action, prev_reward)
    P, R, U, S = abi.rnn_widths(widths, cell, flags)
    count = abi.rnn_param_count(widths, cell, flags)
    n_sets = int(_check_params(params, count).shape[0])
    if not (torch.is_tensor(obs) and obs.dtype == torch.float32 and obs.dim() == 3 and obs.shape[2] == W0 and obs.is_contiguous()):
        raise ValueError("obs must be a contiguous float32 [B, N, %d] tensor" % W0)
    if obs.requires_grad or params.requires_grad:
        raise ValueError(grad_msg)
    (_, N, B), dev = _lead_blocks(obs, "obs", n_sets), obs.device
    adt, atail = (torch.int32, (N,)) if A == 5 else (torch.float64, (N, 2) if A == 2 else (N,))
    need = (("action", action, adt, atail, bool(P)), ("reward", reward, torch.float64, (N,), bool(R)), ("kind", kind, torch.uint8, (N,), True))
    for name, t, dtype, tail, used in need:
        if t is None and (B == 1 or not used):
            continue
        if not (torch.is_tensor(t) and t.dtype == dtype and t.dim() == 1 + len(tail) and tuple(t.shape[1:]) == tail and t.shape[0] >= B - 1
                and t.device == dev and t.is_contiguous()):
            raise ValueError("%s must be a contiguous %s tensor of at least B - 1 = %d blocks %s on obs's device" % (name, dtype, B - 1, list(tail)))
    if state is not None and not _is(state, torch.float32, (N, S), dev):
        raise ValueError("state must be a contiguous float32 [N, S] = [%d, %d] tensor on obs's device" % (N, S))
    if reward0 is not None and not _is(reward0, torch.float64, (N,), dev):
        raise ValueError("reward0 must be a contiguous float64 [N] = [%d] tensor on obs's device" % N)
    return widths, cell, flags, count, n_sets, B, N, dev


def _structs(widths, cell, flags, count, n_sets, params, obs, action, reward, kind, state, reward0):
    """``(abi.Rnn, abi.RnnSequence)`` of checked arguments; the outputs of ``ftl_rnn_forward`` are left NULL."""
    A, W0 = widths[-1], widths[0]
    P, R, U, S = abi.rnn_widths(widths, cell, flags)
    B, N = int(obs.shape[0]), int(obs.shape[1])
    net = _rnn_struct(widths, cell, flags, params, n_sets, N // n_sets, state)
    seq = abi.RnnSequence()
    seq.obs, seq.obs_block_bytes = obs.data_ptr(), N * W0 * 4
    if B > 1:
        if P:
            seq.action, seq.action_block_bytes = action.data_ptr(), N * (16 if A == 2 else 8 if A == 1 else 4)
        if R:
            seq.reward, seq.reward_block_bytes = reward.data_ptr(), N * 8
        seq.kind, seq.kind_block_bytes = kind.data_ptr(), N
    seq.reward0 = reward0.data_ptr() if reward0 is not None else None
    return net, seq


def forward(widths, cell, params, obs, action=None, reward=None, kind=None, state=None, reward0=None, prev_action=True, prev_reward=True,
            out=None, h_out=None, state_out=None, state_at=0):
    """The raw heads of ``n_sets`` recurrent nets (``widths`` = input width, trunk layers, head width; ``cell`` LSTM units) on a recorded
    sequence, in ONE launch (``ftl_rnn_forward``): block b is evaluated operation for operation as ``ftl_rnn_act`` evaluates a decision,
    the state is carried from block to block inside the kernel, and the row block b + 1 reads is all zeros where ``kind[b]`` is
    ``FTL_TR_VOID`` -- what ``collect_rnn`` did when it recorded the sequence.

    ``params`` float32 ``[n_sets, param_count]`` (``RecurrentPolicy.params``); ``obs`` float32 ``[B, N, widths[0]]``; ``n_sets`` must
    divide N and row r uses set ``r // (N // n_sets)``.  ``action`` (float64 ``[>= B-1, N, 2]`` for head 2, float64 ``[>= B-1, N]`` for head
    1, int32 ``[>= B-1, N]`` for head 5), ``reward`` float64 ``[>= B-1, N]`` and ``kind`` uint8 ``[>= B-1, N]`` are the records between
    the blocks: a ``Trajectory``'s T-block tensors are accepted as they are for B = T (``obs[:-1]``) or B = T + 1 (``obs``).  ``action``
    is needed only with ``prev_action``, ``reward`` only with ``prev_reward``, and none of the three for B = 1.  ``state`` float32
    ``[N, S]`` is the state before block 0 (None: zeros, every row at the start of an episode; it is never written), ``reward0`` float64
    ``[N]`` the reward the first decision saw (None: zeros).

    Returns float32 ``[B, N, A]`` (``out=`` reuses such a buffer).  ``h_out`` float32 ``[B, N, cell]`` receives the cell's output of every
    block, ``state_out`` float32 ``[N, S]`` the rows block ``state_at`` read (``0 <= state_at < B``): the ``state`` of a call that continues
    there.  Outputs must not overlap inputs.  The launch goes to the current stream of ``obs``'s device.  ``ValueError`` for every shape,
    dtype, device or contiguity mismatch, ``NotImplementedError`` beyond the limits of ``ftl_rnn`` or beyond 65,535 blocks, both before any
    library call.  ``backward`` is its derivative with respect to ``params``, and ``Net`` puts the
    two under autograd."""
    widths, cell, flags, count, n_sets, B, N, dev = _check_sequence(widths, cell, params, obs, action, reward, kind, state, reward0, prev_action,
                                                                     prev_reward, "forward() has no backward pass: pass detached tensors")
    A, S = widths[-1], abi.rnn_widths(widths, cell, flags)[3]
    if out is not None and not _is(out, torch.float32, (B, N, A), dev):
        raise ValueError("out must be a contiguous float32 %s tensor on obs's device" % ([B, N, A],))
    if h_out is not None and not _is(h_out, torch.float32, (B, N, cell), dev):
        raise ValueError("h_out must be a contiguous float32 %s tensor on obs's device" % ([B, N, cell],))
    if state_out is not None:
        if not _is(state_out, torch.float32, (N, S), dev):
            raise ValueError("state_out must be a contiguous float32 [N, S] = [%d, %d] tensor on obs's device" % (N, S))
        if not 0 <= int(state_at) < B:
            raise ValueError("state_at must name a block, 0 <= state_at < %d, not %r" % (B, state_at))
    if not obs.is_cuda or params.device != dev:
        raise ValueError("obs and params must lie on the same GPU device")
    if out is None:
        out = torch.empty(B, N, A, dtype=torch.float32, device=dev)
    if state is None:
        state = torch.zeros(N, S, dtype=torch.float32, device=dev)
    net, seq = _structs(widths, cell, flags, count, n_sets, params, obs, action, reward, kind, state, reward0)
    seq.head, seq.head_block_bytes = out.data_ptr(), N * A * 4
    if h_out is not None:
        seq.h, seq.h_block_bytes = h_out.data_ptr(), N * cell * 4
    if state_out is not None:
        seq.state_out, seq.state_at = state_out.data_ptr(), int(state_at)
    lib = _lib.load()
    h = _device_handle(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.ftl_rnn_forward(h, C.byref(net), B, N, C.byref(seq), stream), lib)
    return out


class RecurrentCritic(_RnnParams):
    """A value net with memory for ``gae()``, or a population of ``n_sets`` of them: an ``ftl_rnn`` of head width 1 -- trunk, LSTM cell,
    linear value head, the value branch on the cell's output as in the reference's ``*_lstm`` models -- evaluated on a trajectory by
    ``forward`` in one launch.  ``RecurrentCritic(widths, cell, n_sets=1, prev_reward=True, params=None, device=None)``: ``widths[-1]``
    must be 1; ``params`` is the float32 ``[n_sets, param_count]`` tensor of all weights (zeros on ``device``, the current GPU by
    default, unless given), with the views ``layer(l)``, ``cell_weights()``, ``head_weights()`` and ``load_lstm_cell`` of the policy.

    The parameter layout of ``ftl_rnn`` ties the width of ``a_prev`` to the head width, here 1.  The critic can therefore be fed the last
    action (``prev_action=True``) only where an action is one float64 -- the turn of a ``constant_follower_speed`` config --; ``values``
    refuses any other action record with ``ValueError``.  The default feeds the last reward only."""

    def __init__(self, widths, cell, n_sets=1, prev_reward=True, params=None, device=None, prev_action=False):
        self.params = self._hold(widths, cell, n_sets, prev_action, prev_reward, params, device, "critic", head=1)
        self.device = self.params.device

    def values(self, traj, state=None, reward0=None, out=None):
        """``(values, carry)``: float32 ``[T + 1, N]``, the value of every ``traj.obs[t]`` with the memory of the blocks before it -- what
        ``gae(traj, values, ...)`` takes --, and float32 ``[N, S]``, the rows block T read: the ``state`` for the next trajectory's
        ``values`` (with ``reward0 = traj.reward[-1]``), so that the critic's memory runs on through consecutive ``collect`` calls.
        ``state`` None: zeros, every env at the start of an episode; ``reward0`` float64 ``[N]``: the reward the first decision saw
        (``batch.reward`` before the ``collect`` call).  ``out=(values, carry)`` reuses a pair.  With ``prev_action`` the trajectory's
        actions must be the float64 ``[T, N]`` of a ``constant_follower_speed`` config (``ValueError`` otherwise)."""
        if not isinstance(traj, Trajectory) or not torch.is_tensor(traj.obs) or traj.obs.dim() != 3:
            raise ValueError("traj must be a Trajectory with obs [T + 1, N, %d]" % self.widths[0])
        T1, N = int(traj.obs.shape[0]), int(traj.obs.shape[1])
        if self.prev_action and not (torch.is_tensor(traj.action) and traj.action.dtype == torch.float64 and traj.action.dim() == 2):
            raise ValueError("prev_action needs actions of one float64 each (a constant_follower_speed config): the critic's a_prev is as "
                             "wide as its head, 1")
        values = carry = None
        if out is not None:
            values, carry = out
            if not (torch.is_tensor(values) and values.dtype == torch.float32 and tuple(values.shape) == (T1, N) and values.is_contiguous()):
                raise ValueError("out's values must be a contiguous float32 [T + 1, N] tensor")
            values = values.unsqueeze(-1)
        if carry is None:
            if not traj.obs.is_cuda:
                raise ValueError("traj must lie on a GPU device")
            carry = torch.empty(N, self.S, dtype=torch.float32, device=traj.obs.device)
        v = forward(self.widths, self.cell, self.params, traj.obs, traj.action if self.prev_action else None, traj.reward, traj.kind, state,
                    reward0, self.prev_action, self.prev_reward, out=values, state_out=carry, state_at=T1 - 1)
        return v[..., 0], carry


def backward(widths, cell, params, obs, dhead, action=None, reward=None, kind=None, state=None, reward0=None, prev_action=True,
             prev_reward=True, out=None, dstate_in=None, dstate_out=None):
    """``d loss / d params`` of the nets ``forward`` evaluates, by back-propagation through time over the B blocks in one call on the
    current stream (``ftl_rnn_backward``: a kernel that keeps the carry of a tile inside one workgroup, and a small reduction).  Every
    argument of ``forward`` means what it means there; ``dhead`` is the gradient of a scalar loss with respect to the raw head of every
    row, a detached contiguous float32 ``[B, N, A]`` tensor on ``obs``'s device, zeros on the rows to leave out (``~traj.valid``).
    Returns float32 ``[n_sets, param_count]`` in the layout of ``params`` -- overwritten, not accumulated; ``out=`` reuses such a buffer.

    ``dstate_in`` float32 ``[N, 2 * cell]`` is ``d loss / d (h', c')`` of the last block, from a later piece of the sequence (None:
    zeros); ``dstate_out`` float32 ``[N, 2 * cell]`` receives ``d loss / d (h, c)`` of the rows block 0 read: the ``dstate_in`` of the
    piece before, once the caller has zeroed the rows whose ``kind`` at the seam is VOID.

    The arithmetic is fixed operation by operation (include/ftl.h; tests/rnn_backward_numpy.py is the twin): the forward values are
    ``forward``'s bits, the zero rule cuts the carry where ``forward`` cut the state, and the sums over rows run in a fixed order --
    float32 chains inside spans of ``abi.FTL_RNN_BWD_SPAN`` (tile, block) pairs, float64 across.  The workspace (span partials, ``h'`` and
    ``c'`` of every block) is a tensor cached per device and stream.  There is no gradient with respect to observations, actions or
    rewards.  ``ValueError`` / ``NotImplementedError`` as ``forward``, before any library call."""
    widths, cell, flags, count, n_sets, B, N, dev = _check_sequence(widths, cell, params, obs, action, reward, kind, state, reward0, prev_action,
                                                                     prev_reward, "backward() takes detached tensors: there is no gradient "
                                                                     "with respect to obs, and params' gradient is what it returns")
    A, S = widths[-1], abi.rnn_widths(widths, cell, flags)[3]
    if abi.rnn_backward_lds_bytes(widths, cell, flags) > abi.FTL_RNN_BWD_MAX_LDS:
        raise NotImplementedError("backward() keeps a tile's activations in the 160 KiB of LDS of a workgroup: this net needs %d bytes "
                                  "(narrower trunk layers or fewer of them)" % abi.rnn_backward_lds_bytes(widths, cell, flags))
    if not (_is(dhead, torch.float32, (B, N, A), dev) and not dhead.requires_grad):
        raise ValueError("dhead must be a detached contiguous float32 %s tensor on obs's device" % ([B, N, A],))
    if out is not None and not (_is(out, torch.float32, (n_sets, count), dev) and not out.requires_grad):
        raise ValueError("out must be a contiguous float32 [%d, %d] tensor on obs's device" % (n_sets, count))
    for name, t in (("dstate_in", dstate_in), ("dstate_out", dstate_out)):
        if t is not None and not (_is(t, torch.float32, (N, 2 * cell), dev) and not t.requires_grad):
            raise ValueError("%s must be a contiguous float32 [N, 2 * cell] = [%d, %d] tensor on obs's device" % (name, N, 2 * cell))
    if not obs.is_cuda or params.device != dev:
        raise ValueError("obs and params must lie on the same GPU device")
    if out is None:
        out = torch.empty(n_sets, count, dtype=torch.float32, device=dev)
    if state is None:
        state = torch.zeros(N, S, dtype=torch.float32, device=dev)
    net, seq = _structs(widths, cell, flags, count, n_sets, params, obs, action, reward, kind, state, reward0)
    lib = _lib.load()
    h = _device_handle(dev)
    need = lib.ftl_sizeof_rnn_backward_workspace(C.byref(net), B, N)
    if need < 0:
        raise _lib.FtlError("ftl_sizeof_rnn_backward_workspace refused a net that the package's checks passed")
    ws, raw = _workspace("rnn_backward", dev, need)
    g = abi.RnnGradient()
    g.dhead, g.dhead_block_bytes, g.grad = dhead.data_ptr(), N * A * 4, out.data_ptr()
    g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    g.dstate_in = dstate_in.data_ptr() if dstate_in is not None else None
    g.dstate_out = dstate_out.data_ptr() if dstate_out is not None else None
    _lib.check(lib.ftl_rnn_backward(h, C.byref(net), B, N, C.byref(seq), C.byref(g), C.c_void_p(raw)), lib)
    return out


class _NetFunction(torch.autograd.Function):
    """``forward`` with ``backward`` as its derivative with respect to ``params``."""

    @staticmethod
    def forward(ctx, params, net, obs, action, reward, kind, state, reward0):
        ctx.save_for_backward(params)
        ctx.net, ctx.seq = net, (obs, action, reward, kind, state, reward0)
        return forward(net.widths, net.cell, params.detach(), obs, action, reward, kind, state, reward0, net.prev_action, net.prev_reward)

    @staticmethod
    def backward(ctx, dhead):
        (params,), net = ctx.saved_tensors, ctx.net
        obs, action, reward, kind, state, reward0 = ctx.seq
        grad = backward(net.widths, net.cell, params.detach(), obs, dhead.detach().contiguous(), action, reward, kind, state, reward0,
                        net.prev_action, net.prev_reward)
        return (grad,) + (None,) * 7


class Net(_RnnParams, torch.nn.Module):
    """A trainable recurrent net on the device, or a population of ``n_sets`` of them: ``Net(widths, cell, n_sets=1, prev_action=True,
    prev_reward=True, params=None, device=None)`` is an ``nn.Module`` whose one ``nn.Parameter`` ``params`` is the float32 ``[n_sets,
    param_count]`` tensor of all weights in the layout of ``ftl_rnn`` (zeros on ``device``, the current GPU by default, unless given).
    ``params=policy.params`` (a ``RecurrentPolicy``) or ``params=critic.params`` (a ``RecurrentCritic``) shares storage: an optimizer step on
    ``net.params`` is what the policy plays next, with no copy.

    ``net(traj, state=None, reward0=None)`` is ``forward`` under autograd on a ``Trajectory`` of ``collect_rnn`` -- ``traj.obs[:-1]`` with
    ``traj.action`` / ``reward`` / ``kind`` from ``traj.state[0]`` unless ``state`` is given --, float32 ``[T, N, A]``; a tuple ``(obs, action,
    reward, kind)`` of ``forward``'s tensors is taken as it is (``state`` None: zeros).  Its derivative is ``backward``: ``loss.backward()``
    leaves ``d loss / d params`` in ``net.params.grad``, accumulated like any parameter's, with the pinned arithmetic of include/ftl.h.
    ``layer``, ``cell_weights``, ``head_weights`` and ``load_lstm_cell`` are the views of the policy."""

    def __init__(self, widths, cell, n_sets=1, prev_action=True, prev_reward=True, params=None, device=None):
        torch.nn.Module.__init__(self)
        params = self._hold(widths, cell, n_sets, prev_action, prev_reward, params, device, "net")
        self.params = torch.nn.Parameter(params.detach())       # (the parameter shares the tensor's storage)

    def forward(self, seq, state=None, reward0=None):
        if isinstance(seq, Trajectory):
            if not torch.is_tensor(getattr(seq, "state", None)) or not torch.is_tensor(seq.obs) or seq.obs.dim() != 3 or seq.obs.shape[0] < 2:
                raise ValueError("a Trajectory must come from collect_rnn: obs [T + 1, N, H * W] and its state blocks")
            obs, action, reward, kind = seq.obs[:-1], seq.action, seq.reward, seq.kind
            if state is None:
                state = seq.state[0]
        elif isinstance(seq, (tuple, list)) and len(seq) == 4:
            obs, action, reward, kind = seq
        else:
            raise ValueError("net() takes a Trajectory of collect_rnn or a tuple (obs, action, reward, kind)")
        if any(torch.is_tensor(t) and t.requires_grad for t in (obs, action, reward, kind, state, reward0)):
            raise ValueError("the sequence must not require grad: there is no gradient with respect to the record")
        return _NetFunction.apply(self.params, self, obs, action if self.prev_action else None, reward if self.prev_reward else None, kind,
                                  state, reward0)
