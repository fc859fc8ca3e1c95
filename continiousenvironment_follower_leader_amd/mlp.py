"""A dense feed-forward policy on the device, or a population of them: ``MlpPolicy`` reads the batch's ``policy_obs`` and writes the action
of every env (``ftl_mlp_act``), and closes the loop over T steps with one call (``batch.rollout_mlp``, ``ftl_rollout_mlp``).  With
``n_sets`` weight sets, consecutive equal blocks of envs use consecutive sets: a 65,536-env batch scores 1,024 population members on 64
envs each in one rollout, which is all a gradient-free method (evolution strategies, the reference's neuroevolution) needs.  The
arithmetic is fixed operation by operation (the ``ftl_mlp_act`` block of ``include/ftl.h``): ReLU or tanh hidden layers
(``activation``), a linear head mapped to the config's action space.  ``params_from_torch`` / ``torch_module`` move a net between a
``torch.nn.Sequential`` and a row of ``params``.

For a gradient method (the reference trains with PPO) ``sample()`` adds the caller's noise to the head, ``collect()`` /
``batch.collect_mlp`` play T such decisions through episode boundaries with one call and leave a ``Trajectory`` on the device
(``ftl_collect_mlp``), and ``gae()`` turns its rewards and kinds and a critic's values into advantages (``ftl_gae``).  ``forward()`` evaluates a net on
recorded rows with the same arithmetic (``ftl_mlp_forward``): ``Critic`` is a head-1 net whose ``values(traj.obs)`` feed ``gae()``, and
``policy.forward(traj.obs[:-1])`` replays ``traj.head`` bit for bit.  ``backward()`` is its derivative with respect to the weights
(``ftl_mlp_backward``), per set and in a fixed summation order, and ``Net`` ties the two together under torch autograd: an ``nn.Module``
whose one parameter can share storage with ``policy.params`` or ``critic.params``, so one optimizer trains what the device plays.  The
recurrent net has the same pair in ``rnn.py`` (``rnn.backward``, ``rnn.Net``).  Between the two, ``ppo_loss()`` is the PPO loss head of
the Box policies on the device (``ftl_ppo_head``; ``ppo_head()`` is its raw form): from the new heads, the trajectory, the advantages
and the critic's values to the head, value and ``log_std`` gradients, per weight set, for either net family."""
import ctypes as C

import torch

from . import _lib, abi


def head_encoding(cfg):
    """(FTL_ACTION_* encoding, head width) of the action space ``cfg`` declares, as ``VecGame._encode_action`` reads it."""
    if cfg.discrete_action_space and cfg.constant_follower_speed:
        raise ValueError("discrete_action_space with constant_follower_speed ignores the action (ENV:922-925): nothing for a policy to decide")
    if cfg.discrete_action_space:
        return abi.FTL_ACTION_DISCRETE, 5
    if cfg.constant_follower_speed:
        return abi.FTL_ACTION_TURN, 1
    return abi.FTL_ACTION_BOX2, 2


def check_widths(cfg, widths):
    """``widths`` as a tuple of ints, checked against the limits of ``ftl_mlp`` and the action space of ``cfg`` (no device needed)."""
    widths = tuple(int(w) for w in widths)
    if len(widths) < 2:
        raise ValueError("widths must name the input width and at least one layer")
    if len(widths) - 1 > abi.FTL_MLP_MAX_LAYERS:
        raise NotImplementedError("at most %d layers" % abi.FTL_MLP_MAX_LAYERS)
    if min(widths) < 1:
        raise ValueError("every width must be at least 1")
    if widths[0] > abi.FTL_MLP_MAX_IN or max(widths[1:]) > abi.FTL_MLP_MAX_WIDTH:
        raise NotImplementedError("widths beyond %d inputs / %d neurons a layer" % (abi.FTL_MLP_MAX_IN, abi.FTL_MLP_MAX_WIDTH))
    enc, head = head_encoding(cfg)
    if widths[-1] != head:
        raise ValueError("the head of this config's action space is %d wide, not %d" % (head, widths[-1]))
    return widths


ACTIVATIONS = {"relu": abi.FTL_MLP_ACT_RELU, "tanh": abi.FTL_MLP_ACT_TANH}


def check_activation(activation):
    """``activation`` if it names a hidden activation of ``ftl_mlp`` (``"relu"`` or ``"tanh"``), else ``ValueError``."""
    if not isinstance(activation, str) or activation not in ACTIVATIONS:
        raise ValueError('activation must be "relu" or "tanh", not %r' % (activation,))
    return activation


def params_from_torch(module):
    """``(widths, activation, params_row)`` of a ``torch.nn.Sequential`` that alternates ``nn.Linear`` with ``nn.ReLU`` or ``nn.Tanh`` and
    ends in a linear layer: ``params_row`` is a new float32 tensor ``[param_count]`` on the module's device (a CPU module needs no GPU) in
    the layout of ``ftl_mlp`` -- layer by layer ``W_l`` as ``weight.T`` (``[in][out]``) then ``b_l`` -- ready for
    ``policy.params[s].copy_(row)``.  A net without hidden layers
    reports ``"relu"``.  ``ValueError`` for mixed activations or anything else in the sequence (a Linear without bias included)."""
    nn = torch.nn
    if not isinstance(module, nn.Sequential) or len(module) % 2 == 0:
        raise ValueError("params_from_torch reads an nn.Sequential of Linear, activation, Linear, ..., Linear")
    widths, kinds, parts = [], set(), []
    for i, m in enumerate(module):
        if i % 2:
            if type(m) not in (nn.ReLU, nn.Tanh):
                raise ValueError("module %d: nn.ReLU or nn.Tanh expected between two linear layers, not %s" % (i, type(m).__name__))
            kinds.add("relu" if type(m) is nn.ReLU else "tanh")
            continue
        if type(m) is not nn.Linear or m.bias is None:
            raise ValueError("module %d: nn.Linear with a bias expected, not %s" % (i, type(m).__name__))
        if widths and widths[-1] != m.in_features:
            raise ValueError("module %d: %d inputs after a layer of %d" % (i, m.in_features, widths[-1]))
        widths += [m.in_features, m.out_features] if not widths else [m.out_features]
        parts += [m.weight.detach().t().reshape(-1), m.bias.detach().reshape(-1)]
    if len(kinds) > 1:
        raise ValueError("mixed activations: ftl_mlp has one activation for all hidden layers")
    row = torch.cat([p.to(torch.float32) for p in parts]).contiguous()
    return tuple(widths), (kinds.pop() if kinds else "relu"), row


def torch_module(widths, activation, params_row=None):
    """The inverse of ``params_from_torch``: an ``nn.Sequential`` of float32 ``nn.Linear`` layers of ``widths`` with ``nn.ReLU`` or
    ``nn.Tanh`` between them, on the CPU; with ``params_row`` (float32 ``[param_count]``, any device) its weights and biases are copies
    of that row, otherwise torch's own initialisation."""
    widths = tuple(int(w) for w in widths)
    if len(widths) < 2 or min(widths) < 1:
        raise ValueError("widths must name the input width and at least one layer, each at least 1")
    act = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh}[check_activation(activation)]
    mods = []
    for l, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        mods += ([act()] if l else []) + [torch.nn.Linear(a, b)]
    module = torch.nn.Sequential(*mods)
    if params_row is not None:
        count = abi.mlp_param_count(widths)
        if not torch.is_tensor(params_row) or params_row.dtype != torch.float32 or tuple(params_row.shape) != (count,):
            raise ValueError("params_row must be a float32 [%d] tensor" % count)
        row, off = params_row.detach(), 0
        with torch.no_grad():
            for lin in module[::2]:
                a, b = lin.in_features, lin.out_features
                lin.weight.copy_(row[off:off + a * b].view(a, b).t())
                lin.bias.copy_(row[off + a * b:off + (a + 1) * b])
                off += (a + 1) * b
    return module


class Trajectory:
    """What ``MlpPolicy.collect`` leaves on the device for T steps of N envs (the blocks of ``ftl_collect_buffers``):
    ``obs`` float32 ``[T+1, N, H*W]`` -- ``obs[t]`` decided step t, ``obs[t+1]`` is its true successor (the terminal observation where the
    episode ended), ``obs[T]`` what the last step wrote; ``head`` float32 ``[T, N, A]`` the raw head; ``action`` ``[T, N(, 2)]`` what was
    played, in the config's encoding; ``reward`` float64 ``[T, N]``; ``kind`` uint8 ``[T, N]`` of ``abi.FTL_TR_*``; ``noise`` / ``sigma`` the
    caller's tensors (or None).  On a pipelined batch the rows of part k are valid on ``stream(k)``: ``join()`` before reading."""

    def __init__(self, obs, head, action, reward, kind, noise=None, sigma=None):
        self.obs, self.head, self.action, self.reward, self.kind, self.noise, self.sigma = obs, head, action, reward, kind, noise, sigma

    @property
    def valid(self):
        """bool ``[T, N]``: a transition to learn from (not the restart step of next-step reset, not a step after the episode's end)."""
        return self.kind != abi.FTL_TR_VOID

    @property
    def terminated(self):
        """bool ``[T, N]``: the step ended the episode with a status other than the time limit (no bootstrap)."""
        return self.kind == abi.FTL_TR_TERMINATED

    @property
    def truncated(self):
        """bool ``[T, N]``: the step ended the episode at the time limit (the bootstrap continues from ``obs[t+1]``)."""
        return self.kind == abi.FTL_TR_TRUNCATED


_GAE_HANDLES = {}


def _device_handle(device):
    """A one-env handle of the default config on ``device``, kept for the process: ``ftl_gae`` reads nothing of a handle but its device."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in _GAE_HANDLES:
        from .config import make_config
        lib, h = _lib.load(), C.c_void_p()
        _lib.check(lib.ftl_create(C.byref(make_config().c), 1, index, C.byref(h)), lib)
        _GAE_HANDLES[index] = h
    return _GAE_HANDLES[index]


def gae(traj, values, gamma, lam, out=None):
    """Generalised advantage estimates and value targets of a trajectory in one launch (``ftl_gae``): ``traj`` is a ``Trajectory`` or a
    ``(reward f64 [T, N], kind u8 [T, N])`` pair, ``values`` the critic on ``obs[0 .. T]`` as float32 ``[T+1, N]`` (detached; a trailing
    axis of 1 is accepted).  Returns ``(adv, ret)`` float32 ``[T, N]`` -- ``out=(adv, ret)`` reuses a pair.  VOID rows get 0 and cut the
    carry, a terminated step does not bootstrap, a truncated one bootstraps from the terminal observation's value.  Float64 inside, one
    rounding per operation (include/ftl.h)."""
    reward, kind = (traj.reward, traj.kind) if isinstance(traj, Trajectory) else traj
    if not (torch.is_tensor(reward) and reward.dtype == torch.float64 and reward.dim() == 2 and reward.is_cuda and reward.is_contiguous()):
        raise ValueError("reward must be a contiguous float64 [T, N] device tensor")
    T, N = reward.shape
    if not (torch.is_tensor(kind) and kind.dtype == torch.uint8 and tuple(kind.shape) == (T, N) and kind.device == reward.device and kind.is_contiguous()):
        raise ValueError("kind must be a contiguous uint8 [T, N] tensor on reward's device")
    if T < 1 or N < 1:
        raise ValueError("gae() needs T >= 1 and N >= 1")
    if torch.is_tensor(values) and values.dim() == 3 and values.shape[2] == 1:
        values = values[:, :, 0]
    if not torch.is_tensor(values) or values.requires_grad:
        raise ValueError("values must be a detached tensor")
    values = values.contiguous()
    if values.dtype != torch.float32 or tuple(values.shape) != (T + 1, N) or values.device != reward.device:
        raise ValueError("values must be a float32 [T + 1, N] = [%d, %d] tensor on reward's device" % (T + 1, N))
    if out is None:
        out = (torch.empty(T, N, dtype=torch.float32, device=reward.device), torch.empty(T, N, dtype=torch.float32, device=reward.device))
    adv, ret = out
    for name, t in (("adv", adv), ("ret", ret)):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == (T, N) and t.device == reward.device and t.is_contiguous()):
            raise ValueError("out's %s must be a contiguous float32 [T, N] tensor on reward's device" % name)
    lib = _lib.load()
    h = _device_handle(reward.device)
    stream = C.c_void_p(torch.cuda.current_stream(reward.device).cuda_stream)
    _lib.check(lib.ftl_gae(h, T, N, reward.data_ptr(), N * 8, kind.data_ptr(), N, values.data_ptr(), float(gamma), float(lam),
                           adv.data_ptr(), ret.data_ptr(), stream), lib)
    return adv, ret


def check_net_widths(widths):
    """``widths`` as a tuple of ints inside the limits of ``ftl_mlp`` alone (no config: any head width up to ``FTL_MLP_MAX_WIDTH``), what
    ``forward`` evaluates: ``ValueError`` for a malformed list, ``NotImplementedError`` beyond the limits."""
    widths = tuple(int(w) for w in widths)
    if len(widths) < 2:
        raise ValueError("widths must name the input width and at least one layer")
    if len(widths) - 1 > abi.FTL_MLP_MAX_LAYERS:
        raise NotImplementedError("at most %d layers" % abi.FTL_MLP_MAX_LAYERS)
    if min(widths) < 1:
        raise ValueError("every width must be at least 1")
    if widths[0] > abi.FTL_MLP_MAX_IN or max(widths[1:]) > abi.FTL_MLP_MAX_WIDTH:
        raise NotImplementedError("widths beyond %d inputs / %d neurons a layer" % (abi.FTL_MLP_MAX_IN, abi.FTL_MLP_MAX_WIDTH))
    return widths


FORWARD_MAX_BLOCKS = 65535                 # include/ftl.h, ftl_mlp_forward: n_blocks


def _check_params(params, count, n_sets=None, on=None, where=""):
    """The one rule for every ``params`` of the package: a contiguous float32 ``[n_sets, count]`` tensor -- of ``n_sets`` rows when given, of
    at least one otherwise, whose device satisfies the predicate ``on`` (asked last) when given; ``where`` ends the message.  Returns
    ``params``."""
    ok = torch.is_tensor(params) and params.dtype == torch.float32 and params.dim() == 2 and params.shape[1] == count and params.is_contiguous()
    ok = ok and (params.shape[0] >= 1 if n_sets is None else params.shape[0] == n_sets)
    if not (ok and (on is None or on(params.device))):
        raise ValueError("params must be a contiguous float32 [n_sets, %d] tensor%s" % (count, where))
    return params


def _held_params(params, n_sets, count, device, who):
    """The ``params`` of a holder (``Critic``, ``Net`` and the recurrent pair; ``who`` names it in the message): checked, or zeros on
    ``device`` -- the current GPU by default -- when None."""
    if n_sets < 1:
        raise ValueError("n_sets must be at least 1")
    if params is None:
        params = torch.zeros(n_sets, count, dtype=torch.float32, device=torch.device("cuda" if device is None else device))
    return _check_params(params, count, n_sets, None if device is None else lambda d: d == torch.device(device), " on the %s's device" % who)


def _lead_blocks(t, name, n_sets=None):
    """``(lead, N, blocks)`` of a tensor ``[..., N, W]`` whose leading axes are flattened to blocks.  With ``n_sets``, the limits of a net's
    launch as well: ``n_sets`` divides N, at most ``FORWARD_MAX_BLOCKS`` blocks."""
    lead, N = tuple(t.shape[:-2]), int(t.shape[-2])
    blocks = 1
    for d in lead:
        blocks *= int(d)
    if N < 1 or blocks < 1:
        raise ValueError("%s must hold at least one block of at least one row, not %s" % (name, list(t.shape)))
    if n_sets is not None and N % n_sets:
        raise ValueError("n_sets = %d must divide the %d rows of a block" % (n_sets, N))
    if n_sets is not None and blocks > FORWARD_MAX_BLOCKS:
        raise NotImplementedError("at most %d blocks in one call, not %d" % (FORWARD_MAX_BLOCKS, blocks))
    return lead, N, blocks


_WORKSPACE = {}                            # (purpose, device index, raw stream) -> the tensor


def _workspace(purpose, device, need, dtype=torch.float32):
    """``(tensor, raw stream)``: a ``dtype`` tensor of at least ``need`` bytes for the current stream of ``device``, kept per purpose
    (``"mlp_backward"``, ``"rnn_backward"``, ``"ppo_head"``), device and stream, and grown when a call needs more."""
    raw = torch.cuda.current_stream(device).cuda_stream
    key = (purpose, device.index if device.index is not None else torch.cuda.current_device(), raw)
    size = torch.finfo(dtype).bits // 8
    ws = _WORKSPACE.get(key)
    if ws is None or ws.numel() * size < need:
        ws = _WORKSPACE[key] = torch.empty((need + size - 1) // size, dtype=dtype, device=device)
    return ws, raw


def _mlp_struct(widths, params, n_sets, envs_per_set, activation, env_first=0):
    """The ``abi.Mlp`` of checked arguments: rows from ``env_first`` on, ``envs_per_set`` of them to a weight set."""
    net = abi.Mlp()
    net.params, net.set_stride, net.n_sets, net.n_layers = params.data_ptr(), abi.mlp_param_count(widths), n_sets, len(widths) - 1
    for l, w in enumerate(widths):
        net.width[l] = w
    net.env_first, net.envs_per_set, net.activation = env_first, envs_per_set, ACTIVATIONS[activation]
    return net


def _check_rows(widths, params, x, activation, grad_msg, params_too, max_in=None):
    """The checks ``forward`` and ``backward`` share, in ``forward``'s order; returns ``(widths, count, n_sets, lead, N, blocks)``.
    ``max_in`` is ``backward``'s limit on the input width; ``grad_msg`` refuses an ``x`` (``params_too``: or ``params``) that requires grad."""
    widths = check_net_widths(widths)
    check_activation(activation)
    count = abi.mlp_param_count(widths)
    if max_in is not None and widths[0] > max_in:
        raise NotImplementedError("at most %d inputs in backward()" % max_in)
    n_sets = int(_check_params(params, count).shape[0])
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() >= 2 and x.shape[-1] == widths[0] and x.is_contiguous()):
        raise ValueError("x must be a contiguous float32 [..., N, %d] tensor" % widths[0])
    if x.requires_grad or (params_too and params.requires_grad):
        raise ValueError(grad_msg)
    return (widths, count, n_sets) + _lead_blocks(x, "x", n_sets)


def forward(widths, params, x, activation="relu", out=None):
    """The raw heads of ``n_sets`` nets of shape ``widths`` on caller-supplied rows, in one launch (``ftl_mlp_forward``): the forward pass
    of ``ftl_mlp_act`` operation for operation -- the k-ordered ``fmaf`` chains, ReLU or ``tanh32`` hidden layers, a linear head -- without
    an action map.  ``params`` is the float32 ``[n_sets, param_count]`` device tensor of ``MlpPolicy.params``; ``x`` a contiguous float32
    device tensor ``[..., N, widths[0]]`` whose leading axes are flattened to blocks (a trajectory's ``obs`` ``[T+1, N, W0]`` as it is);
    ``n_sets`` must divide N, and row r of every block uses set ``r // (N // n_sets)``.  Returns float32 ``[..., N, widths[-1]]``;
    ``out=`` reuses such a buffer, which must not overlap ``x``.  The launch goes to the current stream of ``x``'s device.

    On the ``obs`` a ``collect()`` recorded, with the net that played, the result equals the recorded ``head`` bit for bit; with a net of
    head width 1 it is a critic's values (``Critic``).  No hidden activation of the rows is materialised: they stay in the kernel's LDS.
    ``ValueError`` for every shape, dtype, device or contiguity mismatch, ``NotImplementedError`` beyond the limits of ``ftl_mlp`` or
    beyond 65,535 blocks, both before any library call.

    Measured on 33 x 65,536 rows of 180-64-64-1 against the same values from torch under ``no_grad``: with 1,024 sets
    2.42 ms (ReLU) / 2.00 ms (tanh) against 3.84 / 3.88 ms for per-block ``baddbmm`` -- the project's timing bar holds --; with ONE set
    2.23 / 1.80 ms against 1.47 / 1.48 ms for torch's single large ``addmm`` chain -- the bar does NOT hold: there torch is faster and
    this call buys the pinned arithmetic and 1.66 GB less peak memory, not time."""
    widths, count, n_sets, lead, N, blocks = _check_rows(widths, params, x, activation, "forward() has no backward pass: pass detached tensors",
                                                         True)
    shape = lead + (N, widths[-1])
    if out is not None and not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()
                                and out.device == x.device):
        raise ValueError("out must be a contiguous float32 %s tensor on x's device" % (list(shape),))
    if not x.is_cuda or params.device != x.device:
        raise ValueError("x and params must lie on the same GPU device")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    net = _mlp_struct(widths, params, n_sets, N // n_sets, activation)
    lib = _lib.load()
    h = _device_handle(x.device)
    stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(lib.ftl_mlp_forward(h, C.byref(net), blocks, N, x.data_ptr(), N * widths[0] * 4, out.data_ptr(), N * widths[-1] * 4, stream), lib)
    return out


class _Holder:
    """What ``Critic`` and ``Net`` share: the checked ``widths``, ``activation``, ``n_sets`` and ``param_count``, the checked or new
    ``params`` tensor (``_hold`` returns it: the critic keeps the tensor, the net wraps it), and ``load`` / ``module``.  ``_WHO`` and
    ``_THIS`` name the class in the messages."""
    _WHO, _THIS = "net", "this one"

    def _hold(self, widths, n_sets, activation, params, device, head=None):
        self.widths = check_net_widths(widths)
        if head is not None and self.widths[-1] != head:
            raise ValueError("a critic's head is %d wide, not %d" % (head, self.widths[-1]))
        self.activation = check_activation(activation)
        self.n_sets, self.param_count = int(n_sets), abi.mlp_param_count(self.widths)
        return _held_params(params, self.n_sets, self.param_count, device, self._WHO)

    def load(self, module, s=None):
        """Copy the weights of a torch module (``params_from_torch``: an ``nn.Sequential`` of this net's widths and activation) into set
        ``s``, or into every set (``s=None``).  Returns ``self``."""
        widths, activation, row = params_from_torch(module)
        if widths != self.widths or (len(widths) > 2 and activation != self.activation):
            raise ValueError("the module is a %s %s net, %s a %s %s one" % (activation, widths, self._THIS, self.activation, self.widths))
        if s is not None and not 0 <= int(s) < self.n_sets:
            raise IndexError("set %d of %d" % (int(s), self.n_sets))
        (self.params if s is None else self.params[int(s)]).copy_(row)
        return self

    def module(self, s=0):
        """A new ``torch.nn.Sequential`` on the CPU with the weights of set ``s`` (``torch_module``)."""
        if not 0 <= int(s) < self.n_sets:
            raise IndexError("set %d of %d" % (int(s), self.n_sets))
        return torch_module(self.widths, self.activation, self.params.detach()[int(s)])


class Critic(_Holder):
    """A value net for ``gae()``, or a population of ``n_sets`` of them: an ``ftl_mlp`` of head width 1 evaluated by ``forward``.
    ``Critic(widths, n_sets=1, activation="tanh", params=None, device=None)``: ``widths[-1]`` must be 1 (``ValueError``); ``params`` is the
    float32 ``[n_sets, param_count]`` tensor of all weights (zeros on ``device``, the current GPU by default, unless given).  The critic
    is trained as a torch module by autograd; ``load(module)`` copies its weights here once per iteration and ``values(traj.obs)`` then
    gives ``gae()`` its values in one launch, with the device's pinned arithmetic and without materialising a hidden activation."""

    _WHO, _THIS = "critic", "the critic"

    def __init__(self, widths, n_sets=1, activation="tanh", params=None, device=None):
        self.params = self._hold(widths, n_sets, activation, params, device, head=1)
        self.device = self.params.device

    def values(self, obs, out=None):
        """float32 ``[..., N]``: the value of every row of ``obs`` ``[..., N, widths[0]]`` (``forward``; ``n_sets`` must divide N, row r
        uses set ``r // (N // n_sets)``).  ``out=`` reuses a contiguous float32 ``[..., N]`` buffer."""
        if out is not None:
            if not (torch.is_tensor(out) and out.is_contiguous() and torch.is_tensor(obs) and tuple(out.shape) == tuple(obs.shape[:-1])):
                raise ValueError("out must be a contiguous float32 [..., N] tensor of obs's leading shape")
            out = out.unsqueeze(-1)
        return forward(self.widths, self.params, obs, self.activation, out)[..., 0]


def backward(widths, params, x, dy, activation="relu", out=None):
    """``d loss / d params`` of ``n_sets`` nets of shape ``widths`` on the rows ``forward`` evaluates, in one call on the current stream
    (``ftl_mlp_backward``: a kernel that recomputes the hidden layers per tile and a small reduction): ``params`` and ``x`` are
    ``forward``'s; ``dy`` is the gradient of a scalar loss with respect to the raw head of every row, a contiguous float32
    ``[..., N, widths[-1]]`` tensor of ``x``'s leading shape on its device, zeros on the rows to leave out (``~traj.valid``).  Returns
    float32 ``[n_sets, param_count]`` in the layout of ``params`` -- overwritten, not accumulated; ``out=`` reuses such a buffer.

    The arithmetic is fixed operation by operation (include/ftl.h; tests/mlp_backward_numpy.py is the twin): the forward values are
    ``forward``'s bits, the sums over rows run in a fixed order -- spans of ``abi.FTL_MLP_BWD_SPAN`` tiles, float32 chains inside, float64
    across -- so the result does not depend on the machine or the launch, and no hidden activation reaches global memory.  The span
    partials go through a workspace tensor cached per device and stream.  There is no gradient with respect to ``x``.
    ``ValueError`` / ``NotImplementedError`` as ``forward``, before any library call."""
    widths, count, n_sets, lead, N, blocks = _check_rows(widths, params, x, activation, "backward() has no gradient with respect to x: pass a "
                                                         "detached tensor", False, abi.FTL_MLP_BWD_MAX_IN)
    shape = lead + (N, widths[-1])
    if not (torch.is_tensor(dy) and dy.dtype == torch.float32 and tuple(dy.shape) == shape and dy.is_contiguous() and dy.device == x.device
            and not dy.requires_grad):
        raise ValueError("dy must be a detached contiguous float32 %s tensor on x's device" % (list(shape),))
    if out is not None and not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (n_sets, count)
                                and out.is_contiguous() and out.device == x.device and not out.requires_grad):
        raise ValueError("out must be a contiguous float32 [%d, %d] tensor on x's device" % (n_sets, count))
    if not x.is_cuda or params.device != x.device:
        raise ValueError("x and params must lie on the same GPU device")
    if out is None:
        out = torch.empty(n_sets, count, dtype=torch.float32, device=x.device)
    net = _mlp_struct(widths, params.detach(), n_sets, N // n_sets, activation)
    lib = _lib.load()
    h = _device_handle(x.device)
    need = lib.ftl_sizeof_mlp_backward_workspace(C.byref(net), blocks, N)
    if need < 0:
        raise _lib.FtlError("ftl_sizeof_mlp_backward_workspace refused a net that the package's checks passed")
    ws, raw = _workspace("mlp_backward", x.device, need)
    _lib.check(lib.ftl_mlp_backward(h, C.byref(net), blocks, N, x.data_ptr(), N * widths[0] * 4, dy.data_ptr(), N * widths[-1] * 4,
                                    out.data_ptr(), ws.data_ptr(), ws.numel() * 4, C.c_void_p(raw)), lib)
    return out


class _NetFunction(torch.autograd.Function):
    """``forward`` with ``backward`` as its derivative with respect to ``params``."""

    @staticmethod
    def forward(ctx, params, x, widths, activation):
        ctx.save_for_backward(params, x)
        ctx.widths, ctx.activation = widths, activation
        return forward(widths, params.detach(), x, activation)

    @staticmethod
    def backward(ctx, dy):
        params, x = ctx.saved_tensors
        return backward(ctx.widths, params.detach(), x, dy.detach().contiguous(), ctx.activation), None, None, None


class Net(_Holder, torch.nn.Module):
    """A trainable net on the device, or a population of ``n_sets`` of them: ``Net(widths, n_sets=1, activation="relu", params=None,
    device=None)`` is an ``nn.Module`` whose one ``nn.Parameter`` ``params`` is the float32 ``[n_sets, param_count]`` tensor of all weights
    in the layout of ``ftl_mlp`` (zeros on ``device``, the current GPU by default, unless given).  ``params=policy.params`` or
    ``params=critic.params`` shares storage: an optimizer step on ``net.params`` is what the policy plays next, with no copy.

    ``net(x)`` is ``forward`` on ``x`` float32 ``[..., N, widths[0]]`` (``n_sets`` must divide N; ``x`` must not require grad) under
    autograd: its derivative is ``backward``, so ``loss.backward()`` leaves ``d loss / d params`` in ``net.params.grad`` with the pinned
    arithmetic of include/ftl.h, for one net as for 1,024, without a hidden activation in global memory.  ``load`` / ``module`` move
    weights to and from a ``torch.nn.Sequential`` as on ``Critic``."""

    def __init__(self, widths, n_sets=1, activation="relu", params=None, device=None):
        torch.nn.Module.__init__(self)
        self.params = torch.nn.Parameter(self._hold(widths, n_sets, activation, params, device).detach())       # (it shares the tensor's storage)

    def forward(self, x):
        if torch.is_tensor(x) and x.requires_grad:
            raise ValueError("x must not require grad: there is no gradient with respect to the rows")
        return _NetFunction.apply(self.params, x, self.widths, self.activation)

    def load(self, module, s=None):
        """``Critic.load`` under ``no_grad``: ``params`` is a parameter here."""
        with torch.no_grad():
            return _Holder.load(self, module, s)


class PpoHead:
    """What ``ppo_head`` returns: ``dhead`` float32 ``[..., N, A]``, ``dvalue`` float32 ``[..., N]`` (None without a value part), ``dlog_std``
    float32 ``[n_sets, A]`` and ``stats`` float64 ``[n_sets, abi.FTL_PPO_STATS]`` -- count, advantage mean and std, policy loss, value loss,
    approximate KL, clip fraction, total loss, per weight set."""

    def __init__(self, dhead, dvalue, dlog_std, stats):
        self.dhead, self.dvalue, self.dlog_std, self.stats = dhead, dvalue, dlog_std, stats


def ppo_head(head, head_old, noise, sigma_old, sigma, adv, ret, kind, value=None, log_sigma_shift=None, clip=0.2, vf_coef=0.5,
             normalize=True, out=None):
    """The PPO loss head of a Box policy in one call on the current stream (``ftl_ppo_head``, four launches, no host synchronisation): from
    the new ``head`` float32 ``[..., N, A]`` (A = 2 or 1; ``Net`` or ``rnn.Net`` on the recorded rows), the record's ``head_old`` and
    ``noise`` of that shape, ``sigma_old`` / ``sigma`` float32 ``[n_sets, A]`` (``n_sets`` must divide N; row r of a block uses set
    ``r // (N // n_sets)``), ``adv`` / ``ret`` float32 and ``kind`` uint8 ``[..., N]`` and, optionally, the critic's ``value`` float32
    ``[..., N]``, to a ``PpoHead``: the gradients of

        sum over sets of  mean over the set's valid rows of  -min(r a, clip(r, 1 - clip, 1 + clip) a) + vf_coef * 0.5 (value - ret)^2

    with respect to every head, every value and ``log_std`` (``log_sigma_shift`` is ``log_std_new - log_std_old`` ``[n_sets, A]``, zeros
    when None), and the statistics table.  ``normalize`` standardises the advantages per set over its valid rows.  Rows whose kind is
    ``FTL_TR_VOID`` get zero gradients and count nowhere.  The arithmetic is fixed operation by operation and the sums run in a fixed
    order (include/ftl.h; tests/ppo_numpy.py is the twin), so ``dhead`` -- the ``dy`` of ``backward`` -- does not depend on the machine
    or the launch.  ``out=`` reuses a ``PpoHead``.  All tensors are detached, contiguous and on one GPU: every mismatch is a ``ValueError``
    before any library call, a head width other than 1 or 2 a ``NotImplementedError``."""
    if not (torch.is_tensor(head) and head.dtype == torch.float32 and head.dim() >= 2 and head.is_contiguous()):
        raise ValueError("head must be a contiguous float32 [..., N, A] tensor")
    A = int(head.shape[-1])
    if A not in (1, 2):
        raise NotImplementedError("ppo_head() takes the Box heads, 2 or 1 wide, not %d (Discrete(5) needs a pinned logarithm)" % A)
    lead, N, blocks = _lead_blocks(head, "head")
    dev = head.device

    def check(name, t, shape, dtype=torch.float32):
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == dev
                and not t.requires_grad):
            raise ValueError("%s must be a detached contiguous %s %s tensor on head's device" % (name, dtype, list(shape)))

    if head.requires_grad:
        raise ValueError("head must be detached: ppo_head() returns the gradients, ppo_loss() is the autograd form")
    check("head_old", head_old, head.shape)
    check("noise", noise, head.shape)
    if not (torch.is_tensor(sigma) and sigma.dim() == 2 and sigma.shape[0] >= 1):
        raise ValueError("sigma must be a float32 [n_sets, %d] tensor" % A)
    n_sets = int(sigma.shape[0])
    check("sigma", sigma, (n_sets, A))
    check("sigma_old", sigma_old, (n_sets, A))
    if log_sigma_shift is not None:
        check("log_sigma_shift", log_sigma_shift, (n_sets, A))
    if N % n_sets:
        raise ValueError("n_sets = %d must divide the %d rows of a block" % (n_sets, N))
    check("adv", adv, lead + (N,))
    check("ret", ret, lead + (N,))
    check("kind", kind, lead + (N,), torch.uint8)
    if value is not None:
        check("value", value, lead + (N,))
    clip, vf_coef = float(clip), float(vf_coef)
    if not 0.0 <= clip < float("inf"):
        raise ValueError("clip must be a finite number of at least 0, not %r" % (clip,))
    if out is not None:
        if not isinstance(out, PpoHead):
            raise ValueError("out must be a PpoHead")
        check("out.dhead", out.dhead, head.shape)
        check("out.dlog_std", out.dlog_std, (n_sets, A))
        check("out.stats", out.stats, (n_sets, abi.FTL_PPO_STATS), torch.float64)
        if value is not None:
            check("out.dvalue", out.dvalue, lead + (N,))
        elif out.dvalue is not None:
            raise ValueError("out.dvalue must be None without value")
    if not head.is_cuda:
        raise ValueError("head must lie on a GPU device")
    if out is None:
        out = PpoHead(torch.empty_like(head), torch.empty_like(value) if value is not None else None,
                      torch.empty(n_sets, A, dtype=torch.float32, device=dev), torch.empty(n_sets, abi.FTL_PPO_STATS, dtype=torch.float64, device=dev))
    lib = _lib.load()
    h = _device_handle(dev)
    need = lib.ftl_sizeof_ppo_head_workspace(blocks, N, n_sets)
    if need < 0:
        raise NotImplementedError("ftl_ppo_head: more than 2^31 - 1 segments in one call; split the blocks")
    ws, raw = _workspace("ppo_head", dev, need, torch.float64)
    a = abi.PpoHeadArgs()
    a.n_blocks, a.n, a.n_sets, a.width = blocks, N, n_sets, A
    a.head_new, a.head_old, a.noise = head.data_ptr(), head_old.data_ptr(), noise.data_ptr()
    a.head_new_block_bytes = a.head_old_block_bytes = a.noise_block_bytes = a.dhead_block_bytes = N * A * 4
    a.sigma_old, a.sigma_new = sigma_old.data_ptr(), sigma.data_ptr()
    a.log_sigma_shift = log_sigma_shift.data_ptr() if log_sigma_shift is not None else None
    a.adv, a.ret, a.kind = adv.data_ptr(), ret.data_ptr(), kind.data_ptr()
    a.adv_block_bytes = a.ret_block_bytes = a.value_new_block_bytes = a.dvalue_block_bytes = N * 4
    a.kind_block_bytes = N
    a.value_new = value.data_ptr() if value is not None else None
    a.clip_lo, a.clip_hi, a.vf_coef, a.normalize = 1.0 - clip, 1.0 + clip, vf_coef, 1 if normalize else 0
    a.dhead, a.dvalue = out.dhead.data_ptr(), out.dvalue.data_ptr() if value is not None else None
    a.dlog_std, a.stats = out.dlog_std.data_ptr(), out.stats.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    _lib.check(lib.ftl_ppo_head(h, C.byref(a), C.c_void_p(raw)), lib)
    return out


class _PpoLossFunction(torch.autograd.Function):
    """The scalar loss of ``ppo_head`` with its ``dhead``, ``dvalue`` and ``dlog_std`` as the derivative."""

    @staticmethod
    def forward(ctx, head, value, log_std, head_old, noise, sigma_old, log_std_old, adv, ret, kind, clip, vf_coef, normalize):
        ls = log_std.detach()
        r = ppo_head(head.detach().contiguous(), head_old, noise, sigma_old, ls.exp(), adv, ret, kind,
                     value.detach().contiguous() if value is not None else None, (ls - log_std_old).contiguous(), clip, vf_coef, normalize)
        ctx.save_for_backward(r.dhead, r.dlog_std, *(() if r.dvalue is None else (r.dvalue,)))
        ctx.mark_non_differentiable(r.stats)
        return r.stats[:, 7].sum().to(torch.float32), r.stats

    @staticmethod
    def backward(ctx, gloss, gstats):
        dhead, dlog_std, *dvalue = ctx.saved_tensors
        return (dhead * gloss, dvalue[0] * gloss if dvalue else None, dlog_std * gloss) + (None,) * 10


def ppo_loss(traj, head, log_std, adv, ret, value=None, log_std_old=None, clip=0.2, vf_coef=0.5, normalize=True):
    """The PPO loss of a recorded trajectory under autograd, on the device (``ppo_head``): ``traj`` is the ``Trajectory`` of ``collect()``
    or of the recurrent ``collect_rnn`` (its ``head``, ``noise``, ``sigma`` and ``kind`` are read), ``head`` the new heads ``[T, N, A]``
    of ``Net`` or ``rnn.Net`` on its rows, ``log_std`` the float32 ``[n_sets, A]`` parameter, ``adv`` / ``ret`` those of ``gae()``,
    ``value`` the critic's new values ``[T, N]`` or ``[T, N, 1]`` (None: no value part).  ``log_std_old`` defaults to
    ``traj.sigma.log()``.  Returns the scalar loss -- the sum over the weight sets of each set's mean over its valid rows, a float32
    tensor with the float64 table ``.stats`` ``[n_sets, 8]`` attached --, and ``loss.backward()`` hands ``dhead``, ``dvalue`` and
    ``dlog_std`` to autograd: ``opt.zero_grad(); mlp.ppo_loss(...).backward(); opt.step()`` is a PPO epoch for one net as for a
    population, with no boolean-mask indexing, no host synchronisation and a ``dy`` that is pinned bit for bit.  The entropy bonus is
    not included: with a state-independent sigma it is ``log_std.sum()`` plus a constant; add it in torch."""
    for name in ("head", "noise", "sigma", "kind"):
        if not torch.is_tensor(getattr(traj, name, None)):
            raise ValueError("traj.%s is missing: ppo_loss() reads head, noise, sigma and kind of a stochastic trajectory" % name)
    if not (torch.is_tensor(head) and head.dim() >= 2 and tuple(head.shape) == tuple(traj.head.shape)):
        raise ValueError("head must have the shape of traj.head, %s" % (list(traj.head.shape),))
    if not (torch.is_tensor(log_std) and log_std.dtype == torch.float32 and tuple(log_std.shape) == tuple(traj.sigma.shape)):
        raise ValueError("log_std must be a float32 %s tensor, the shape of traj.sigma" % (list(traj.sigma.shape),))
    if value is not None:
        if torch.is_tensor(value) and value.dim() == head.dim() and value.shape[-1] == 1:
            value = value[..., 0]
        if not (torch.is_tensor(value) and tuple(value.shape) == tuple(head.shape[:-1])):
            raise ValueError("value must be a [..., N] or [..., N, 1] tensor of head's leading shape")
    if log_std_old is None:
        log_std_old = traj.sigma.log()
    if not (torch.is_tensor(log_std_old) and tuple(log_std_old.shape) == tuple(log_std.shape) and not log_std_old.requires_grad):
        raise ValueError("log_std_old must be a detached tensor of log_std's shape")
    loss, stats = _PpoLossFunction.apply(head, value, log_std, traj.head, traj.noise, traj.sigma.detach(), log_std_old, adv, ret, traj.kind,
                                         clip, vf_coef, normalize)
    loss.stats = stats
    return loss


class MlpPolicy:
    """``n_sets`` feed-forward nets of shape ``widths`` (input width first, head width last) on ``batch`` (a ``VecGame`` or a
    ``PipelinedVecGame`` built with ``policy_obs=True``); env e uses set ``e // (batch.n // n_sets)``.

    ``MlpPolicy(batch, widths, params=None, n_sets=1, activation="relu")``.  ``activation`` is the hidden layers' function, ``"relu"`` or
    ``"tanh"`` (``ftl_mlp.activation``: tanh is the fixed float32 sequence ``tanh32`` of include/ftl.h), kept as ``policy.activation``;
    any other value is a ``ValueError``.  The head is linear either way.

    ``params`` is the float32 ``[n_sets, param_count]`` device tensor of all weights (zeros unless given; the caller writes into it, so an
    ES update is one torch op); ``layer(l)`` gives views of one layer's weights and biases.  ``act()`` decides for every env from the
    ``policy_obs`` the batch's last reset / step / scan wrote and returns the persistent action tensor in the config's encoding: float64
    ``[N, 2]``, float64 ``[N]`` under ``constant_follower_speed``, int32 ``[N]`` under ``discrete_action_space`` -- what ``batch.step``
    takes.  The policy is callable with an observation it ignores, so ``batch.evaluate(policy, scen_ids)`` scores it per scenario.

    On a pipelined batch every part works on its rows on its own stream: like ``step``, ``act()`` does not join."""

    _ROLLOUT, _COLLECT = "ftl_rollout_mlp", "ftl_collect_mlp"                          # the library functions of this net family
    _COUNT_MISMATCH = "ftl_mlp_param_count disagrees with abi.mlp_param_count: library and package do not match"

    def __init__(self, batch, widths, params=None, n_sets=1, activation="relu"):
        self.activation = check_activation(activation)
        self.widths = check_widths(batch.cfg, widths)
        self.param_count = abi.mlp_param_count(self.widths)
        self._bind(batch, n_sets, params)

    def _bind(self, batch, n_sets, params):
        """What a policy of either family does with its batch once ``widths`` and ``param_count`` stand: the checks against the batch, the
        checked or new ``params``, the library, the persistent action tensor and ``_parts``, the built struct of every part."""
        widths = self.widths
        self.encoding, _ = head_encoding(batch.cfg)
        pol = getattr(batch, "policy_obs", None)
        if pol is None:
            raise ValueError("the policy reads policy_obs: build the batch with policy_obs=True on a config that has a sensor for it")
        if widths[0] != pol.shape[1] * pol.shape[2]:
            raise ValueError("widths[0] must be H * W = %d of policy_obs, not %d" % (pol.shape[1] * pol.shape[2], widths[0]))
        n_sets = int(n_sets)
        if n_sets < 1 or batch.n % n_sets:
            raise ValueError("n_sets must divide the batch's %d envs" % batch.n)
        self.batch, self.n, self.device, self.n_sets, self.envs_per_set = batch, batch.n, batch.device, n_sets, batch.n // n_sets
        if params is None:
            params = torch.zeros(n_sets, self.param_count, dtype=torch.float32, device=self.device)
        self.params = _check_params(params, self.param_count, n_sets, lambda d: d == self.device, " on the batch's device")
        self._buffers()
        self.lib = _lib.load()
        if self._lib_param_count() != self.param_count:
            raise _lib.FtlError(self._COUNT_MISMATCH)
        shape = (self.n, 2) if self.encoding == abi.FTL_ACTION_BOX2 else (self.n,)
        self.action = torch.zeros(*shape, dtype=torch.int32 if self.encoding == abi.FTL_ACTION_DISCRETE else torch.float64, device=self.device)
        self.row = self.action.element_size() * (2 if self.encoding == abi.FTL_ACTION_BOX2 else 1)     # bytes of one env's action
        games = getattr(batch, "games", None)
        # (game, first env, its net struct) of every handle under the batch
        self._parts = [(g, lo, self._net(lo)) for g, lo in ([(batch, 0)] if games is None else [(g, sh.lo) for g, sh in zip(games, batch.shards)])]

    def _buffers(self):
        """The persistent tensors a net family keeps beside ``params`` (``head`` and ``obs`` here arrive with the first ``sample()``)."""

    def _lib_param_count(self):
        return self.lib.ftl_mlp_param_count((C.c_int32 * len(self.widths))(*self.widths), len(self.widths) - 1)

    def _net(self, env_first):
        return _mlp_struct(self.widths, self.params, self.n_sets, self.envs_per_set, self.activation, env_first)

    def layer(self, l):
        """Views ``(W [n_sets, in, out], b [n_sets, out])`` of layer ``l`` (0-based) in ``params``: ``W[s].copy_(linear.weight.T)``
        loads a ``torch.nn.Linear``."""
        w = self.widths
        if not 0 <= l < len(w) - 1:
            raise IndexError("layer %d of %d" % (l, len(w) - 1))
        off = abi.mlp_param_count(w[:l + 1])
        nw = w[l] * w[l + 1]
        return self.params[:, off:off + nw].view(self.n_sets, w[l], w[l + 1]), self.params[:, off + nw:off + nw + w[l + 1]]

    def _streams(self, tensor=None):
        b = self.batch
        return b._part_streams(tensor) if hasattr(b, "_part_streams") else [b._stream()]

    def act(self):
        """The forward pass of every env (``ftl_mlp_act``, one launch per part); returns ``action``."""
        self.batch._need_pool()
        ap = self.action.data_ptr()
        for (g, lo, net), s in zip(self._parts, self._streams()):
            _lib.check(self.lib.ftl_mlp_act(g.h, g._out_ref, C.byref(net), ap + lo * self.row, s), self.lib)
        return self.action

    def __call__(self, obs=None):
        return self.act()

    def rollout(self, T, gamma=1.0, record=False):
        """``batch.rollout_mlp(self, ...)`` (``batch.rollout_rnn`` for a recurrent policy)."""
        b, T = self.batch, int(T)
        b._need_pool()
        if T < 1:
            raise ValueError("a rollout needs T >= 1")
        actions = torch.empty(T, *self.action.shape, dtype=self.action.dtype, device=self.device) if record else None
        b._prepare_rollout_outputs()
        ap = actions.data_ptr() if record else 0
        rollout = getattr(self.lib, self._ROLLOUT)
        for (g, lo, net), s in zip(self._parts, self._streams(actions)):
            _lib.check(rollout(g.h, T, float(gamma), g._out_ref, C.byref(g._rollout_outputs()), C.byref(net),
                               (ap + lo * self.row) if record else None, self.n * self.row if record else 0, 0, s), self.lib)
        out = (b.rollout_ret, b.rollout_steps, b.rollout_status)
        return out + (actions,) if record else out

    # ------------------------------------------------------------------ stochastic decisions and recorded trajectories (ftl_mlp_sample, ftl_collect_mlp)
    def _check_noise(self, noise, sigma, lead=()):
        """``noise`` (float32 ``lead + [N, A]``) and ``sigma`` (float32 ``[n_sets, A]``) of a sampling call, checked; either may be None."""
        A = self.widths[-1]
        for name, t, shape in (("noise", noise, tuple(lead) + (self.n, A)), ("sigma", sigma, (self.n_sets, A))):
            if t is None:
                continue
            if (not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != self.device
                    or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 %s tensor on the batch's device" % (name, list(shape)))
        if noise is not None and sigma is None and self.encoding != abi.FTL_ACTION_DISCRETE:
            raise ValueError("a Box head with noise needs sigma (z = y + sigma * noise)")

    def sample(self, noise=None, sigma=None):
        """One stochastic decision of every env (``ftl_mlp_sample``, one launch per part), beside ``act()``: ``noise`` float32 ``[N, A]``
        (A the head width) is added to the head before its map -- scaled by ``sigma`` float32 ``[n_sets, A]`` on the Box heads, as a
        Gumbel draw on Discrete(5) -- and the raw head and the observation rows the kernel read are kept in ``self.head`` ``[N, A]`` and
        ``self.obs`` ``[N, H * W]``.  ``noise=None`` is ``act()`` bit for bit.  Returns ``action``."""
        self.batch._need_pool()
        self._check_noise(noise, sigma)
        if not hasattr(self, "head"):
            self.head = torch.zeros(self.n, self.widths[-1], dtype=torch.float32, device=self.device)
            self.obs = torch.zeros(self.n, self.widths[0], dtype=torch.float32, device=self.device)
        A, W0 = self.widths[-1], self.widths[0]
        ap, hp, op = self.action.data_ptr(), self.head.data_ptr(), self.obs.data_ptr()
        for (g, lo, net), s in zip(self._parts, self._streams(noise)):
            _lib.check(self.lib.ftl_mlp_sample(g.h, g._out_ref, C.byref(net), (noise.data_ptr() + lo * A * 4) if noise is not None else None,
                                               sigma.data_ptr() if sigma is not None else None, hp + lo * A * 4, op + lo * W0 * 4,
                                               ap + lo * self.row, s), self.lib)
        self._keep = (noise, sigma)
        return self.action

    def collect(self, T, noise=None, sigma=None, auto_reset="next_step", out=None):
        """``batch.collect_mlp(self, ...)``."""
        return self._collect(T, noise, sigma, auto_reset, out)

    def _state_blocks(self, T, record_state):
        """``{name: (shape, dtype)}`` of what a trajectory of this net family holds beside the feed-forward record."""
        return {}

    def _collect_struct(self, out, lo):
        """``(the struct the library takes, its ftl_collect_buffers)`` for the part whose first env is ``lo``, with the family's own blocks set."""
        cb = abi.CollectBuffers()
        return cb, cb

    def _collect(self, T, noise, sigma, auto_reset, out, record_state=False):
        """The one ``collect`` of both net families: ``_state_blocks`` and ``_collect_struct`` add a recurrent policy's state blocks."""
        b, T = self.batch, int(T)
        b._need_pool()
        if T < 1:
            raise ValueError("a trajectory needs T >= 1")
        if auto_reset is not False and auto_reset != "next_step":
            raise ValueError('collect() takes auto_reset=False or "next_step": the other modes put the next episode\'s first observation where '
                             'the terminal one belongs (got %r)' % (auto_reset,))
        self._check_noise(noise, sigma, lead=(T,))
        A, W0, N = self.widths[-1], self.widths[0], self.n
        extra = self._state_blocks(T, record_state)
        want = dict(obs=((T + 1, N, W0), torch.float32), head=((T, N, A), torch.float32), action=((T,) + tuple(self.action.shape), self.action.dtype),
                    reward=((T, N), torch.float64), kind=((T, N), torch.uint8), **extra)
        if out is None:
            new = {k: torch.empty(*shape, dtype=dtype, device=self.device) for k, (shape, dtype) in want.items()}
            out = Trajectory(**{k: t for k, t in new.items() if k not in extra})
            for k in extra:
                setattr(out, k, new[k])
        else:
            for name, (shape, dtype) in want.items():
                t = getattr(out, name, None)
                if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous()):
                    raise ValueError("out.%s must be a contiguous %s %s tensor on the batch's device" % (name, dtype, list(shape)))
        out.noise, out.sigma = noise, sigma
        flags = abi.FTL_STEP_NEXT_RESET if auto_reset == "next_step" else 0
        collect = getattr(self.lib, self._COLLECT)
        for (g, lo, net), s in zip(self._parts, self._streams(noise)):
            bufs, cb = self._collect_struct(out, lo)
            cb.obs, cb.head, cb.action = out.obs.data_ptr() + lo * W0 * 4, out.head.data_ptr() + lo * A * 4, out.action.data_ptr() + lo * self.row
            cb.reward, cb.kind = out.reward.data_ptr() + lo * 8, out.kind.data_ptr() + lo
            cb.noise = (noise.data_ptr() + lo * A * 4) if noise is not None else None
            cb.sigma = sigma.data_ptr() if sigma is not None else None
            cb.obs_step_bytes, cb.head_step_bytes, cb.action_step_bytes = N * W0 * 4, N * A * 4, N * self.row
            cb.reward_step_bytes, cb.kind_step_bytes, cb.noise_step_bytes = N * 8, N, N * A * 4
            _lib.check(collect(g.h, T, g._out_ref, C.byref(net), C.byref(bufs), flags, s), self.lib)
        self._keep = out                                            # (the parts' streams write into it: it outlives the call)
        return out

    def forward(self, x, out=None):
        """The raw heads of the policy's own net -- its sets and its activation -- on recorded rows ``x`` float32 ``[..., N, H * W]`` (N the
        batch's envs: ``traj.obs``, or any stack of observation blocks), as float32 ``[..., N, A]`` in one launch (the module's
        ``forward``); ``policy.forward(traj.obs[:-1])`` is ``traj.head`` bit for bit.  The launch goes to the current stream, not to the
        parts' streams: on a pipelined batch ``join()`` first, as before reading a ``Trajectory``."""
        if not torch.is_tensor(x) or x.dim() < 2 or x.shape[-2] != self.n:
            raise ValueError("x must be a [..., N, H * W] tensor with the batch's N = %d rows a block" % self.n)
        return forward(self.widths, self.params, x, self.activation, out)

    def fitness(self):
        """f64[n_sets]: the mean of the last rollout's returns over every set's envs (joins a pipelined batch)."""
        self.batch._wait_parts()
        return self.batch.rollout_ret.view(self.n_sets, -1).mean(1)
