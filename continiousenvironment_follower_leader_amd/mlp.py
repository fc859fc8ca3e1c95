"""A dense feed-forward policy on the device, or a population of them: ``MlpPolicy`` reads the batch's ``policy_obs`` and writes the action
of every env (``ftl_mlp_act``), and closes the loop over T steps with one call (``batch.rollout_mlp``, ``ftl_rollout_mlp``).  With
``n_sets`` weight sets, consecutive equal blocks of envs use consecutive sets: a 65,536-env batch scores 1,024 population members on 64
envs each in one rollout, which is all a gradient-free method (evolution strategies, the reference's neuroevolution) needs.  The
arithmetic is fixed operation by operation (the ``ftl_mlp_act`` block of ``include/ftl.h``): ReLU hidden layers, a linear head mapped to
the config's action space."""
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


class MlpPolicy:
    """``n_sets`` feed-forward nets of shape ``widths`` (input width first, head width last) on ``batch`` (a ``VecGame`` or a
    ``PipelinedVecGame`` built with ``policy_obs=True``); env e uses set ``e // (batch.n // n_sets)``.

    ``params`` is the float32 ``[n_sets, param_count]`` device tensor of all weights (zeros unless given; the caller writes into it, so an
    ES update is one torch op); ``layer(l)`` gives views of one layer's weights and biases.  ``act()`` decides for every env from the
    ``policy_obs`` the batch's last reset / step / scan wrote and returns the persistent action tensor in the config's encoding: float64
    ``[N, 2]``, float64 ``[N]`` under ``constant_follower_speed``, int32 ``[N]`` under ``discrete_action_space`` -- what ``batch.step``
    takes.  The policy is callable with an observation it ignores, so ``batch.evaluate(policy, scen_ids)`` scores it per scenario.

    On a pipelined batch every part works on its rows on its own stream: like ``step``, ``act()`` does not join."""

    def __init__(self, batch, widths, params=None, n_sets=1):
        self.widths = widths = check_widths(batch.cfg, widths)
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
        self.param_count = abi.mlp_param_count(widths)
        if params is None:
            params = torch.zeros(n_sets, self.param_count, dtype=torch.float32, device=self.device)
        if (not torch.is_tensor(params) or params.dtype != torch.float32 or tuple(params.shape) != (n_sets, self.param_count)
                or params.device != self.device or not params.is_contiguous()):
            raise ValueError("params must be a contiguous float32 [n_sets, %d] tensor on the batch's device" % self.param_count)
        self.params = params
        self.lib = _lib.load()
        if self.lib.ftl_mlp_param_count((C.c_int32 * len(widths))(*widths), len(widths) - 1) != self.param_count:
            raise _lib.FtlError("ftl_mlp_param_count disagrees with abi.mlp_param_count: library and package do not match")
        shape = (self.n, 2) if self.encoding == abi.FTL_ACTION_BOX2 else (self.n,)
        self.action = torch.zeros(*shape, dtype=torch.int32 if self.encoding == abi.FTL_ACTION_DISCRETE else torch.float64, device=self.device)
        self.row = self.action.element_size() * (2 if self.encoding == abi.FTL_ACTION_BOX2 else 1)     # bytes of one env's action
        games = getattr(batch, "games", None)
        # (game, first env, its ftl_mlp) of every handle under the batch
        self._parts = [(g, lo, self._net(lo)) for g, lo in ([(batch, 0)] if games is None else [(g, sh.lo) for g, sh in zip(games, batch.shards)])]

    def _net(self, env_first):
        net = abi.Mlp()
        net.params, net.set_stride, net.n_sets, net.n_layers = self.params.data_ptr(), self.param_count, self.n_sets, len(self.widths) - 1
        for l, w in enumerate(self.widths):
            net.width[l] = w
        net.env_first, net.envs_per_set = env_first, self.envs_per_set
        return net

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
        """``batch.rollout_mlp(self, ...)``."""
        b, T = self.batch, int(T)
        b._need_pool()
        if T < 1:
            raise ValueError("a rollout needs T >= 1")
        actions = torch.empty(T, *self.action.shape, dtype=self.action.dtype, device=self.device) if record else None
        b._prepare_rollout_outputs()
        ap = actions.data_ptr() if record else 0
        for (g, lo, net), s in zip(self._parts, self._streams(actions)):
            _lib.check(self.lib.ftl_rollout_mlp(g.h, T, float(gamma), g._out_ref, C.byref(g._rollout_outputs()), C.byref(net),
                                                (ap + lo * self.row) if record else None, self.n * self.row if record else 0, 0, s), self.lib)
        out = (b.rollout_ret, b.rollout_steps, b.rollout_status)
        return out + (actions,) if record else out

    def fitness(self):
        """f64[n_sets]: the mean of the last rollout's returns over every set's envs (joins a pipelined batch)."""
        self.batch._wait_parts()
        return self.batch.rollout_ret.view(self.n_sets, -1).mean(1)
