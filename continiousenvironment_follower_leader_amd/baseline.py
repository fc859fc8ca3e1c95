"""The reference's baseline controller on the device: ``run_2d.py --mode base`` (lines 109-151) -- ``utils/misc.py:move_to_the_point``
along a FIFO of the leader's target points -- as a policy (``BaselineFollower.act``) and as closed-loop rollouts with one call
(``batch.rollout_baseline``).  The contract is the ``ftl_baseline_act`` block of ``include/ftl.h``."""
import ctypes as C

import torch

from . import _lib, abi


class BaselineFollower:
    """The way-point FIFO of every env of ``batch`` (a ``VecGame`` or a ``PipelinedVecGame``) and the controller that reads it.

    ``state`` is the uint8 ``[N, 16 + 16 * cap]`` device tensor of ``ftl_baseline_act``: row e = int32 ``{head, count, pending, flags}``
    and ``cap`` float64 points used as a ring.  Rows are self-contained: ``state[j] = state[i]`` moves a follower, so a caller that
    snapshots / clones / restores envs copies these rows along with them.  A zeroed row is a fresh follower, and an env whose step count is 0
    (any reset, any auto-reset discipline) starts afresh by itself -- there is nothing to call at a reset.

    ``act()`` decides for every env from what the batch's last reset / step wrote (``obs_num``, ``target``) and returns the persistent
    float64 ``[N, 2]`` action tensor; it first books the step just taken, so call it exactly once per step.  The follower is callable with
    an observation it ignores: ``batch.evaluate(follower, scen_ids, sensors=False)`` scores the baseline per scenario.

    On a pipelined batch every part works on its rows of the one buffer on its own stream: like ``step``, ``act()`` does not join."""

    def __init__(self, batch, cap=64):
        if batch.cfg.discrete_action_space or batch.cfg.constant_follower_speed:
            raise ValueError("the baseline follower feeds Box(2) actions: not for a config with discrete_action_space or constant_follower_speed")
        cap = int(cap)
        if cap < 2:
            raise ValueError("cap must be at least 2")
        self.batch, self.cap, self.n, self.device = batch, cap, batch.n, batch.device
        self.row = abi.baseline_row_bytes(cap)
        self.lib = _lib.load()
        self.state = torch.zeros(self.n, self.row, dtype=torch.uint8, device=self.device)
        self.action = torch.zeros(self.n, 2, dtype=torch.float64, device=self.device)
        games = getattr(batch, "games", None)
        # (game, first env, envs) of every handle under the batch
        self._parts = [(batch, 0, batch.n)] if games is None else [(g, sh.lo, sh.n) for g, sh in zip(games, batch.shards)]
        for g, lo, n in self._parts:
            assert self.lib.ftl_baseline_bytes(g.h, cap) == n * self.row

    def _streams(self, tensor=None):
        b = self.batch
        return b._part_streams(tensor) if hasattr(b, "_part_streams") else [b._stream()]

    def act(self):
        """Book the step just taken and decide the next action of every env (``ftl_baseline_act``); returns ``action`` f64[N, 2]."""
        self.batch._need_pool()
        sp, ap = self.state.data_ptr(), self.action.data_ptr()
        for (g, lo, n), s in zip(self._parts, self._streams()):
            _lib.check(self.lib.ftl_baseline_act(g.h, g._out_ref, sp + lo * self.row, n * self.row, self.cap, ap + lo * 16, s), self.lib)
        return self.action

    def __call__(self, obs=None):
        return self.act()

    def rollout(self, T, gamma=1.0, sensors=True, record=False):
        """``batch.rollout_baseline(self, ...)``."""
        T = int(T)
        self.batch._need_pool()
        if T < 1:
            raise ValueError("a rollout needs T >= 1")
        return self._rollout(T, None, gamma, sensors, record)

    def rollout_guided(self, resid, tail=0, gamma=1.0, sensors=True, record=False):
        """``batch.rollout_guided(self, ...)``."""
        tail = int(tail)
        self.batch._need_pool()
        if (not torch.is_tensor(resid) or resid.dim() != 3 or resid.shape[0] < 1 or tuple(resid.shape[1:]) != (self.n, 2)
                or resid.dtype != torch.float64 or resid.device != self.state.device):
            raise ValueError("resid must be a float64 [T, n_envs, 2] tensor on the batch's device with T >= 1")
        if tail < 0:
            raise ValueError("tail must be at least 0")
        self._keep_resid = resid = resid.contiguous()      # (alive until the next call: the parts of a pipelined batch read it on their streams)
        return self._rollout(int(resid.shape[0]) + tail, resid, gamma, sensors, record)

    def _rollout(self, steps, resid, gamma, sensors, record):
        """The call of every part and the return tuple of both rollouts: ``steps`` steps in all, the first ``len(resid)`` of them guided
        (``ftl_rollout_guided``); ``resid`` None is ``ftl_rollout_baseline``."""
        b, guided = self.batch, resid is not None
        T = int(resid.shape[0]) if guided else steps
        call = self.lib.ftl_rollout_guided if guided else self.lib.ftl_rollout_baseline
        actions = torch.empty(steps, self.n, 2, dtype=torch.float64, device=self.device) if record else None
        b._prepare_rollout_outputs()
        sp, ap = self.state.data_ptr(), (actions.data_ptr() if record else 0)
        flags = 0 if sensors else abi.FTL_STEP_NO_SENSORS
        for (g, lo, n), s in zip(self._parts, self._streams(actions)):
            head, res = ((g.h, T, steps - T), (resid.data_ptr() + lo * 16, self.n * 16)) if guided else ((g.h, T), ())
            _lib.check(call(*head, float(gamma), g._out_ref, C.byref(g._rollout_outputs()), sp + lo * self.row, n * self.row, self.cap, *res,
                            (ap + lo * 16) if record else None, self.n * 16 if record else 0, flags, s), self.lib)
        out = (b.rollout_ret, b.rollout_steps, b.rollout_status)
        return out + (actions,) if record else out

    def _header(self):
        self.batch._wait_parts()
        return self.state[:, :16].contiguous().view(torch.int32)

    def flags(self):
        """int32[N]: the sticky ``abi.FTL_BL_EMPTY`` / ``abi.FTL_BL_OVERFLOW`` bits of every follower (joins a pipelined batch)."""
        return self._header()[:, abi.BL_FLAGS]

    def stack_len(self):
        """int32[N]: the number of points in every follower's FIFO (joins a pipelined batch)."""
        return self._header()[:, abi.BL_COUNT]

    def front(self):
        """f64[N, 2]: the point every follower is heading for (joins a pipelined batch)."""
        head = self._header()[:, abi.BL_HEAD].long()
        pts = self.state[:, 16:].contiguous().view(torch.float64).view(self.n, self.cap, 2)
        return pts[torch.arange(self.n, device=self.device), head]
