"""Action search on the device: ``K`` candidate action sequences per env, rolled out blind on clones in a second batch, the best one kept
and refined with a shrinking radius (random shooting).  One ``ftl_search`` call per decision, no host synchronisation; the contract is the
``ftl_search`` block of ``include/ftl.h``.  ``GuidedSearch`` is the same search over residuals added to the baseline follower's closed-loop
action, with a closed-loop baseline tail behind the horizon (``ftl_search_guided``)."""
import ctypes as C
import dataclasses

import torch

from . import _lib, abi


def check_search_args(cfg, K, T, hold, iters, gamma, spread, decay):
    """The ValueErrors of ``ActionSearch`` that need no device: the action space and the ranges of ``ftl_search_params``."""
    if cfg.discrete_action_space or cfg.constant_follower_speed:
        raise ValueError("the action search draws Box(2) actions: not for a config with discrete_action_space or constant_follower_speed")
    K, T, hold, iters = int(K), int(T), int(hold), int(iters)
    if min(K, T, hold, iters) < 1:
        raise ValueError("K, T, hold and iters must be at least 1")
    if K >= 1 << 19 or iters >= 128 or T // hold >= 65536:
        raise ValueError("beyond the limits of the draw key: K < 2**19, iters < 128, T // hold < 65536")
    if not (0.0 < float(spread) <= 1.0 and 0.0 < float(decay) <= 1.0):
        raise ValueError("spread and decay must lie in (0, 1]")
    if float(gamma) - float(gamma) != 0.0:
        raise ValueError("gamma must be finite")
    return K, T, hold, iters


class _CloneSearch:
    """What ``ActionSearch`` and ``GuidedSearch`` share: the checked parameters, the clone ``VecGame(N * K)``, the buffers of
    ``ftl_search_buffers``, the radius schedule and the rule by which the clones follow the real batch's scenario pool."""

    def _setup(self, batch, what, K, T, hold, iters, gamma, spread, decay, seed, warm, own_stream, buffers):
        K, T, hold, iters = check_search_args(batch.cfg, K, T, hold, iters, gamma, spread, decay)
        if getattr(batch, "games", None) is not None:
            raise ValueError("the %s takes a VecGame: a pipelined real batch is out of scope" % what)
        from .vec_game import VecGame
        self.batch, self.n, self.device = batch, batch.n, batch.device
        self.K, self.T, self.hold, self.iters, self.gamma = K, T, hold, iters, float(gamma)
        self.spread, self.decay, self.seed, self.warm, self.own_stream = float(spread), float(decay), int(seed), bool(warm), bool(own_stream)
        self.lib = _lib.load()
        cfg = batch.cfg
        if self.own_stream:                                # the clones' own streams start past this batch's
            c = abi.Config.from_buffer_copy(cfg.c)
            c.env_id_base = cfg.c.env_id_base + self.n
            cfg = dataclasses.replace(cfg, c=c)
        n, nk = self.n, self.n * K
        self.clones = VecGame(nk, device=self.device, config=cfg)
        if self.clones.layout_id != batch.layout_id:
            raise ValueError("the clone batch got another env layout than the real batch")
        dev = self.device
        self.rows = torch.empty(n, batch.env_bytes, dtype=torch.uint8, device=dev)
        self.env_ids = torch.arange(nk, dtype=torch.int32, device=dev)
        self.row_ids = torch.div(self.env_ids, K, rounding_mode="floor").to(torch.int32)
        self.nominal = torch.zeros(T, n, 2, dtype=torch.float64, device=dev)
        self.cand = torch.zeros(T, nk, 2, dtype=torch.float64, device=dev)
        self.action = torch.zeros(n, 2, dtype=torch.float64, device=dev)
        self.best_k = torch.zeros(n, dtype=torch.int32, device=dev)
        self.best_ret = torch.zeros(n, dtype=torch.float64, device=dev)
        self.params = p = abi.SearchParams()
        p.K, p.T, p.hold, p.iters, p.gamma, p.spread, p.decay = K, T, hold, iters, self.gamma, self.spread, self.decay
        p.seed, p.flags = self.seed & ((1 << 64) - 1), abi.FTL_SEARCH_OWN_STREAM if self.own_stream else 0
        self.buffers = b = buffers()
        for name in ("rows", "row_ids", "env_ids", "nominal", "cand", "action", "best_k", "best_ret"):
            setattr(b, name, getattr(self, name).data_ptr())
        b.out, b.ro = C.pointer(self.clones._out), C.pointer(self.clones._rollout_outputs())
        self.ret = self.clones.rollout_ret                 # f64[N * K]: the returns of the last round's candidates
        self.calls = 0
        self._token = None

    def close(self):
        self.clones.close()

    def radius(self, it):
        """The radius of round ``it``: s_0 = spread, s_{it+1} = s_it * decay, as ``ftl_search`` computes it."""
        s = self.spread
        for _ in range(it):
            s = s * self.decay
        return s

    def _follow_pool(self):
        from .vec_game import _pool_token
        self.batch._need_pool()
        pool = self.batch.pool
        token = _pool_token(pool)
        if token == self._token:
            return
        if self._token is not None and token[0] == self._token[0]:
            raise ValueError("the scenario pool was written since the search loaded it (ScenarioPool.write, a moving ScenarioRing / "
                             "DeviceScenarioRing): the search is tied to the pool contents, like a snapshot")
        self.clones.load_scenarios(pool)
        self._token = token

    def _next_call(self, call):
        if call is None:
            call, self.calls = self.calls, self.calls + 1
        return int(call)

    def __call__(self, obs=None):
        return self.act()


class ActionSearch(_CloneSearch):
    """A planner for every env of ``batch`` (a ``VecGame``), usable as a policy wherever ``BaselineFollower`` is.

    ``act()`` packs the ``N`` envs, fans each out into ``K`` clones of an internal ``VecGame(N * K)`` on the same scenario pool, rolls the
    clones ``T`` steps forward without sensors under ``K`` action sequences -- candidate 0 is the plan so far, the others add uniform offsets of
    radius ``spread`` (a share of the Box(2) width, one draw per ``hold`` steps) --, keeps the sequence with the largest discounted return,
    repeats ``iters`` times with the radius times ``decay``, and returns the persistent float64 ``[N, 2]`` ``action`` = the plan's first step.
    ``best_ret`` f64[N], ``best_k`` i32[N], ``nominal`` f64[T, N, 2] (the plan) and ``cand`` f64[T, N * K, 2] show the last round.
    With ``warm`` the next call starts from the plan shifted by one step; an env whose step count is 0 (any reset discipline), and every env
    on the first call or without ``warm``, starts from (max speed, straight on).  The real batch is only read: its state and outputs are
    untouched, so an attached episode queue is no obstacle (``batch.evaluate(search, scen_ids, sensors=False)``).

    The clones keep their source's random stream: they are the env's exact future, so ``batch.rollout(search.nominal, gamma)`` returns
    ``best_ret`` bit for bit -- and the search sees the world's future random draws (leader speed regimes, random frames per step, bear
    way-points).  ``own_stream=True`` is the honest model: every clone draws from a stream of its own (outside those of this batch's envs).

    The candidates are keyed by ``seed``, the env's absolute stream id and the call counter ``calls`` (``act(call=...)`` overrides it), not
    by the env's slot.  The pool is loaded once; a batch that was given another pool is followed, a pool that was written since (a moving
    ``ScenarioRing`` / ``DeviceScenarioRing``) is refused as ``restore()`` refuses it.  A ``PipelinedVecGame`` is out of scope."""

    def __init__(self, batch, K, T, hold=1, iters=1, gamma=1.0, spread=1.0, decay=0.5, seed=0, warm=True, own_stream=False):
        self._setup(batch, "action search", K, T, hold, iters, gamma, spread, decay, seed, warm, own_stream, abi.SearchBuffers)

    def act(self, call=None):
        """Search from the batch's current state (``ftl_search`` on the current stream) and return ``action`` f64[N, 2].  ``call`` is the
        counter that keys the draws and, at 0, makes every env start from the default plan; None: ``calls``, which then advances."""
        self._follow_pool()
        _lib.check(self.lib.ftl_search(self.batch.h, self.clones.h, C.byref(self.params), self._next_call(call), 1 if self.warm else 0,
                                       C.byref(self.buffers), self.batch._stream()), self.lib)
        return self.action


class GuidedSearch(_CloneSearch):
    """``ActionSearch`` over residuals added to the baseline follower's own closed-loop action, scored over a horizon that ends in a
    closed-loop baseline tail (``ftl_search_guided``); a policy wherever ``BaselineFollower`` and ``ActionSearch`` are.

    It owns the way-point FIFOs of the real envs (``follower``, a ``BaselineFollower(batch, cap)``: ``state`` uint8 ``[N, row]``), those of
    the clones (``clone_state`` uint8 ``[N * K, row]``) and the clone ``VecGame(N * K)``.  ``act()`` packs the envs, fans each out into ``K``
    clones with its follower row and the observation its follower reads, rolls the clones ``T + tail`` blind steps forward -- in the first
    ``T`` the baseline's action is clipped to the Box(2), a candidate's residual added and the sum clipped again; the ``tail`` steps are the
    plain baseline --, keeps the residual sequence with the largest discounted return, repeats ``iters`` times with the radius times
    ``decay`` and finally decides on the real batch: ``action`` = clip(clip(baseline) + ``nominal[0]``), which books the real follower's
    step exactly once, as ``BaselineFollower.act`` does -- so call it exactly once per step.  ``nominal`` f64[T, N, 2] is the residual plan
    and ``cand`` f64[T, N * K, 2] the residual candidates, drawn as ``ActionSearch`` draws actions from the box of the same width centred on
    0.  The plan a call starts from is (0, 0) -- the baseline itself -- for a new episode, on call 0 and without ``warm``: then ``best_ret``
    is never below the baseline's return over ``T + tail`` steps, and equals it for ``K = 1``.  With the clones on their source's stream
    ``batch.rollout_guided(copy of the follower, nominal, tail, gamma)`` returns ``best_ret`` bit for bit.  The real batch's state and
    outputs are only read.  ``flags()`` / ``front()`` are the real follower's.  Everything else is as in ``ActionSearch``."""

    def __init__(self, batch, K, T, tail, hold=1, iters=1, gamma=1.0, spread=1.0, decay=0.5, seed=0, warm=True, own_stream=False, cap=64):
        from .baseline import BaselineFollower
        tail, cap = int(tail), int(cap)
        check_search_args(batch.cfg, K, T, hold, iters, gamma, spread, decay)
        if tail < 0 or tail > (1 << 31) - 1 - int(T):
            raise ValueError("tail must be at least 0 (and T + tail an int32)")
        if cap < 2:
            raise ValueError("cap must be at least 2")
        self._setup(batch, "guided search", K, T, hold, iters, gamma, spread, decay, seed, warm, own_stream, abi.GuidedBuffers)
        self.tail, self.cap = tail, cap
        self.follower = BaselineFollower(batch, cap)
        self.row = self.follower.row
        self.clone_state = torch.zeros(self.n * self.K, self.row, dtype=torch.uint8, device=self.device)
        b = self.buffers
        b.real_out = C.pointer(batch._out)
        b.real_bl, b.real_bl_bytes = self.follower.state.data_ptr(), self.n * self.row
        b.search_bl, b.search_bl_bytes = self.clone_state.data_ptr(), self.n * self.K * self.row
        b.cap = cap

    def act(self, call=None):
        """Search from the batch's current state and decide (``ftl_search_guided`` on the current stream); returns ``action`` f64[N, 2].
        ``call`` as in ``ActionSearch.act``.  Books the step just taken in the real follower: once per step."""
        self._follow_pool()
        _lib.check(self.lib.ftl_search_guided(self.batch.h, self.clones.h, C.byref(self.params), self._next_call(call), 1 if self.warm else 0,
                                              self.tail, C.byref(self.buffers), self.batch._stream()), self.lib)
        return self.action

    def flags(self):
        """``BaselineFollower.flags()`` of the real follower."""
        return self.follower.flags()

    def front(self):
        """``BaselineFollower.front()`` of the real follower."""
        return self.follower.front()
