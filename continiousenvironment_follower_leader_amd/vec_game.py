"""``VecGame`` -- N independent follow-the-leader environments advanced by one HIP kernel launch per
``step()`` (the batched counterpart of the reference's ``Game.reset/step``,
follow_the_leader_continuous_env.py:434-543, 908-945).

PyTorch is used for plumbing only: it owns the device buffers (state blob, scenario pool, outputs) and the
stream; all arithmetic happens in ``libftl_hip.so`` behind the C-ABI of ``include/ftl.h``."""
import ctypes as C
import dataclasses
import hashlib
import math
import uuid
import weakref
from contextlib import nullcontext as _nullcontext

import numpy as np
import torch

from . import _lib, abi
from .config import GameConfig, make_config
from .shard import shard_range

_DT = {0: torch.int32, 1: torch.float32, 2: torch.float64}


class ScenarioPool:
    """Post-reset scenarios (the output of the reference's reset-time generation, ENV:434-539) as device arrays."""

    @staticmethod
    def pack(cfg: GameConfig, static_rects, robot_pos, robot_dir, robot_rect, routes, init_trajs):
        """Host arrays in the layout of ``ftl_scenarios`` (routes / initial trajectories padded to route_cap / init_traj_cap)."""
        c = cfg.c
        P = len(robot_pos)
        R = cfg.n_robots
        sr = np.asarray(static_rects, np.int32).reshape(P, -1, 4)
        if sr.shape[1] != c.n_static:
            raise ValueError("scenario has %d static rects, config expects %d" % (sr.shape[1], c.n_static))
        route = np.zeros((P, c.route_cap, 2), np.float64)
        route_len = np.zeros(P, np.int32)
        it = np.zeros((P, c.init_traj_cap, 2), np.float32)
        it_len = np.zeros(P, np.int32)
        for i in range(P):
            r = np.asarray(routes[i], np.float64).reshape(-1, 2)
            t = np.asarray(init_trajs[i], np.float32).reshape(-1, 2)
            if len(r) > c.route_cap:
                raise ValueError("route of scenario %d has %d way-points > route_cap %d" % (i, len(r), c.route_cap))
            if len(r) == 1:
                raise ValueError("a one-point route makes the reference's reset raise IndexError (ENV:513)")
            if len(t) > c.init_traj_cap:
                raise ValueError("initial trajectory of scenario %d has %d points > init_traj_cap %d"
                                 % (i, len(t), c.init_traj_cap))
            route[i, :len(r)] = r
            route_len[i] = len(r)
            it[i, :len(t)] = t
            it_len[i] = len(t)
        return dict(static_rects=np.ascontiguousarray(sr),
                    robot_pos=np.ascontiguousarray(np.asarray(robot_pos, np.float32).reshape(P, R, 2)),
                    robot_dir=np.ascontiguousarray(np.asarray(robot_dir, np.float64).reshape(P, R)),
                    robot_rect=np.ascontiguousarray(np.asarray(robot_rect, np.int32).reshape(P, R, 4)),
                    route=route, route_len=route_len, init_traj=it, init_traj_len=it_len)

    def __init__(self, cfg: GameConfig, static_rects, robot_pos, robot_dir, robot_rect, routes, init_trajs, device):
        host = self.pack(cfg, static_rects, robot_pos, robot_dir, robot_rect, routes, init_trajs)
        dev = torch.device(device)
        self.n = len(host["robot_pos"])
        self.t = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        self._bind()

    def _bind(self):
        if not hasattr(self, "uid"):           # identity + content version: what an EnvSnapshot is tied to (EnvSnapshot.pool_token)
            self.uid, self.version = uuid.uuid4().hex, 0
        s = abi.Scenarios()
        s.n_scenarios = self.n
        for k, v in self.t.items():
            setattr(s, k, v.data_ptr())
        self.c_struct = s

    @classmethod
    def empty(cls, cfg: GameConfig, capacity, device):
        """A pool of ``capacity`` zeroed entries to be filled with ``write`` (ScenarioRing)."""
        c, R = cfg.c, cfg.n_robots
        shapes = dict(static_rects=((capacity, c.n_static, 4), torch.int32), robot_pos=((capacity, R, 2), torch.float32),
                      robot_dir=((capacity, R), torch.float64), robot_rect=((capacity, R, 4), torch.int32),
                      route=((capacity, c.route_cap, 2), torch.float64), route_len=((capacity,), torch.int32),
                      init_traj=((capacity, c.init_traj_cap, 2), torch.float32), init_traj_len=((capacity,), torch.int32))
        self = cls.__new__(cls)
        self.n = int(capacity)
        self.t = {k: torch.zeros(sh, dtype=dt, device=device) for k, (sh, dt) in shapes.items()}
        self._bind()
        return self

    def write(self, base, host, stream=None):
        """Copy host arrays (``pack`` layout, pinned for an asynchronous copy) over entries ``[base, base + n)`` on ``stream``."""
        n = len(host["robot_pos"])
        if base < 0 or base + n > self.n:
            raise ValueError("entries outside the pool")
        with torch.cuda.stream(stream) if stream is not None else _nullcontext():
            for k, v in host.items():
                self.t[k][base:base + n].copy_(v if isinstance(v, torch.Tensor) else torch.from_numpy(v), non_blocking=True)
        self.version += 1

    def digest(self):
        """sha256 of the pool's contents (entries ``[0, n)`` of every array, host copies): what ``VecGame.state_dict`` records so that a
        checkpoint is only loaded next to the worlds its episodes run on.  Synchronises."""
        h = hashlib.sha256()
        for k in sorted(self.t):
            t = self.t[k][:self.n].contiguous().cpu()
            h.update(k.encode())
            h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
        return h.hexdigest()

    @classmethod
    def generate(cls, cfg, seeds, device, n_threads=0):
        """Pool of the usable scenarios among python seeds ``seeds`` from the host-side generator (scenario.py): what
        ``game.seed(s); game.reset()`` builds in the reference, without the reference."""
        from .scenario import generate_scenarios
        g = generate_scenarios(cfg, seeds, n_threads)
        keep = np.nonzero(g["usable"])[0]
        if len(keep) == 0:
            raise ValueError("no usable scenario among the given seeds")
        pool = cls.__new__(cls)
        pool.n = len(keep)
        pool.t = {k: torch.from_numpy(np.ascontiguousarray(g[k][keep])).to(device) for k in
                  ("static_rects", "robot_pos", "robot_dir", "robot_rect", "route", "route_len", "init_traj", "init_traj_len")}
        pool._bind()
        pool.seeds = g["seed"][keep]
        return pool

    @classmethod
    def generate_on_device(cls, cfg, seeds, device):
        """``generate`` with the generator on the GPU (scenario.generate_scenarios_device): the usable scenarios in seed order, compacted on
        the device."""
        from .scenario import SCEN_KEYS, generate_scenarios_device
        g = generate_scenarios_device(cfg, seeds, device)
        keep = torch.nonzero(g["usable"]).reshape(-1)
        if keep.numel() == 0:
            raise ValueError("no usable scenario among the given seeds")
        pool = cls.__new__(cls)
        pool.n = int(keep.numel())
        pool.t = {k: g[k].index_select(0, keep).contiguous() for k in SCEN_KEYS}
        pool._bind()
        pool.seeds = g["seed"].index_select(0, keep)
        return pool

    @classmethod
    def from_npz(cls, cfg, path, device, limit=None):
        z = np.load(path)
        n = len(z["seed"]) if limit is None else min(limit, len(z["seed"]))
        routes = [z["route"][i, :z["route_len"][i]].astype(np.float64) for i in range(n)]
        trajs = [z["init_traj"][i, :z["init_traj_len"][i]] for i in range(n)]
        return cls(cfg, z["static_rects"][:n].astype(np.int32), z["robot_pos"][:n], z["robot_dir"][:n],
                   z["robot_rect"][:n].astype(np.int32), routes, trajs, device)


def error_for_bits(bits, n_envs=1):
    """Exception object for a set of FTL_ERR_* bits: the type the reference raises where it has one."""
    where = "%d env(s)" % n_envs
    if bits & abi.FTL_ERR_BAD_STREAM:
        return ValueError("an episode queue's stream id outside 0 .. 2**31 - 1 in %s" % where)
    if bits & abi.FTL_ERR_BAD_ACTION:           # ENV:922: discrete_rotation_speed_to_value[action] with an action outside 0..4
        return KeyError("Discrete(5) action outside 0..4 in %s" % where)
    if bits & abi.FTL_ERR_TRACKER_SEED:         # SEN:264-297 (the tracker is scanned before every ray sensor, CLS:263-267)
        return IndexError("pop from an empty deque (tracker seeded with fewer than 2 points or trimmed before the corridor "
                          "exists, sensors.py:288-297; %s)" % where)
    if bits & abi.FTL_ERR_EMPTY_CORRIDOR:       # SEN:893/962: `all_obs_arr` is unbound when len(corridor) <= 1
        return UnboundLocalError("local variable 'all_obs_arr' referenced before assignment (ray sensor scanned with a "
                                 "corridor of <= 1 points, sensors.py:893-962; %s)" % where)
    names = [n for b, n in ((abi.FTL_ERR_TRAJ_OVERFLOW, "traj_cap"), (abi.FTL_ERR_CORR_OVERFLOW, "corr_cap"), (abi.FTL_ERR_HIST1_OVERFLOW, "hist1_cap"),
                            (abi.FTL_ERR_LIDAR_OVERFLOW, "objects within a lidar's range")) if bits & b]
    return _lib.FtlError("capacity overflow of the batched state (%s) in %s: results after the overflow differ from the "
                         "reference -- raise the capacity in make_config()" % (", ".join(names) or hex(bits), where))


def _output_table(cfg, policy_obs, final_obs):
    """name -> (shape after the env axis, dtype) of the per-env output tensors of a batch, in the order snapshots carry them: the step
    outputs, ``policy_obs`` when asked for and the config has sensors for it, and with ``final_obs`` their ``final_`` twins plus the
    ``ended`` / ``restarted`` masks.  A new per-env output is one row here."""
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    t = dict(obs_num=((abi.FTL_OBS_NUM,), f32), lasers=((max(cfg.lasers_len, 1),), f32), target=((2,), f64), reward=((), f64),
             done=((), u8), status=((3,), u8))
    # fused ContinuousObserveModifier_sensorPrev output (wrappers.py:169-221): [n, H, sum of row widths], float32, over the
    # sensor classes the wrapper concatenates (LaserSpec.in_policy_obs), in dict order
    sel = [l for l in cfg.lasers if l.in_policy_obs]
    if policy_obs and sel:
        hs = {l.history for l in sel}
        if len(hs) != 1:
            raise ValueError("policy_obs needs the same max_prev_obs on every sensor it concatenates (wrappers.py:207, 217 assert it)")
        t["policy_obs"] = ((hs.pop(), sum(l.width for l in sel)), f32)
    if final_obs:                              # ftl_final_outputs: terminal rows + ended / restarted masks
        t.update(final_obs_num=t["obs_num"], final_lasers=t["lasers"], final_target=t["target"], ended=((), u8), restarted=((), u8))
        if "policy_obs" in t:
            t["final_policy_obs"] = t["policy_obs"]
    return t


class _BatchBase:
    """What ``VecGame`` and ``PipelinedVecGame`` share: every call whose body is the same once the parts have been waited for.

    A subclass provides ``_wait_parts()`` (the current stream waits for whatever steps the batch on other streams), the per-ids
    operations ``_snapshot_ids`` / ``_restore_ids`` / ``_render_ids`` and the attributes ``cfg``, ``n``, ``device``, ``pool``, ``queue``,
    ``layout_id``, ``env_bytes``, ``_window``, ``_tune``."""

    def _set_outputs(self, outs, final_obs):
        """Keep the output tensors ``outs`` (name -> tensor, the rows of ``_output_table``) as attributes and as ``output_rows()``."""
        self.final_obs = bool(final_obs)
        self.policy_obs = None
        if self.final_obs:
            self.final_policy_obs = None
        for name, t in outs.items():
            setattr(self, name, t)
        self._rows = outs

    def output_rows(self):
        """name -> the per-env output tensors a snapshot carries: the step outputs, ``policy_obs`` and the final buffers when enabled."""
        return self._rows

    def _need_pool(self):
        if self.pool is None:
            raise _lib.FtlError("load_scenarios() first")

    def _need_queue(self):
        if self.queue is None:
            raise _lib.FtlError("set_episode_queue() first")

    def _need_sampler(self):
        if self.sampler is None:
            raise _lib.FtlError("set_scenario_sampler() first")

    def _check_sampler(self, sampler):
        """A ``ScenarioSampler`` that fits this batch: same device, window inside the pool."""
        self._need_pool()
        if not isinstance(sampler, ScenarioSampler):
            raise TypeError("set_scenario_sampler() takes a ScenarioSampler or None")
        if sampler.device != self.device:
            raise ValueError("the sampler lives on %s, the batch on %s" % (sampler.device, self.device))
        if sampler.base + sampler.count > self.pool.n:
            raise ValueError("the sampler's window [%d, %d) lies outside the pool of %d scenarios"
                             % (sampler.base, sampler.base + sampler.count, self.pool.n))

    def _reset_args(self, scen_idx, mask):
        """(scen_idx i32[N], mask u8[N] or None) of a ``reset`` call as contiguous device tensors, checked."""
        self._need_pool()
        if scen_idx is None:
            scen_idx = torch.arange(self.n, dtype=torch.int32, device=self.device) % self.pool.n
        scen_idx = torch.as_tensor(scen_idx, dtype=torch.int32, device=self.device).contiguous()
        if scen_idx.numel() != self.n:
            raise ValueError("scen_idx must have one entry per env")
        if bool((scen_idx < 0).any()) or bool((scen_idx >= self.pool.n).any()):
            raise ValueError("scen_idx out of range")
        if mask is not None:
            mask = torch.as_tensor(mask, dtype=torch.uint8, device=self.device).contiguous()
        return scen_idx, mask

    def evaluate(self, policy, scen_ids, stream_ids=None, check_every=16, max_calls=None, sensors=True):
        """Play every scenario of ``scen_ids`` exactly once with ``action = policy((obs_num, lasers))`` and return the records (structured
        numpy array, ``abi.RECORD_DTYPE``, row q = entry q).  The queue's ``finished()`` count is read (one synchronisation) every
        ``check_every`` calls.  ``max_calls`` defaults to ceil(Q / n_envs) * (max_steps // least frames per step + 2) + check_every --
        no hand-out order needs more -- and exceeding it raises instead of spinning.  Detaches the queue afterwards.  The policy sees the
        whole batch's rows, so the parts of a pipelined batch are joined after every step.  ``sensors=False`` steps without the sensor
        kernels (``step(..., sensors=False)``) for a policy that reads no ray sensor: ``lasers`` then stays what the queue's reset
        scanned; the records do not depend on it."""
        q = self.set_episode_queue(scen_ids, stream_ids)
        try:
            self.reset_from_queue()

            def obs():
                self._wait_parts()
                return self.obs_num, self.lasers
            _evaluate_loop(self.cfg, self.n, q, obs, lambda a: self.step(a, auto_reset="queue", sensors=sensors), policy, check_every, max_calls)
            self._wait_parts()
            return q.records()
        finally:
            self.set_episode_queue(None)

    def rollout_baseline(self, follower, T, gamma=1.0, sensors=True, record=False):
        """``T`` closed-loop steps of the reference's baseline controller with one call and no host round trip (``ftl_rollout_baseline``):
        ``rollout`` with the action of every step decided on the stream by ``follower`` (a ``baseline.BaselineFollower`` of this batch)
        from the observation the step before it wrote -- so the outputs must hold the observation of the current state (the last reset /
        step / rollout wrote them).  Returns ``(ret, steps, status)`` as ``rollout`` does, plus with ``record=True`` the float64
        ``[T, N, 2]`` actions that were played.  Bit-identical to ``T`` times ``follower.act()`` + ``step(sensors=False; the last one as
        asked)``, and in env state and returns to ``rollout`` on the recorded actions.  Does not join a pipelined batch, like ``step``."""
        if getattr(follower, "batch", None) is not self:
            raise ValueError("rollout_baseline() takes a BaselineFollower of this batch")
        return follower.rollout(T, gamma, sensors, record)

    def rollout_guided(self, follower, resid, tail=0, gamma=1.0, sensors=True, record=False):
        """``rollout_baseline`` over ``T + tail`` steps whose first ``T`` decisions are guided by the float64 ``[T, N, 2]`` residuals
        ``resid`` (``ftl_rollout_guided``): in step t < T the baseline's action is clipped to the Box(2), ``resid[t]`` added and the sum
        clipped again; the ``tail`` steps after them are the plain baseline.  One fold and one discount across both parts.  Returns
        ``(ret, steps, status)``, plus with ``record=True`` the ``[T + tail, N, 2]`` actions that were played.  A zero ``resid`` steps the envs
        and the follower as ``rollout_baseline(follower, T + tail)`` does.  With the residual plan of a ``search.GuidedSearch`` (its
        ``nominal``) and a copy of its follower from the same state, ``ret`` is its ``best_ret`` bit for bit."""
        if getattr(follower, "batch", None) is not self:
            raise ValueError("rollout_guided() takes a BaselineFollower of this batch")
        return follower.rollout_guided(resid, tail, gamma, sensors, record)

    def rollout_mlp(self, policy, T, gamma=1.0, record=False):
        """``T`` closed-loop steps of a feed-forward policy population with one call and no host round trip (``ftl_rollout_mlp``):
        ``rollout`` with the action of every step decided on the stream by ``policy`` (an ``mlp.MlpPolicy`` of this batch) from the
        ``policy_obs`` the step before it wrote -- so the outputs must hold the observation of the current state, and every step scans.
        Returns ``(ret, steps, status)`` as ``rollout`` does, plus with ``record=True`` the ``[T, N, ...]`` actions that were played, in
        the config's encoding.  Bit-identical to ``T`` times ``policy.act()`` + ``step()``, and in env state and returns to ``rollout`` on
        the recorded actions.  Does not join a pipelined batch, like ``step``."""
        if getattr(policy, "batch", None) is not self or not hasattr(policy, "widths"):
            raise ValueError("rollout_mlp() takes an MlpPolicy of this batch")
        return policy.rollout(T, gamma, record)

    def collect_mlp(self, policy, T, noise=None, sigma=None, auto_reset="next_step", out=None):
        """``T`` stochastic closed-loop steps of a feed-forward policy population through episode boundaries with one call and no host
        round trip, recorded for a policy-gradient method (``ftl_collect_mlp``): per step ``policy.sample(noise[t], sigma)``,
        ``step(auto_reset=...)`` and a record of the reward and of what kind of transition it was.  ``noise`` float32 ``[T, N, A]`` and
        ``sigma`` float32 ``[n_sets, A]`` as ``MlpPolicy.sample`` takes them (None: the deterministic policy).  ``auto_reset`` is
        ``"next_step"`` -- ``obs[t+1]`` is the true successor of every transition, and the restart step is marked ``FTL_TR_VOID`` -- or
        ``False`` (finished envs stay done; every later row is VOID).  Returns an ``mlp.Trajectory`` (``out=`` reuses one of the same
        shape); ``mlp.gae`` turns it and a critic's values into advantages.  Bit-identical to the loop it replaces.  Does not join a
        pipelined batch, like ``step``."""
        if getattr(policy, "batch", None) is not self or not hasattr(policy, "widths"):
            raise ValueError("collect_mlp() takes an MlpPolicy of this batch")
        return policy.collect(T, noise, sigma, auto_reset, out)

    def rollout_rnn(self, policy, T, gamma=1.0, record=False):
        """``rollout_mlp`` for a recurrent policy population (an ``rnn.RecurrentPolicy`` of this batch; ``ftl_rollout_rnn``): every step
        is one decision with its state update on the stream and one scanning step; a finished env's state row is zeroed.  Bit-identical
        to ``T`` times ``policy.act()`` + ``step()``, ``policy.state`` included.  Does not join a pipelined batch, like ``step``."""
        if getattr(policy, "batch", None) is not self or not hasattr(policy, "cell"):
            raise ValueError("rollout_rnn() takes a RecurrentPolicy of this batch")
        return policy.rollout(T, gamma, record)

    def collect_rnn(self, policy, T, noise=None, sigma=None, auto_reset="next_step", out=None, record_state=False):
        """``collect_mlp`` for a recurrent policy population (``ftl_collect_rnn``).  The ``mlp.Trajectory`` gains ``state`` float32
        ``[1 or T, N, S]``: the state rows decision t read (``record_state=True``: every t; else only t = 0, what back-propagation through
        time starts from).  The state is zeroed after the decision of every ``FTL_TR_VOID`` row, so the row the first decision of an
        episode reads is all zeros.  ``mlp.gae`` works on the result unchanged.  Bit-identical to the loop it replaces.  Does not join a
        pipelined batch, like ``step``."""
        if getattr(policy, "batch", None) is not self or not hasattr(policy, "cell"):
            raise ValueError("collect_rnn() takes a RecurrentPolicy of this batch")
        return policy.collect(T, noise, sigma, auto_reset, out, record_state)

    def terminated_truncated(self):
        """(terminated, truncated) bool [N] device tensors of the last step, without a host synchronisation (needs ``final_obs=True``):
        truncated = ended and mission status FINISHED_BY_TIME (the reference's max_steps limit, ENV:1126-1134: a value bootstrap
        continues from the terminal observation), terminated = ended and not truncated.  The statuses are the reference's own: it tests
        the step limit after the crash tests of the frame, so a crash in the frame that reaches max_steps reads as a time-out.
        Computed on the current stream: on a pipelined batch ``join()`` first (or take part k's rows of ``ended`` / ``status`` on
        ``stream(k)``)."""
        if not self.final_obs:
            raise ValueError("terminated_truncated() needs %s(..., final_obs=True)" % type(self).__name__)
        ended = self.ended.bool()
        truncated = ended & (self.status[:, 0] == abi.MISSION.index("finished_by_time"))
        return ended & ~truncated, truncated

    # ------------------------------------------------------------------ snapshot / clone / restore (ftl_pack_envs, ftl_unpack_envs)
    # over env indices of the whole batch; on a pipelined batch each is a synchronisation point (the parts are joined first, as
    # state_field does): rows move between the parts on the current stream, which the parts' next steps wait for
    def snapshot(self, env_ids=None):
        """``EnvSnapshot`` of envs ``env_ids`` (env indices of this batch, repeats allowed; None: all) -- the packed state rows and the output
        rows, enqueued on the current stream.  Tied to the scenario pool as it is now (see ``EnvSnapshot``).  Reads the ids on the host.
        Refused while an episode queue is attached: the rows would not say which entries their envs are playing."""
        _refuse_with_queue(self.queue, "snapshot()")
        self._wait_parts()
        ids = _host_ids(env_ids, self.n)
        self._need_pool()
        return self._snapshot_ids(ids)

    def restore(self, snap, env_ids=None, slot_stats=False, own_stream=False):
        """Write the envs of ``snap`` into envs ``env_ids`` of this batch (distinct indices, one per snapshot row; None: 0 .. len(snap) - 1):
        their state and their output rows, so that ``obs_num`` etc. show the restored envs at once.  Each env then continues its source's
        episode bit for bit under the same actions: it keeps its source's random stream (``own_stream=True``: the destination's own, which
        diverges on the first random draw).  ``slot_stats=True`` also moves the slot's episode records (``ep_stats``, episode count, sticky
        error word: ``episode_metrics`` counts the source's episodes again); by default the destination keeps its own.  Raises ValueError,
        with nothing written, for ids out of range or repeated, a snapshot of another layout, or a pool that changed since the snapshot."""
        self._wait_parts()
        ids = _host_ids(env_ids, self.n) if env_ids is not None else torch.arange(len(snap), dtype=torch.int64)
        self._check_snapshot(snap, ids)
        self._restore_ids(snap, ids, slot_stats, own_stream)

    def _check_snapshot(self, snap, ids):
        self._need_pool()
        if not isinstance(snap, EnvSnapshot):
            raise TypeError("restore() takes an EnvSnapshot")
        if snap.layout_id != self.layout_id:
            raise ValueError("the snapshot was taken from a batch of another layout (config, capacities or sensors differ)")
        if snap.pool_token != _pool_token(self.pool):
            raise ValueError("the scenario pool is not the one the snapshot was taken on, or it was written since (ScenarioPool.write, a "
                             "moving ScenarioRing / DeviceScenarioRing): snapshots are tied to the pool contents")
        if int(ids.numel()) != len(snap):
            raise ValueError("%d destination ids for %d snapshot rows" % (ids.numel(), len(snap)))
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.n):
            raise ValueError("env_ids outside [0, %d)" % self.n)
        if torch.unique(ids).numel() != ids.numel():
            raise ValueError("duplicate destination env ids")
        missing = [k for k in self.output_rows() if k not in snap.outputs]
        if missing:
            raise ValueError("the snapshot lacks the output rows %s of this batch" % missing)

    def clone(self, src_ids, dst_ids, slot_stats=False, own_stream=False):
        """Copy envs ``src_ids`` into envs ``dst_ids`` (``restore`` of a ``snapshot``: every source is read before any destination is written,
        so a destination may also be a source, e.g. a permutation; on a pipelined batch they may lie in different parts).  The search
        case: one env into K slots, each stepped with another action."""
        self._wait_parts()
        src, dst = _host_ids(src_ids, self.n), _host_ids(dst_ids, self.n)
        if src.numel() != dst.numel():
            raise ValueError("src_ids and dst_ids differ in length")
        if torch.unique(dst).numel() != dst.numel():
            raise ValueError("duplicate destination env ids")
        self._need_pool()
        self._restore_ids(self._snapshot_ids(src), dst, slot_stats, own_stream)

    def state_dict(self):
        """The whole batch as a checkpoint of plain tensors (``torch.save`` / ``torch.load`` it): every env's row in global env order, with
        its slot records, the output rows, ``env_id_base`` / ``n_envs``, the reset window, the ``tune`` settings (none for a pipelined
        batch: its parts keep their own) and a content digest of the scenario pool.  Synchronises.  Refused while an episode queue is
        attached (a half-drained queue is not part of a checkpoint: drain it or detach it first)."""
        _refuse_with_queue(self.queue, "state_dict()")
        self._wait_parts()
        self._need_pool()
        snap = self._snapshot_ids(torch.arange(self.n, dtype=torch.int64))
        return dict(format=1, layout_id=self.layout_id, env_id_base=int(self.cfg.c.env_id_base), n_envs=self.n,
                    rows=snap.rows.cpu(), outputs={k: v.cpu() for k, v in snap.outputs.items()},
                    reset_window=self._window, tune=dict(self._tune), pool_n=int(self.pool.n), pool_digest=self.pool.digest())

    # ------------------------------------------------------------------ views
    def laser_view(self, name):
        for l in self.cfg.lasers:
            if l.name == name:
                return self.lasers[:, l.out_offset:l.out_offset + l.history * l.width].view(self.n, l.history, l.width)
        raise KeyError(name)

    def aux_view(self, name):
        """Output block of a LaserSensor / LeaderTrackDetector_vector / _radar sensor: float32 ``[n_envs, *shape]`` with the shape
        the reference's ``scan`` returns (SEN:131-134, 381, 476)."""
        for a in self.cfg.aux:
            if a.name == name:
                return self.lasers[:, a.out_offset:a.out_offset + a.out_len].view(self.n, *a.shape)
        raise KeyError(name)

    # ------------------------------------------------------------------ rendering (ftl_render)
    def render_layers(self):
        """FTL_RENDER_* bits of the constructor's show_* flags (ENV:267-272); the target ring is always drawn (ENV:1278)."""
        return _render_layers(self.cfg)

    def render(self, env_ids=None, scale=1.0, size=None, origin=(0, 0), layers=None, out=None):
        """Top-down RGB frames of envs ``env_ids`` (env indices, repeats allowed; None: all) as a uint8 device tensor ``[k, H, W, 3]``
        (row-major ``[y][x][rgb]``, the reference's ``render()`` matrix), enqueued on the current stream without a host synchronisation.
        ``scale``: world pixels per output pixel; ``size``: (W, H) in output pixels (default: the world at this scale); ``origin``: world
        coordinate of the top-left corner; ``layers``: FTL_RENDER_* bits (None: the constructor's show_* flags); ``out``: a contiguous
        uint8 ``[k, H, W, 3]`` tensor to write into (e.g. frame t of a ``[T, k, H, W, 3]`` recording).  Reads the state and the outputs of
        the last reset / step, writes nothing else (include/ftl.h, ftl_render).  Memory: the image is k * H * W * 3 bytes and the cached
        workspace about k * (route_cap + traj_cap + ...) * 32 bytes (59 KB per env on config B) -- ``env_ids=None`` on a 65,536-env batch
        asks for 3.9 GB of workspace and, at scale 1, 295 GB of frames: pass the envs to record.  The workspace of the last k is kept
        until the next call with another k (``release_render_workspace`` frees it).  On a pipelined batch the ids may span parts and the
        call is a synchronisation point: it joins the parts and reads the ids on the host."""
        self._wait_parts()
        return self._render_ids(_render_ids(env_ids, self.n, self.device), scale, size, origin, layers, out)

    def _render_out(self, k, w, h, out):
        """The tensor ``render`` writes ``k`` frames of ``w`` x ``h`` into: ``out`` checked, or a new one."""
        if out is None:
            return torch.empty(k, h, w, 3, dtype=torch.uint8, device=self.device)
        if tuple(out.shape) != (k, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous uint8 tensor [%d, %d, %d, 3] on %s" % (k, h, w, self.device))
        return out


class VecGame(_BatchBase):
    """N parallel envs on one GPU.

    ``reset(scen_idx, mask)`` / ``step(action, auto_reset)`` return views of persistent device tensors:
    ``obs_num`` f32[N,10] (numerical_features, ENV:1793-1802), ``lasers`` f32[N, sum_k H_k*N_k] (one
    ``[H_k, N_k]`` block per ray sensor, ``laser_view(name)``), ``target`` f64[N,2], ``reward`` f64[N],
    ``done`` u8[N], ``status`` u8[N,3] (mission/agent/leader codes of ``abi.MISSION/AGENT/LEADER``).

    ``final_obs=True`` adds the persistent tensors of ``ftl_step_final``, passed on every step except ``auto_reset=True``:
    ``final_obs_num``, ``final_lasers``, ``final_target`` (+ ``final_policy_obs`` with ``policy_obs``) hold the terminal observation
    of the envs whose episode ended in the last ``auto_reset="same_step"`` step (other rows keep older values); ``ended`` u8[N] marks
    the envs whose episode ended in the last step, ``restarted`` u8[N] the envs it re-initialised (``terminated_truncated()``).

    Evaluation: ``set_episode_queue`` / ``reset_from_queue`` / ``step(a, auto_reset="queue")`` play a list of scenarios exactly once
    each, whichever slot is free, with one record per entry (``EpisodeQueue``); ``evaluate(policy, scen_ids)`` is the whole loop.

    Curricula: ``set_scenario_sampler`` / ``reset_from_sampler`` / ``step(a, auto_reset="sample")`` restart a finished env on a world drawn
    from the weights of a ``ScenarioSampler`` and add the episode it ended to the sampler's per-scenario table, all on the device."""

    def __init__(self, n_envs, device="cuda:0", config: GameConfig = None, policy_obs=False, _outputs=None, final_obs=False, **game_kwargs):
        self.cfg = config if config is not None else make_config(**game_kwargs)
        self.n = int(n_envs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.FtlError("VecGame needs a ROCm device (got %s): there is no CPU path" % self.device)
        if not torch.cuda.is_available():
            raise _lib.FtlError("no ROCm device is visible: the batched env runs on the GPU only (there is no CPU path)")
        self.lib = _lib.load()
        h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.ftl_create(C.byref(self.cfg.c), self.n, dev_index, C.byref(h)), self.lib)
        self.h = h
        nbytes = self.lib.ftl_state_bytes(self.h)
        with torch.cuda.device(self.device):
            self.state = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = self.state.data_ptr()
        self._state_off = (-base) % 256
        _lib.check(self.lib.ftl_bind_state(self.h, base + self._state_off, nbytes), self.lib)
        outs = {}
        for name, (shape, dtype) in _output_table(self.cfg, policy_obs, final_obs).items():
            if _outputs is None:
                outs[name] = torch.zeros(self.n, *shape, dtype=dtype, device=self.device)
                continue
            t = outs[name] = _outputs[name]    # the rows of a larger tensor that the caller owns (PipelinedVecGame)
            if tuple(t.shape) != (self.n, *shape) or t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
                raise ValueError("output tensor %r does not fit this batch" % name)
        self._set_outputs(outs, final_obs)
        o, f = abi.Outputs(), abi.FinalOutputs()
        for field, _ in abi.Outputs._fields_:
            if field in outs:
                setattr(o, field, outs[field].data_ptr())
        for field, _ in abi.FinalOutputs._fields_:      # a field that ftl_outputs has too is that output's final_ twin
            t = outs.get("final_" + field if hasattr(o, field) else field)
            if t is not None:
                setattr(f, field, t.data_ptr())
        self._fin = f if self.final_obs else None
        self._metrics = torch.zeros(abi.FTL_N_METRICS, dtype=torch.float64, device=self.device)
        self._errors = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._out, self._out_ref = o, C.byref(o)
        self.pool = None
        self._fields = {}
        self._window = None
        self._tune = {}
        self.queue = None
        self.ticket = None
        self.sampler = None
        self.env_bytes = int(self.lib.ftl_env_bytes(self.h))
        self.layout_id = int(self.lib.ftl_env_layout_id(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.ftl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ scenarios / reset / step
    def load_scenarios(self, pool: ScenarioPool):
        self.pool = pool
        _lib.check(self.lib.ftl_load_scenarios(self.h, C.byref(pool.c_struct)), self.lib)
        self._window = (0, pool.n, self.n % pool.n)

    def set_reset_window(self, base, count, stride=0):
        """Pool entries ``[base, base + count)`` the in-kernel auto-reset draws from and the step of its walk (``ftl_set_reset_window``;
        the whole pool with stride n_envs after ``load_scenarios``): how a ``ScenarioRing`` hands freshly generated worlds to a running
        batch.  ``stride`` should be coprime to ``count`` (0 keeps n_envs)."""
        _lib.check(self.lib.ftl_set_reset_window(self.h, int(base), int(count), int(stride)), self.lib)
        self._window = (int(base), int(count), (int(stride) if int(stride) > 0 else self.n) % int(count))

    def tune(self, coscheduled_envs=None, regroup_every=None, two_streams=None):
        """Scheduling hints (``ftl_tune``; results never depend on them): how many envs are stepped on the device at the same time when
        this batch is one of several on several streams, how often the cost order of the envs is rebuilt, the handle's own two-stream mode."""
        for name, key, v in (("coscheduled_envs", abi.FTL_TUNE_COSCHEDULED_ENVS, coscheduled_envs), ("regroup_every", abi.FTL_TUNE_REGROUP_EVERY, regroup_every),
                             ("two_streams", abi.FTL_TUNE_TWO_STREAMS, two_streams)):
            if v is not None:
                _lib.check(self.lib.ftl_tune(self.h, key, int(v)), self.lib)
                self._tune[name] = int(v)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self, scen_idx=None, mask=None, check_errors=False, live_errors=False):
        scen_idx, mask = self._reset_args(scen_idx, mask)
        mptr = mask.data_ptr() if mask is not None else None
        self._keep = (scen_idx, mask)
        _lib.check(self.lib.ftl_reset(self.h, scen_idx.data_ptr(), mptr, C.byref(self._out), self._stream()), self.lib)
        if check_errors:
            self.raise_on_errors(live_errors)
        return self.obs_num, self.lasers

    def step(self, action, auto_reset=False, check_errors=False, live_errors=False, sensors=True):
        """action: f64[N,2] device tensor = (speed px/frame, signed rotation deg/frame) (ENV:927-933).  With
        ``discrete_action_space=True`` an integer tensor [N] (or [N,1]) of Discrete(5) indices, with ``constant_follower_speed=True`` a
        float tensor [N] (or [N,1]) of rotations: both are decoded on the device as ENV:909-925 does (``ftl_step_encoded``).
        ``auto_reset``: False -- finished envs stay done; True -- they are re-initialised inside this step, the outputs keep the terminal
        reward / done / status and the new episode's observation (FTL_STEP_AUTO_RESET); ``"same_step"`` -- True plus the terminal
        observations in the final buffers (needs ``final_obs=True``); ``"next_step"`` -- this step returns the terminal observation, an env
        that is done on entry is re-initialised instead of stepped (its action ignored; reward 0, done 0, status 0: FTL_STEP_NEXT_RESET);
        ``"queue"`` -- a finished env records its episode and takes the next entry of the attached episode queue, or parks
        (``set_episode_queue``; FTL_STEP_QUEUE_RESET; outputs as under True, the final buffers are filled when the batch has them);
        ``"sample"`` -- a finished env adds its episode to the table of the attached ``ScenarioSampler`` and restarts on a world drawn from
        its weights (``set_scenario_sampler``; FTL_STEP_SAMPLE_RESET; outputs as under True, the final buffers are filled when the batch has
        them, ``ended`` = ``restarted`` = done).
        ``sensors=False`` (with any ``auto_reset`` value; FTL_STEP_NO_SENSORS) leaves out the sensor kernels: ``lasers`` and ``policy_obs``
        are not written and go stale -- they keep the readings of the last scan, and under ``"same_step"`` / ``"queue"`` / ``"sample"``
        ``final_lasers`` / ``final_policy_obs`` are copies of those stale rows -- while ``obs_num``, ``target``, ``reward``, ``done``,
        ``status``, the masks and the whole state are what the same step with sensors gives; ``scan()`` brings the readings up to date.
        ``check_errors=True`` synchronises and raises what the reference would have raised in any env (``raise_on_errors``);
        the default leaves the per-env sticky error words for ``error_report()`` so that the step stays asynchronous."""
        action, enc = self._encode_action(action, self.n)
        flags, fin = self._step_mode(auto_reset)
        self._step_final(action.data_ptr(), enc, flags | (0 if sensors else abi.FTL_STEP_NO_SENSORS), fin, self._stream())
        if check_errors:
            self.raise_on_errors(live_errors)
        return self.obs_num, self.lasers, self.reward, self.done, self.status

    def scan(self):
        """The sensor half of a step on the current state (``ftl_scan``): refreshes ``lasers``, and ``policy_obs`` when the batch has it, on
        the current stream and returns ``lasers``.  After ``step(..., sensors=False)`` the readings are those the same step with sensors
        gives; after ``restore()`` / ``clone()`` those the source env had.  Touches nothing else."""
        self._need_pool()
        self._scan(self._stream())
        return self.lasers

    def _scan(self, stream):
        _lib.check(self.lib.ftl_scan(self.h, self._out_ref, stream), self.lib)

    def rollout(self, actions, gamma=1.0, sensors=True):
        """T steps without auto-reset under the open-loop action sequence ``actions`` with one call (``ftl_rollout``): ``[T, N, 2]`` float64,
        ``[T, N]`` integers for Discrete(5) or ``[T, N]`` floats for Box(1), checked as ``step`` checks one step's actions.  Returns
        ``(ret, steps, status)``, persistent device tensors allocated on first use: ``ret`` f64[N] = sum of gamma**t * reward_t over the
        steps the env was alive in (its done word 0 on entry; the step that raises done counts), ``steps`` i32[N] the number of such steps
        (0 for an env that was done on entry), ``status`` u8[N,3] the status row of the step that ended the episode (0/0/0 if none did).
        The step outputs are those of step T-1; only that step scans, and with ``sensors=False`` none does (``lasers`` / ``policy_obs``
        go stale as under ``step(..., sensors=False)``)."""
        self._need_pool()
        flat, enc, T = self._encode_rollout(actions, self.n)
        row = flat.element_size() * (2 if enc == abi.FTL_ACTION_BOX2 else 1)
        self._rollout(flat.data_ptr(), self.n * row, enc, T, gamma, sensors, self._stream())
        return self.rollout_ret, self.rollout_steps, self.rollout_status

    def _encode_rollout(self, actions, n):
        """(the [T * n, ..] tensor ``_encode_action`` makes of a [T, n, ..] action sequence, its encoding, T)."""
        if actions.dim() < 2 or actions.shape[0] < 1 or actions.shape[1] != n:
            raise ValueError("a rollout's actions must be [T, n_envs, ...] with T >= 1")
        T = int(actions.shape[0])
        flat, enc = self._encode_action(actions.reshape(T * n, *actions.shape[2:]), T * n)
        self._keep_rollout = flat
        return flat, enc, T

    def _rollout_outputs(self, views=None):
        """Allocate (or, the parts of a pipelined batch, take as ``views``) the persistent ``rollout_ret`` / ``_steps`` / ``_status``."""
        if getattr(self, "_ro", None) is None:
            if views is None:
                views = (torch.zeros(self.n, dtype=torch.float64, device=self.device), torch.zeros(self.n, dtype=torch.int32, device=self.device),
                         torch.zeros(self.n, 3, dtype=torch.uint8, device=self.device))
            self.rollout_ret, self.rollout_steps, self.rollout_status = views
            ro = abi.RolloutOutputs()
            ro.ret, ro.steps, ro.status = (t.data_ptr() for t in views)
            self._ro = ro
        return self._ro

    def _prepare_rollout_outputs(self):
        self._rollout_outputs()

    def _rollout(self, action_ptr, step_bytes, enc, T, gamma, sensors, stream):
        """The one call of ``ftl_rollout``: ``action_ptr`` the device address of this batch's first action row of step 0."""
        ro = self._rollout_outputs()
        _lib.check(self.lib.ftl_rollout(self.h, action_ptr, step_bytes, enc, T, float(gamma), self._out_ref, C.byref(ro),
                                        0 if sensors else abi.FTL_STEP_NO_SENSORS, stream), self.lib)

    def _step_final(self, action_ptr, enc, flags, fin, stream):
        """The one call of ``ftl_step_final``: ``action_ptr`` the device address of this batch's first action row, ``fin`` as
        ``_step_mode`` gives it, ``stream`` a ``c_void_p``."""
        _lib.check(self.lib.ftl_step_final(self.h, action_ptr, enc, self._out_ref, fin, flags, stream), self.lib)

    def _step_mode(self, auto_reset):
        """(FTL_STEP_* flags, ftl_final_outputs pointer or None) of a ``step(auto_reset=...)`` value."""
        fin = C.byref(self._fin) if self._fin is not None else None
        if not isinstance(auto_reset, str):
            if auto_reset:                     # today's meaning exactly: no final buffers
                return abi.FTL_STEP_AUTO_RESET, None
            return 0, fin
        if auto_reset == "same_step":
            if fin is None:
                raise ValueError('auto_reset="same_step" needs the final buffers: VecGame(..., final_obs=True)')
            return abi.FTL_STEP_AUTO_RESET, fin
        if auto_reset == "next_step":
            return abi.FTL_STEP_NEXT_RESET, fin
        if auto_reset == "queue":
            if self.queue is None:
                raise _lib.FtlError('auto_reset="queue" needs set_episode_queue() first')
            return abi.FTL_STEP_QUEUE_RESET, fin
        if auto_reset == "sample":
            if self.sampler is None:
                raise _lib.FtlError('auto_reset="sample" needs set_scenario_sampler() first')
            return abi.FTL_STEP_SAMPLE_RESET, fin
        raise ValueError('auto_reset must be False, True, "same_step", "next_step", "queue" or "sample" (got %r)' % (auto_reset,))

    # ------------------------------------------------------------------ episode queue (ftl_set_episode_queue, ftl_queue_start)
    def set_episode_queue(self, scen_ids, stream_ids=None, stream_base=0):
        """Attach a queue of pool indices ``scen_ids`` [Q] to this batch and return its ``EpisodeQueue``: every entry is played exactly
        once by whichever slot is free, entry q on random stream ``stream_ids[q]`` (default ``stream_base + q``), and its result goes to
        row q of the queue's table.  The episode of entry q is what env q of a fresh ``VecGame(Q, env_id_base=stream_base)`` reset on
        ``scen_ids`` plays under the same actions, whatever ``n_envs`` is.  ``scen_ids`` may be an ``EpisodeQueue`` (the parts of a
        pipelined batch share one); ``None`` detaches.  Follow with ``reset_from_queue()`` and ``step(a, auto_reset="queue")``.  A queue is
        not refilled while it drains: attach a new one."""
        if scen_ids is None:
            _lib.check(self.lib.ftl_set_episode_queue(self.h, None), self.lib)
            self.queue = self.ticket = self._queue_c = None
            return None
        self._need_pool()
        q = scen_ids if isinstance(scen_ids, EpisodeQueue) else EpisodeQueue(scen_ids, stream_ids, stream_base, self.device, self.pool.n)
        ticket = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
        c = q.c_struct(ticket)
        _lib.check(self.lib.ftl_set_episode_queue(self.h, C.byref(c)), self.lib)
        self.queue, self.ticket, self._queue_c = q, ticket, c
        return q

    def reset_from_queue(self):
        """The queue's ``reset()``: slot e takes entry head + e (slots past the end of the queue park: ``ticket`` -1, done set); returns the
        first observations like ``reset``."""
        self._need_queue()
        _lib.check(self.lib.ftl_queue_start(self.h, C.byref(self._out), self._stream()), self.lib)
        return self.obs_num, self.lasers

    # ------------------------------------------------------------------ scenario sampler (ftl_set_scenario_sampler, ftl_sampler_start)
    def set_scenario_sampler(self, sampler, _owner=None):
        """Attach a ``ScenarioSampler`` (``None`` detaches: the batch is then exactly what it was before): ``step(a, auto_reset="sample")``
        restarts every finished env on pool entry ``base + idx`` drawn from the sampler's weights and adds the episode it ended to the
        sampler's table.  Builds the sampler's cdf on the current stream (``refresh_sampler``).  Follow with ``reset_from_sampler()`` or
        keep the running episodes.  Snapshots, ``clone`` and ``state_dict`` work as without one: the sampler keeps no per-slot state (save
        its weights and table with ``ScenarioSampler.state_dict``)."""
        if sampler is None:
            _lib.check(self.lib.ftl_set_scenario_sampler(self.h, None), self.lib)
            self.sampler = self._sampler_c = None
            return None
        self._check_sampler(sampler)
        c = sampler.c_struct()
        _lib.check(self.lib.ftl_set_scenario_sampler(self.h, C.byref(c)), self.lib)
        self.sampler, self._sampler_c = sampler, c
        if _owner is None:                       # (the parts of a pipelined batch: the whole batch owns the sampler and refreshes once)
            sampler._attach(self)
            self.refresh_sampler()
        return sampler

    def refresh_sampler(self):
        """Rebuild the sampler's cdf from its weights on the current stream (``ftl_sampler_refresh``); ``ScenarioSampler.set_weights``
        calls it.  Steps enqueued later on this stream draw from the new cdf."""
        self._need_sampler()
        _lib.check(self.lib.ftl_sampler_refresh(self.h, self._stream()), self.lib)

    def reset_from_sampler(self):
        """The sampler's ``reset()``: every slot draws its world with the stream / reset-count words its state holds (no table update);
        returns the first observations like ``reset``."""
        self._need_sampler()
        _lib.check(self.lib.ftl_sampler_start(self.h, C.byref(self._out), self._stream()), self.lib)
        return self.obs_num, self.lasers

    def _encode_action(self, action, n):
        """(tensor to hand to ftl_step_encoded, FTL_ACTION_* encoding) for an action of ``n`` envs of this config (ENV:909-925)."""
        enc = abi.FTL_ACTION_BOX2
        if action.device != self.device:
            raise ValueError("action must live on %s" % self.device)
        if self.cfg.discrete_action_space or self.cfg.constant_follower_speed:
            if tuple(action.shape) not in ((n,), (n, 1)):
                raise ValueError("action must be [n_envs] or [n_envs, 1] for this action space (ENV:358-372)")
            if self.cfg.discrete_action_space and self.cfg.constant_follower_speed:
                # ENV:922 then ENV:925: np.concatenate([[0.25], (max_speed, rotation)]) -- the follower's max_speed ends up as the rotation
                action = torch.tensor([0.25, self.cfg.c.follower.max_speed], dtype=torch.float64, device=self.device).repeat(n, 1)
            elif self.cfg.discrete_action_space:
                if action.dtype.is_floating_point or action.dtype == torch.bool:
                    raise ValueError("Discrete(5) actions must be an integer tensor")
                action, enc = action.reshape(n).to(torch.int32).contiguous(), abi.FTL_ACTION_DISCRETE
            else:
                if not action.dtype.is_floating_point:
                    raise ValueError("Box(1) actions must be a float tensor")
                action, enc = action.reshape(n).to(torch.float64).contiguous(), abi.FTL_ACTION_TURN
            self._keep_action = action
        elif action.dtype != torch.float64 or not action.is_contiguous() or tuple(action.shape) != (n, 2):
            raise ValueError("action must be a contiguous float64 [n_envs, 2] tensor on %s" % self.device)
        return action, enc

    # ------------------------------------------------------------------ episode metrics / error report
    def episode_metrics(self, clear=False):
        """f64[8] device tensor ``[episodes, sum return, sum frames, n_success, n_crash, n_low_reward, n_too_far, n_timeout]``
        over the episodes that ended since the state was created (or since the last ``clear=True`` call): what the
        reference reports at ``done`` (ENV:941-944), accumulated on the device before auto-reset wipes the counters.
        This is the vector a multi-GPU job all-reduces (``shard.reduce_metrics``).  Also refreshes ``error_report()``."""
        flags = abi.FTL_METRICS_CLEAR if clear else 0
        _lib.check(self.lib.ftl_episode_metrics(self.h, self._metrics.data_ptr(), self._errors.data_ptr(), flags, self._stream()), self.lib)
        return self._metrics

    def kernel_timing(self, enable=True):
        """Measurement hook: HIP events around every kernel of the following steps (``kernel_times``)."""
        _lib.check(self.lib.ftl_kernel_timing(self.h, 1 if enable else 0), self.lib)

    def kernel_times(self):
        """Average per-kernel duration in microseconds over the steps timed since the last call:
        ``dict(frames_us, rays_us, aux_us, regroup_us, steps)`` (frames includes the v1 tracker's kernel when the config has one; aux =
        ftl_aux_kernel of configs with row-f3 sensors; regroup = both regroup kernels, averaged over ALL steps)."""
        ms, n = (C.c_double * 4)(), C.c_int32()
        _lib.check(self.lib.ftl_kernel_times(self.h, C.byref(ms), C.byref(n)), self.lib)
        k = max(n.value, 1)
        return dict(frames_us=ms[0] / k * 1e3, rays_us=ms[1] / k * 1e3, aux_us=ms[2] / k * 1e3, regroup_us=ms[3] / k * 1e3, steps=n.value)

    def error_report(self):
        """(number of envs whose sticky error word is set, OR of the FTL_ERR_* bits) -- the conditions under which a
        reference run would have raised (or a capacity of the batched state overflowed).  The words survive reset and
        auto-reset; ``episode_metrics(clear=True)`` clears them together with the metrics records."""
        self.episode_metrics()
        n, bits = self._errors.tolist()
        return int(n), int(bits)

    def raise_on_errors(self, live=False):
        """The exception the reference would have raised (or FtlError for a capacity overflow) if any env reported one.
        ``live=True`` looks at the error words of the episodes in progress (``FTL_EI_ERROR``, cleared by reset like the sensors the
        reference's reset() rebuilds) instead of the sticky words that survive resets: what a caller that handles the exception and
        resets -- the single-env facade -- needs."""
        if live:
            w = self.state_field("env_int")[:, abi.EI_ERROR]
            bad = w != 0
            n = int(bad.sum().item())
            bits = 0
            if n:
                for v in w[bad].unique().tolist():
                    bits |= int(v)
        else:
            n, bits = self.error_report()
        if bits:
            raise error_for_bits(bits, n)

    # ------------------------------------------------------------------ the per-ids operations under snapshot / restore / clone
    def _wait_parts(self):
        pass

    def _snapshot_ids(self, ids):
        k = int(ids.numel())
        rows = torch.empty(k, self.env_bytes, dtype=torch.uint8, device=self.device)
        dev = ids.to(device=self.device, dtype=torch.int32)
        if k:
            _lib.check(self.lib.ftl_pack_envs(self.h, dev.data_ptr(), k, rows.data_ptr(), self._stream()), self.lib)
        idx = dev.long()
        outs = {name: t.index_select(0, idx) for name, t in self.output_rows().items()}
        return EnvSnapshot(rows, outs, self.layout_id, _pool_token(self.pool))

    def _restore_ids(self, snap, ids, slot_stats, own_stream):
        k = int(ids.numel())
        if k == 0:
            return
        flags = (abi.FTL_ENV_SLOT_STATS if slot_stats else 0) | (abi.FTL_ENV_OWN_STREAM if own_stream else 0)
        rows = snap.rows.to(self.device).contiguous()
        dev = ids.to(device=self.device, dtype=torch.int32)
        _lib.check(self.lib.ftl_unpack_envs(self.h, rows.data_ptr(), dev.data_ptr(), k, flags, self._stream()), self.lib)
        self._keep_restore = (rows, dev)
        idx = dev.long()
        for name, t in self.output_rows().items():
            t.index_copy_(0, idx, snap.outputs[name].to(self.device))

    def load_state_dict(self, sd, apply_tune=True, _digest=None):
        """Continue a checkpoint of ``state_dict``: this batch takes the rows whose global env ids (env_id_base + index) it owns, with their
        slot records -- a checkpoint of one batch loads into batches of other sizes / bases that together cover it (re-sharding, shard.py).
        Needs ``load_scenarios`` of a pool with the checkpoint's contents first; sets the checkpoint's reset window (its stride, not this
        batch's n_envs) and, with ``apply_tune``, its ``tune`` settings where they fit this batch."""
        self._need_pool()
        if sd.get("format") != 1 or int(sd["layout_id"]) != self.layout_id:
            raise ValueError("the checkpoint was taken from a batch of another layout (config, capacities or sensors differ)")
        base0, n0 = int(sd["env_id_base"]), int(sd["n_envs"])
        lo = int(self.cfg.c.env_id_base) - base0
        if lo < 0 or lo + self.n > n0:
            raise ValueError("the checkpoint holds global envs [%d, %d); this batch is [%d, %d)"
                             % (base0, base0 + n0, self.cfg.c.env_id_base, self.cfg.c.env_id_base + self.n))
        if int(sd["pool_n"]) != self.pool.n or sd["pool_digest"] != (_digest or self.pool.digest()):
            raise ValueError("the scenario pool differs from the checkpoint's (content digest)")
        missing = [k for k in self.output_rows() if k not in sd["outputs"]]
        if missing:
            raise ValueError("the checkpoint lacks the output rows %s of this batch" % missing)
        snap = EnvSnapshot(sd["rows"][lo:lo + self.n], {k: v[lo:lo + self.n] for k, v in sd["outputs"].items()}, self.layout_id,
                           _pool_token(self.pool))
        self._restore_ids(snap, torch.arange(self.n, dtype=torch.int64), True, False)
        if sd.get("reset_window") is not None:
            b, c, st = sd["reset_window"]
            self.set_reset_window(b, c, st if st > 0 else c)       # (stride c: the walk's step 0 mod c, not this batch's n_envs)
        if apply_tune:
            t = dict(sd.get("tune") or {})
            if t.get("coscheduled_envs", self.n) < self.n:
                t.pop("coscheduled_envs")
            self.tune(**t)

    # ------------------------------------------------------------------ views of the state
    def follower_info(self, name):
        """FollowerInfo.scan for every env (SEN:834-842): float32 [n, speed_direction_param] = (follower speed / max_speed,
        direction / 360, then ones) -- two divisions on the state, done with torch on the device."""
        k = dict(self.cfg.follower_info)[name]
        rd = self.state_field("rb_dbl").view(self.n, self.cfg.n_robots, abi.RD_COUNT)[:, 1]
        out = torch.ones(self.n, k, dtype=torch.float32, device=self.device)
        out[:, 0] = (rd[:, abi.RD_SPEED] / self.cfg.c.follower.max_speed).to(torch.float32)
        out[:, 1] = (rd[:, abi.RD_DIRECTION] / 360).to(torch.float32)
        return out

    def state_field(self, name):
        """Typed [n_envs, per_env] view of a named field of the state blob (parity tests / tracker obs)."""
        if name not in self._fields:
            off, per, dt, st = C.c_size_t(), C.c_size_t(), C.c_int32(), C.c_size_t()
            _lib.check(self.lib.ftl_state_field(self.h, name.encode(), C.byref(off), C.byref(per), C.byref(dt), C.byref(st)), self.lib)
            tdt = _DT[dt.value]
            esz = torch.empty((), dtype=tdt).element_size()
            a = self._state_off + off.value
            if per.value == 0:
                self._fields[name] = torch.empty(self.n, 0, dtype=tdt, device=self.device)
            else:      # rows of the per-env record are st bytes apart (a strided view), the long fields are dense
                span = (self.n - 1) * st.value + per.value * esz
                self._fields[name] = torch.as_strided(self.state[a:a + span + (-span) % esz].view(tdt), (self.n, per.value), (st.value // esz, 1))
        return self._fields[name]

    # ------------------------------------------------------------------ rendering (ftl_render): the hook under render()
    def release_render_workspace(self):
        """Free the workspace ``render`` keeps for its last k (the memory returns to torch's caching allocator)."""
        self._render_ws = None

    def _render_ids(self, ids, scale, size, origin, layers, out):
        k = int(ids.numel())
        if k == 0:
            raise ValueError("no env to render")
        rp, (w, h) = _render_params(self.cfg, scale, size, origin, layers)
        out = self._render_out(k, w, h, out)
        ws = getattr(self, "_render_ws", None)
        if ws is None or ws[0] != k:           # the workspace of the last k is kept (a recorder renders the same k again and again)
            nb = C.c_size_t()
            _lib.check(self.lib.ftl_render_workspace(self.h, k, C.byref(nb)), self.lib)
            self._render_ws = None                # (the old buffer goes before the new one is allocated)
            ws = self._render_ws = (k, torch.empty(nb.value, dtype=torch.uint8, device=self.device))
        buf = ws[1]
        buf.record_stream(torch.cuda.current_stream(self.device))     # (freed later: not reused before this call's kernels are done)
        _lib.check(self.lib.ftl_render(self.h, ids.data_ptr(), k, C.byref(rp), buf.data_ptr(), buf.numel(), out.data_ptr(), self._stream()), self.lib)
        self._keep_render = ids
        return out

    def tracker_obs(self, env):
        """(leader_positions_hist, corridor) of one env, as the reference returns them under the tracker key
        (sensors.py:324-325): hist f64[C,2]; corridor f64[C,2(right/left),2]."""
        ei = self.state_field("env_int")[env].cpu().numpy()
        lo, hi = int(ei[abi.EI_CORR_LO]), int(ei[abi.EI_CORR_HI])
        cap = self.cfg.c.corr_cap
        idx = torch.arange(lo, hi, device=self.device) % cap
        corr = self.state_field("corr")[env].view(cap, 2, 2)[idx].cpu().numpy()
        if self.cfg.c.has_tracker == 1:       # v1 tracker (SEN:148-229): float32 history list of its own, corridor never trimmed
            hist = self.state_field("hist1")[env].view(-1, 2)[:int(ei[abi.EI_HIST1_LEN])].cpu().numpy()
        else:
            hist = self.state_field("hist")[env].view(cap, 2)[idx].cpu().numpy()
        return hist, corr


class EnvSnapshot:
    """Saved envs (``VecGame.snapshot``): ``rows`` uint8 ``[k, env_bytes]`` -- the packed state of each env (include/ftl.h, ftl_pack_envs)
    --, ``outputs`` name -> ``[k, ...]`` output rows (obs_num, lasers, target, reward, done, status, and policy_obs / the final buffers
    when the batch has them), ``layout_id`` (``ftl_env_layout_id``) and ``pool_token`` = (uid, version) of the scenario pool.

    A snapshot holds scenario INDICES, not scenarios: it restores only into a batch that runs the same ``ScenarioPool`` object, unwritten
    since (``ScenarioPool.write`` and a moving ``ScenarioRing`` / ``DeviceScenarioRing`` bump its version).  ``cpu()`` / ``to(device)``
    move it; it survives ``torch.save`` / ``torch.load`` (kept with the same pool object in the process, or use ``state_dict``)."""

    def __init__(self, rows, outputs, layout_id, pool_token):
        self.rows, self.outputs, self.layout_id, self.pool_token = rows, dict(outputs), int(layout_id), tuple(pool_token)

    def __len__(self):
        return int(self.rows.shape[0])

    def to(self, device):
        return EnvSnapshot(self.rows.to(device), {k: v.to(device) for k, v in self.outputs.items()}, self.layout_id, self.pool_token)

    def cpu(self):
        return self.to("cpu")


if hasattr(torch.serialization, "add_safe_globals"):       # torch.load(weights_only=True), the default, may rebuild it
    torch.serialization.add_safe_globals([EnvSnapshot])


class EpisodeQueue:
    """A list of Q scenarios to be played exactly once each, and the table of their results, on the device (``ftl_episode_queue``).

    Owns the arrays: ``scenario`` i32[Q], ``stream`` i64[Q] or None (entry q then plays on stream ``stream_base + q``), ``head`` i32[1]
    (the next entry to hand out) and the records.  ``records()`` copies the table to the host (one synchronisation) as a structured numpy
    array of ``abi.RECORD_DTYPE``: state (0 not started, 1 running, 2 finished), scenario, env (the slot that played it), frames, calls,
    status[3], errors, flags (``abi.FTL_EPISODE_DONE_AT_RESET``), ret, stream.  ``table()`` gives the columns as device tensors (views of
    the records, no copy; ``errors`` / ``flags`` as int32 bit patterns); ``finished()`` / ``remaining()`` are device scalars."""

    def __init__(self, scen_ids, stream_ids=None, stream_base=0, device="cuda:0", pool_n=None):
        self.device = torch.device(device)
        scen = torch.as_tensor(scen_ids).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        self.n = int(scen.numel())
        if self.n <= 0:
            raise ValueError("an episode queue needs at least one entry")
        if bool((scen < 0).any()) or (pool_n is not None and bool((scen >= pool_n).any())):
            raise ValueError("scen_ids out of range")
        self.scenario = scen
        self.stream, self.stream_base = None, int(stream_base)
        if stream_ids is not None:
            st = torch.as_tensor(stream_ids).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
            if st.numel() != self.n:
                raise ValueError("stream_ids must have one entry per scenario")
            if bool((st < 0).any()) or bool((st > 2 ** 31 - 1).any()):
                raise ValueError("stream ids must lie in 0 .. 2**31 - 1")
            self.stream = st
        self.head = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._words = C.sizeof(abi.EpisodeRecord) // 8
        self._rec = torch.zeros(self.n, self._words, dtype=torch.int64, device=self.device)

    def c_struct(self, ticket):
        """``abi.EpisodeQueueC`` of this queue for a handle whose slots' tickets live in ``ticket`` (i32[n_envs], device)."""
        c = abi.EpisodeQueueC()
        c.scenario, c.stream = self.scenario.data_ptr(), (self.stream.data_ptr() if self.stream is not None else None)
        c.stream_base, c.n = self.stream_base, self.n
        c.head, c.records, c.ticket = self.head.data_ptr(), self._rec.data_ptr(), ticket.data_ptr()
        return c

    def records(self):
        return self._rec[:self.n].cpu().numpy().view(np.dtype(abi.RECORD_DTYPE)).reshape(self.n)

    def table(self):
        w = self._rec[:self.n].view(torch.int32)          # [Q, 14]
        return dict(state=w[:, 0], scenario=w[:, 1], env=w[:, 2], frames=w[:, 3], calls=w[:, 4], status=w[:, 5:8], errors=w[:, 8],
                    flags=w[:, 9], ret=self._rec[:self.n].view(torch.float64)[:, 5], stream=self._rec[:self.n, 6])

    def finished(self):
        return (self._rec[:self.n].view(torch.int32)[:, 0] == 2).sum()

    def remaining(self):
        return self.n - self.finished()


class ScenarioSampler:
    """Weights over the pool entries ``[base, base + count)`` and the per-scenario outcome table, on the device (``ftl_scenario_sampler``).

    Owns ``weight`` (uint32 bit patterns in an int32 tensor), ``cdf`` (int64, written by the library) and the table int64
    ``[count, abi.FTL_N_SCEN_STATS]``.  Attach it with ``VecGame.set_scenario_sampler`` (or the pipelined batch's: its parts share ONE
    sampler, one table, one cdf); a finished env then draws entry i with probability weight[i] / sum(weight) -- in integers: an entry of
    weight 0 is never drawn; all weights 0 means uniform.  The class builds no curriculum: the caller turns ``table()`` into weights.
    On a CPU device the class only holds and quantises weights (it cannot be attached)."""

    def __init__(self, count, base=0, device="cuda:0"):
        self.device = torch.device(device)
        self.count, self.base = int(count), int(base)
        if self.count <= 0 or self.base < 0:
            raise ValueError("a scenario sampler needs count > 0 and base >= 0")
        self.weight = torch.zeros(self.count, dtype=torch.int32, device=self.device)
        self.cdf = torch.zeros(self.count, dtype=torch.int64, device=self.device)
        self._table = torch.zeros(self.count, abi.FTL_N_SCEN_STATS, dtype=torch.int64, device=self.device)
        self._owner = None

    def c_struct(self):
        c = abi.ScenarioSamplerC()
        c.weight, c.cdf, c.base, c.count, c.table = self.weight.data_ptr(), self.cdf.data_ptr(), self.base, self.count, self._table.data_ptr()
        return c

    def _attach(self, batch):
        self._owner = weakref.ref(batch)

    def _batch(self):
        b = self._owner() if self._owner is not None else None
        return b if b is not None and getattr(b, "sampler", None) is self else None

    @staticmethod
    def quantise(w):
        """int64 weights of a float tensor: ``rint(w / max(w) * 2**24)`` (ties to even), at least 1 where ``w > 0`` -- a positive weight
        is never rounded away; all zero stays all zero (uniform).  Negative or non-finite values raise ValueError."""
        w = torch.as_tensor(w)
        if not w.dtype.is_floating_point:
            w = w.to(torch.float64)
        w = w.double().reshape(-1)
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError("weights must be finite and not negative")
        m = w.max() if w.numel() else w.new_zeros(())
        if float(m) == 0.0:
            return torch.zeros(w.shape, dtype=torch.int64, device=w.device)
        q = torch.round(w / m * float(2 ** 24)).to(torch.int64)
        return torch.where((w > 0) & (q < 1), torch.ones_like(q), q)

    def set_weights(self, w):
        """Weights from a float tensor of length ``count`` (``quantise``); rebuilds the cdf through the batch the sampler is attached to
        -- on a pipelined batch a synchronisation point."""
        w = torch.as_tensor(w)
        if w.numel() != self.count:
            raise ValueError("weights must have one entry per scenario of the window (%d)" % self.count)
        self._store(self.quantise(w))

    def set_raw_weights(self, w):
        """Weights as integers 0 .. 2**32 - 1 (an int64 tensor of length ``count``), taken as they are."""
        w = torch.as_tensor(w)
        if w.dtype.is_floating_point or w.dtype == torch.bool:
            raise ValueError("raw weights must be an integer tensor")
        w = w.to(torch.int64).reshape(-1)
        if w.numel() != self.count:
            raise ValueError("weights must have one entry per scenario of the window (%d)" % self.count)
        if bool((w < 0).any()) or bool((w > 2 ** 32 - 1).any()):
            raise ValueError("raw weights must lie in 0 .. 2**32 - 1")
        self._store(w)

    def _store(self, q):
        q = q.to(self.device)
        self.weight.copy_(torch.where(q >= 2 ** 31, q - 2 ** 32, q).to(torch.int32))     # the uint32 bit pattern
        b = self._batch()
        if b is not None:
            b.refresh_sampler()

    def raw_weights(self):
        """The weights as an int64 tensor of values 0 .. 2**32 - 1."""
        return self.weight.to(torch.int64) & 0xFFFFFFFF

    def table(self, clear=False):
        """The outcome table as a dict of int64 ``[count]`` device tensors (a copy) -- ``abi.SS_NAMES``: episodes, frames_sum, success,
        crash, low_reward, too_far, timeout, return_q16, done_at_reset, last_call (the 1-based ``auto_reset="sample"`` call since the attach
        in which an episode on the scenario last ended; 0: never) -- plus float64 ``mean_return`` (return_q16 / 65536 / episodes) and
        ``success_rate``, both 0 where no episode ended yet.  ``clear=True`` zeroes the table afterwards.  On a pipelined batch the parts
        are joined first."""
        b = self._batch()
        if b is not None:
            b._wait_parts()
        t = self._table.clone()
        if clear:
            self._table.zero_()
        out = {name: t[:, k] for k, name in enumerate(abi.SS_NAMES)}
        ep = t[:, abi.SS_EPISODES].clamp(min=1).double()
        out["mean_return"] = t[:, abi.SS_RETURN_Q16].double() / 65536.0 / ep
        out["success_rate"] = t[:, abi.SS_SUCCESS].double() / ep
        return out

    def state_dict(self):
        """Weights and table as plain CPU tensors (joins the parts of a pipelined batch; synchronises)."""
        b = self._batch()
        if b is not None:
            b._wait_parts()
        return dict(format=1, base=self.base, count=self.count, weight=self.raw_weights().cpu(), table=self._table.cpu())

    def load_state_dict(self, sd):
        if sd.get("format") != 1 or int(sd["count"]) != self.count or int(sd["base"]) != self.base:
            raise ValueError("the checkpoint is of a sampler over another window")
        b = self._batch()
        if b is not None:
            b._wait_parts()
        self._table.copy_(sd["table"].to(self.device))
        self.set_raw_weights(sd["weight"])


def _refuse_with_queue(queue, what):
    if queue is not None:
        raise _lib.FtlError("%s with an episode queue attached: a half-drained queue cannot be saved -- drain it (evaluate) or detach it "
                            "(set_episode_queue(None)) first" % what)


def _evaluate_loop(cfg, n, q, obs, step, policy, check_every, max_calls):
    """The loop of ``evaluate``: ``obs()`` -> the observation tuple on the current stream, ``step(action)`` one queue step."""
    check_every = max(int(check_every), 1)
    c = cfg.c
    least = c.rand_fps_lo if c.rand_fps_hi > 0 else c.frames_per_step
    if max_calls is None:
        max_calls = -(-q.n // n) * (c.max_steps // least + 2) + check_every
    calls = 0
    while True:
        step(policy(obs()))
        calls += 1
        if calls % check_every == 0 or calls >= max_calls:
            if int(q.finished()) == q.n:
                return calls
            if calls >= max_calls:
                raise _lib.FtlError("evaluate: %d of %d episodes finished after max_calls = %d calls" % (int(q.finished()), q.n, max_calls))


def _pool_token(pool):
    return (pool.uid, int(pool.version))


def _host_ids(env_ids, n):
    """int64 host tensor of env indices in [0, n) (None: all)."""
    if env_ids is None:
        return torch.arange(n, dtype=torch.int64)
    a = torch.as_tensor(env_ids.detach().cpu() if isinstance(env_ids, torch.Tensor) else np.asarray(env_ids)).reshape(-1)
    if a.dtype.is_floating_point or a.dtype == torch.bool:
        raise ValueError("env ids must be integers")
    a = a.to(torch.int64)
    if a.numel() and (int(a.min()) < 0 or int(a.max()) >= n):
        raise ValueError("env ids outside [0, %d)" % n)
    return a


_SHOW_FLAGS = (("show_leader_path_flag", abi.RENDER_PATH), ("show_box_flag", abi.RENDER_BOX), ("show_objects_flag", abi.RENDER_OBJECTS),
               ("show_rectangles_flag", abi.RENDER_RECTS), ("show_sensors_flag", abi.RENDER_SENSORS))


def _render_layers(cfg):
    bits = abi.RENDER_TARGET
    for key, bit in _SHOW_FLAGS:
        if cfg.kwargs.get(key, True):
            bits |= bit
    return bits


def _render_ids(env_ids, n, device):
    """int32 device tensor of env indices; ids given on the host are range-checked here (device ids out of range give white frames)."""
    if env_ids is None:
        return torch.arange(n, dtype=torch.int32, device=device)
    if isinstance(env_ids, torch.Tensor) and env_ids.device.type == "cuda":
        return env_ids.to(device=device, dtype=torch.int32).reshape(-1).contiguous()
    a = np.asarray(env_ids.cpu() if isinstance(env_ids, torch.Tensor) else env_ids, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() >= n):
        raise ValueError("env_ids outside [0, %d)" % n)
    return torch.from_numpy(a.astype(np.int32)).to(device)


def _render_params(cfg, scale, size, origin, layers):
    scale = float(scale)
    if not scale > 0 or not math.isfinite(scale):
        raise ValueError("scale must be positive")
    if size is None:
        size = (int(math.ceil(cfg.c.width / scale)), int(math.ceil(cfg.c.height / scale)))
    w, h = int(size[0]), int(size[1])
    rp = abi.RenderParams()
    rp.width, rp.height, rp.scale = w, h, scale
    rp.origin_x, rp.origin_y = float(origin[0]), float(origin[1])
    rp.layers = _render_layers(cfg) if layers is None else int(layers)
    return rp, (w, h)


def _split_ids(ids, shards, games):
    """Split env indices of a whole batch (int64 host tensor, any order, repeats allowed) over its parts: for every part that owns some
    of them ``(game, positions in ids, the part's own indices of those envs)``.  A new per-ids operation is one loop over this."""
    for g, sh in zip(games, shards):
        pos = torch.nonzero((ids >= sh.lo) & (ids < sh.hi)).reshape(-1)
        if pos.numel():
            yield g, pos, ids[pos] - sh.lo


class PipelinedVecGame(_BatchBase):
    """A batch of N envs stepped as ``parts`` independent sub-batches, each on its own HIP stream of this process.

    Envs never interact, so part k's step t+1 depends on nothing but part k's step t.  Run that way -- no join between the parts --
    one part's ray kernel (VALU-bound, 80 registers a lane) runs beside another part's frame kernel (latency-bound, half the VALU idle),
    and the last, thinly occupied wavefronts of either are covered by the other stream's work: 250 M env-steps/s against 215 M for the
    same 65,536 envs of config B as one batch on one stream.  Every env sees exactly the arithmetic of ``VecGame``:
    the parts are ``VecGame`` batches over consecutive env ranges, their per-env random streams keyed by the GLOBAL env index and
    their auto-reset walking the scenario pool with the whole batch's stride, so results are bit-identical to one ``VecGame(N)``
    (tests/test_gpu_api.py).

    ``step(action)`` enqueues every part on its stream and returns the combined output tensors WITHOUT waiting: part k's rows are valid
    on ``stream(k)``; ``join()`` makes the current stream wait for all parts.  A caller that joins after every step re-aligns the parts
    and gets ``VecGame``'s throughput back; a training loop keeps them apart by consuming part k's rows (``rows(k)``) on ``stream(k)``
    and feeding ``step_part(k, action_k)`` -- the double-buffered sampling loop of asynchronous RL frameworks."""

    def __init__(self, n_envs, parts=2, device="cuda:0", config: GameConfig = None, policy_obs=False, final_obs=False, **game_kwargs):
        cfg = config if config is not None else make_config(**game_kwargs)
        self.cfg, self.n, self.device = cfg, int(n_envs), torch.device(device)
        if parts < 1 or parts > self.n:
            raise ValueError("parts must be in 1..n_envs")
        # ONE set of output tensors; the parts write their row ranges
        outs = {name: torch.zeros(self.n, *shape, dtype=dtype, device=self.device)
                for name, (shape, dtype) in _output_table(cfg, policy_obs, final_obs).items()}
        self.shards = [shard_range(self.n, k, parts) for k in range(parts)]
        self.games, self.streams = [], []
        for sh in self.shards:
            ck = dataclasses.replace(cfg, c=abi.Config.from_buffer_copy(cfg.c))
            ck.c.env_id_base = cfg.c.env_id_base + sh.lo          # per-env random streams are keyed by the global env index
            g = VecGame(sh.n, device=self.device, config=ck, policy_obs=policy_obs, _outputs={k: v[sh.lo:sh.hi] for k, v in outs.items()},
                        final_obs=final_obs)
            if parts > 1:
                # the parts take the role of the handle's own two-stream mode (random_frames_per_step), without its join; the envs are sorted
                # by cost when the WHOLE batch oversubscribes the device, on a staler order than a lone handle's (259 against 255 M env-steps/s)
                g.tune(two_streams=0, coscheduled_envs=self.n, regroup_every=8)
            self.games.append(g)
            self.streams.append(torch.cuda.Stream(device=self.device))
        self._set_outputs(outs, final_obs)
        self.pool = None
        self.queue = None
        self.sampler = None
        self._serial = False
        self._metrics = torch.zeros(abi.FTL_N_METRICS, dtype=torch.float64, device=self.device)
        self._stream_ptrs = [C.c_void_p(s.cuda_stream) for s in self.streams]
        self._ev = torch.cuda.Event()

    parts = property(lambda self: len(self.games))
    layout_id = property(lambda self: self.games[0].layout_id)
    env_bytes = property(lambda self: self.games[0].env_bytes)
    _window = property(lambda self: self.games[0]._window)
    _tune = property(lambda self: {})          # (a checkpoint of the whole batch carries no hints: the parts keep their own)

    def close(self):
        for g in self.games:
            g.close()

    def stream(self, k):
        return self.streams[k]

    def rows(self, k):
        """(lo, hi) of part k's envs in the combined tensors."""
        return self.shards[k].lo, self.shards[k].hi

    def _on(self, k):
        """Context: part k's stream, after everything the current stream has been given so far (the action tensor's producer)."""
        cur = torch.cuda.current_stream(self.device)
        if self._serial:
            return torch.cuda.stream(cur)
        self.streams[k].wait_stream(cur)
        return torch.cuda.stream(self.streams[k])

    def join(self):
        """The current stream waits for every part (outputs of all rows valid on it afterwards)."""
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            cur.wait_stream(s)

    _wait_parts = join

    def load_scenarios(self, pool: ScenarioPool):
        self.pool = pool
        for g in self.games:
            g.load_scenarios(pool)
            g.set_reset_window(0, pool.n, self.n)      # the auto-reset walks the pool with the WHOLE batch's stride, as VecGame(n) does

    def set_reset_window(self, base, count, stride=0):
        """``VecGame.set_reset_window`` for every part; ``stride`` 0 keeps the whole batch's n_envs."""
        for g in self.games:
            g.set_reset_window(base, count, stride if stride > 0 else self.n)

    def state_field(self, name):
        """[n_envs, per_env] COPY of a named state field over all parts (``VecGame.state_field`` gives views, part by part)."""
        self.join()
        return torch.cat([g.state_field(name) for g in self.games], 0)

    def _reset_parts(self, reset):
        """``reset(game, shard)`` of every part on its stream, then ``join()``; returns the first observations like ``reset``."""
        for k, (g, sh) in enumerate(zip(self.games, self.shards)):
            with self._on(k):
                reset(g, sh)
        self.join()
        return self.obs_num, self.lasers

    def reset(self, scen_idx=None, mask=None):
        scen_idx, mask = self._reset_args(scen_idx, mask)
        return self._reset_parts(lambda g, sh: g.reset(scen_idx[sh.lo:sh.hi], None if mask is None else mask[sh.lo:sh.hi]))

    def step_part(self, k, action, auto_reset=False, sensors=True):
        """One step of part k on its stream; ``action`` = the rows of part k (any layout ``VecGame.step`` takes); ``auto_reset`` and
        ``sensors`` as ``VecGame.step`` (the final buffers' rows of part k are valid on ``stream(k)``)."""
        with self._on(k):
            self.games[k].step(action, auto_reset=auto_reset, sensors=sensors)
            if not self._serial:
                action.record_stream(self.streams[k])

    def step(self, action, auto_reset=False, sensors=True):
        """One step of every part (``action``: the whole batch's tensor, rows in env order; ``auto_reset`` and ``sensors`` as
        ``VecGame.step``).  Does not join -- see the class text.
        The part streams wait for what the current stream has been given so far (the producer of ``action``); nothing waits for them."""
        g0 = self.games[0]
        action, enc = g0._encode_action(action, self.n)            # checked / decoded once for the whole batch, then handed over by row range
        self._keep_action = action
        modes = [g._step_mode(auto_reset) for g in self.games]      # (validated before anything is enqueued)
        blind = 0 if sensors else abi.FTL_STEP_NO_SENSORS
        base, row = action.data_ptr(), action.element_size() * (2 if enc == abi.FTL_ACTION_BOX2 else 1)
        for g, sh, sptr, (flags, fin) in zip(self.games, self.shards, self._part_streams(action), modes):
            g._step_final(base + sh.lo * row, enc, flags | blind, fin, sptr)
        return self.obs_num, self.lasers, self.reward, self.done, self.status

    def _part_streams(self, action=None):
        """The ``c_void_p`` stream of every part for one call over the whole batch: the parts' own streams, each made to wait for what
        the current stream has been given so far and told about ``action`` -- or, while ``kernel_timing`` is on, the current stream."""
        cur = torch.cuda.current_stream(self.device)
        if self._serial:
            return [C.c_void_p(cur.cuda_stream)] * len(self.games)
        self._ev.record(cur)
        for stream in self.streams:
            stream.wait_event(self._ev)
            if action is not None:
                action.record_stream(stream)       # (the caller may drop the tensor right away: its memory must outlive the part's read)
        return self._stream_ptrs

    def scan(self):
        """``VecGame.scan`` of every part on its stream; does not join, like ``step`` (part k's rows of ``lasers`` / ``policy_obs`` are
        valid on ``stream(k)``)."""
        self._need_pool()
        for g, sptr in zip(self.games, self._part_streams()):
            g._scan(sptr)
        return self.lasers

    def rollout(self, actions, gamma=1.0, sensors=True):
        """``VecGame.rollout`` of every part on its stream (``actions``: the whole batch's ``[T, N, ...]`` tensor; every part reads its
        rows of it); returns the whole batch's ``(ret, steps, status)``.  Does not join, like ``step``."""
        self._need_pool()
        flat, enc, T = self.games[0]._encode_rollout(actions, self.n)
        self._keep_action = flat
        self._prepare_rollout_outputs()
        base, row = flat.data_ptr(), flat.element_size() * (2 if enc == abi.FTL_ACTION_BOX2 else 1)
        for g, sh, sptr in zip(self.games, self.shards, self._part_streams(flat)):
            g._rollout(base + sh.lo * row, self.n * row, enc, T, gamma, sensors, sptr)
        return self.rollout_ret, self.rollout_steps, self.rollout_status

    def _prepare_rollout_outputs(self):
        """The whole batch's ``rollout_ret`` / ``_steps`` / ``_status``, allocated on first use; every part takes its rows."""
        if getattr(self, "rollout_ret", None) is None:
            dev = self.device
            self.rollout_ret, self.rollout_steps, self.rollout_status = (torch.zeros(self.n, dtype=torch.float64, device=dev), torch.zeros(
                self.n, dtype=torch.int32, device=dev), torch.zeros(self.n, 3, dtype=torch.uint8, device=dev))
            for g, sh in zip(self.games, self.shards):
                g._rollout_outputs((self.rollout_ret[sh.lo:sh.hi], self.rollout_steps[sh.lo:sh.hi], self.rollout_status[sh.lo:sh.hi]))

    def set_episode_queue(self, scen_ids, stream_ids=None, stream_base=0):
        """``VecGame.set_episode_queue`` for the whole batch: the parts share ONE queue -- one head, one table -- so every entry is still
        played exactly once and its record is the same as on one ``VecGame``; which part plays what depends on timing."""
        if scen_ids is None:
            for g in self.games:
                g.set_episode_queue(None)
            self.queue = None
            return None
        self._need_pool()
        q = scen_ids if isinstance(scen_ids, EpisodeQueue) else EpisodeQueue(scen_ids, stream_ids, stream_base, self.device, self.pool.n)
        self.join()
        for g in self.games:
            g.set_episode_queue(q)
        self.queue = q
        return q

    ticket = property(lambda self: torch.cat([g.ticket for g in self.games]) if self.queue is not None else None)

    def reset_from_queue(self):
        """``VecGame.reset_from_queue`` of every part on its stream, then ``join()``."""
        self._need_queue()
        return self._reset_parts(lambda g, sh: g.reset_from_queue())

    def set_scenario_sampler(self, sampler):
        """``VecGame.set_scenario_sampler`` for the whole batch: the parts share ONE sampler -- one table, one cdf -- and, their draws being
        pure functions of each env's own words, play exactly what one ``VecGame`` plays.  Joins the parts."""
        self.join()
        if sampler is None:
            for g in self.games:
                g.set_scenario_sampler(None)
            self.sampler = None
            return None
        self._check_sampler(sampler)
        for g in self.games:
            g.set_scenario_sampler(sampler, _owner=self)
        self.sampler = sampler
        sampler._attach(self)
        self.refresh_sampler()
        return sampler

    def refresh_sampler(self):
        """Rebuild the shared cdf once, on the current stream.  A synchronisation point like ``load_scenarios`` on a running batch: the
        current stream first waits for every part (their steps in flight read the old cdf), and the parts' next steps wait for it."""
        self._need_sampler()
        self.join()
        self.games[0].refresh_sampler()

    def reset_from_sampler(self):
        """``VecGame.reset_from_sampler`` of every part on its stream, then ``join()``."""
        self._need_sampler()
        return self._reset_parts(lambda g, sh: g.reset_from_sampler())

    def episode_metrics(self, clear=False):
        self.join()
        self._metrics.zero_()
        for g in self.games:
            self._metrics += g.episode_metrics(clear)
        return self._metrics

    def error_report(self):
        self.join()
        n, bits = 0, 0
        for g in self.games:
            a, b = g.error_report()
            n, bits = n + a, bits | b
        return n, bits

    def raise_on_errors(self, live=False):
        """``VecGame.raise_on_errors`` over all parts (joins first)."""
        self.join()
        for g in self.games:
            g.raise_on_errors(live)

    def release_render_workspace(self):
        for g in self.games:
            g.release_render_workspace()

    # the per-ids operations over global env indices: one pass of _split_ids each, the parts' results scattered back by position
    def _render_ids(self, ids, scale, size, origin, layers, out):
        ids = ids.cpu().long()
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.n):
            raise ValueError("env_ids outside [0, %d)" % self.n)
        _, (w, h) = _render_params(self.cfg, scale, size, origin, layers)
        k = int(ids.numel())
        out = self._render_out(k, w, h, out)
        for g, pos, local in _split_ids(ids, self.shards, self.games):
            local = local.to(device=self.device, dtype=torch.int32)
            if pos.numel() == k:               # every id in this part: straight into out
                g._render_ids(local, scale, size, origin, layers, out)
            else:
                out.index_copy_(0, pos.to(self.device), g._render_ids(local, scale, size, origin, layers, None))
        return out

    def _snapshot_ids(self, ids):
        k = int(ids.numel())
        rows = torch.empty(k, self.env_bytes, dtype=torch.uint8, device=self.device)
        outs = {name: torch.empty((k,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device) for name, t in self.output_rows().items()}
        for g, pos, local in _split_ids(ids, self.shards, self.games):
            part, dpos = g._snapshot_ids(local), pos.to(self.device)
            rows.index_copy_(0, dpos, part.rows)
            for name, t in outs.items():
                t.index_copy_(0, dpos, part.outputs[name])
        return EnvSnapshot(rows, outs, self.layout_id, _pool_token(self.pool))

    def _restore_ids(self, snap, ids, slot_stats, own_stream):
        for g, pos, local in _split_ids(ids, self.shards, self.games):
            sub = EnvSnapshot(snap.rows.index_select(0, pos.to(snap.rows.device)),
                              {k: v.index_select(0, pos.to(v.device)) for k, v in snap.outputs.items()}, snap.layout_id, snap.pool_token)
            g._restore_ids(sub, local, slot_stats, own_stream)

    def load_state_dict(self, sd):
        """``VecGame.load_state_dict`` for every part (each takes the rows of its global env ids); the parts keep their own scheduling
        hints.  Joins the parts first."""
        self.join()
        self._need_pool()
        digest = self.pool.digest()
        for g in self.games:                    # (every part checks the checkpoint before the first one writes: same layout, same range)
            lo = int(g.cfg.c.env_id_base) - int(sd["env_id_base"])
            if int(sd["layout_id"]) != g.layout_id or lo < 0 or lo + g.n > int(sd["n_envs"]):
                raise ValueError("the checkpoint does not cover this batch's envs with the same layout")
        for g in self.games:
            g.load_state_dict(sd, apply_tune=False, _digest=digest)

    def kernel_timing(self, enable=True):
        """Measurement hook.  While enabled the parts run one after the other on the CURRENT stream, so that every kernel's HIP events
        time that kernel alone (``kernel_times``: averages per LAUNCH, i.e. per part)."""
        self.join()
        torch.cuda.current_stream(self.device).synchronize()
        self._serial = bool(enable)
        for g in self.games:
            g.kernel_timing(enable)

    def kernel_times(self):
        ts = [g.kernel_times() for g in self.games]
        out = {k: sum(t[k] for t in ts) / len(ts) for k in ("frames_us", "rays_us", "aux_us", "regroup_us")}
        out["steps"] = ts[0]["steps"]
        out["launches_per_step"] = len(ts)
        return out
