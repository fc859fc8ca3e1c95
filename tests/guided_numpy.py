"""numpy twin of the guided search's own arithmetic (include/ftl.h: ftl_baseline_act_guided, ftl_search_guided): the clip-add-clip of the
guided action, the residual box, and one guided decision of one env on the host follower of tests/baseline_numpy.py.  Float64, the header's
operation order, one rounding per operation.  Shared by tests/test_guided_abi.py and tests/test_gpu_guided.py."""
import numpy as np

import baseline_numpy
import search_numpy


def box(cfg):
    """(lo, hi) of the Box(2) action space: that of the action search."""
    return search_numpy.box(cfg)


def residual_box(cfg):
    """(lo, hi) of the residuals: the box of the action Box's width centred on 0."""
    lo, hi = box(cfg)
    half = (hi - lo) / 2.0
    return -half, half


def guided_action(base, resid, lo, hi):
    """fmin(fmax(fmin(fmax(base, lo), hi) + resid, lo), hi) element by element on float64 arrays."""
    base, resid = np.asarray(base, dtype=np.float64), np.asarray(resid, dtype=np.float64)
    return np.fmin(np.fmax(np.fmin(np.fmax(base, lo), hi) + resid, lo), hi)


def act(follower, num, target, step_count, resid, lo, hi):
    """One guided decision of ``follower`` (a ``baseline_numpy.Follower``): its bookkeeping and raw action, then the guided action."""
    v, w = follower.act(num, target, step_count)
    return guided_action(np.array([v, w]), resid, lo, hi)


def sample(nominal, streams, seed, call, it, K, hold, s, cfg):
    """The residual candidates of a round: ``search_numpy.sample`` on the residual box."""
    lo, hi = residual_box(cfg)
    return search_numpy.sample(nominal, streams, seed, call, it, K, hold, s, lo, hi)


def begin(step_count, nominal, call, warm):
    """The residual plan a call starts from: ``search_numpy.begin`` with the default (0, 0)."""
    return search_numpy.begin(step_count, nominal, call, warm, 0.0)


def follower_from_row(row, cap):
    """A ``baseline_numpy.Follower`` holding what the uint8 device row ``row`` (16 + 16 * cap bytes) holds."""
    row = np.ascontiguousarray(row)
    head, count, pending, flags = (int(x) for x in row[:16].view(np.int32))
    pts = row[16:].view(np.float64).reshape(cap, 2)
    f = baseline_numpy.Follower(cap)
    f.fifo = [(float(pts[(head + i) % cap, 0]), float(pts[(head + i) % cap, 1])) for i in range(count)]
    f.pending, f.flags = bool(pending), flags
    return f
