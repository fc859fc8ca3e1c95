"""numpy twin of the PPO loss head (include/ftl.h, the ftl_ppo_head block): the row arithmetic line by line with float32 scalars
(``mlp_numpy.fmaf32``, ``rnn_numpy.exp32``), the segment reductions lane by lane in float64, the per-set scalars and the stats table.
Everything the device computes is pinned to this bit for bit.  ``exact=True`` is NOT the contract: the same formulas in float64
throughout with ``np.exp``, for the comparison with torch's float64 autograd."""
import numpy as np

import mlp_numpy as M
import rnn_numpy as R
from continiousenvironment_follower_leader_amd import abi

F = np.float32
SEG, STATS, VOID = abi.FTL_PPO_SEG, abi.FTL_PPO_STATS, abi.FTL_TR_VOID


def rows(head_new, head_old, noise, sigma_old, sigma_new, shift, adv, ret, value, mean32, inv32, invc, clip_lo, clip_hi, vf_coef,
         normalize, exact=False):
    """The row lines on R rows at once: ``head_new`` / ``head_old`` / ``noise`` / ``sigma_*`` / ``shift`` are ``[R, A]`` (the set's values
    repeated per row), ``adv`` / ``ret`` / ``value`` (or None) / ``mean32`` / ``inv32`` / ``invc`` ``[R]``.  Returns a dict of the row's
    outputs and of the values the reductions sum."""
    T = np.float64 if exact else F
    c = lambda v: np.asarray(v, T)
    fma = (lambda a, b, d: c(a) * c(b) + c(d)) if exact else M.fmaf32
    if exact:
        ratio = lambda d: np.exp(d)
    else:
        def ratio(d):
            neg = R.exp32(np.where(d <= 0, d, F(0.0)))
            pos = (F(1.0) / R.exp32(np.where(d > 0, -d, F(0.0)))).astype(F)
            return np.where(d != d, d, np.where(d <= 0, neg, pos)).astype(F)
    head_new, head_old, noise, sigma_old, sigma_new, shift = (c(v) for v in (head_new, head_old, noise, sigma_old, sigma_new, shift))
    A = head_new.shape[1]
    with np.errstate(all="ignore"):
        e = head_old - head_new
        t = fma(sigma_old, noise, e)
        u = (t / sigma_new).astype(T)
        p = u * u
        q = noise * noise
        w = q - p
        l = fma(T(0.5), w, -shift)
        d = l[:, 0] if A == 1 else l[:, 0] + l[:, 1]
        r = ratio(d)
        a = c(adv)
        if normalize:
            am = a - c(mean32)
            a = am * c(inv32)
        s1 = r * a
        rc = np.fmin(np.fmax(r, T(clip_lo)), T(clip_hi))
        s2 = rc * a
        active = ~(s2 < s1)
        g = np.where(active, -(s1 * c(invc)), T(0.0)).astype(T)
        us = (u / sigma_new).astype(T)
        dhead = g[:, None] * us
        pm = p - T(1.0)
        k = g[:, None] * pm
        out = dict(d=d, ratio=r, a=a, s1=s1, s2=s2, active=active, dhead=dhead.astype(T), k=k.astype(T),
                   pl=(-np.where(active, s1, s2)).astype(T), nd=(-d).astype(T), clipped=(r < T(clip_lo)) | (r > T(clip_hi)))
        if value is None:
            out["dvalue"], out["vl"] = None, np.zeros_like(d)
        else:
            hv = c(value) - c(ret)
            vh = T(vf_coef) * hv
            out["dvalue"] = (vh * c(invc)).astype(T)
            hh = hv * hv
            out["vl"] = (T(0.5) * hh).astype(T)
    return out


def segment_sum(x, valid):
    """A segment's partial of ``x`` (float64 ``[len]``, len <= SEG): lane k of 64 sums offsets k mod 64 ascending from +0.0 and skips the
    rows that are not ``valid``; then x[k] += x[k + stride] for stride 32 .. 1."""
    n = x.shape[0]
    assert 1 <= n <= SEG
    pad = (-n) % 64
    xs = np.concatenate([np.asarray(x, np.float64), np.zeros(pad)]).reshape(-1, 64)
    vs = np.concatenate([np.asarray(valid, bool), np.zeros(pad, bool)]).reshape(-1, 64)
    lanes = np.zeros(64)
    with np.errstate(all="ignore"):
        for xi, vi in zip(xs, vs):
            lanes = np.where(vi, lanes + xi, lanes)
        stride = 32
        while stride >= 1:
            lanes[:stride] = lanes[:stride] + lanes[stride:2 * stride]
            stride //= 2
    return lanes[0]


def segments(n, n_sets):
    """(rows of a set in a block, segments of such a slice)."""
    rows_ = n // n_sets
    return rows_, -(-rows_ // SEG)


def set_totals(x, valid, n_sets):
    """float64 ``[n_sets]``: per set the sum from +0.0 of the segment partials of ``x`` ``[B, n]`` in ascending (block, segment) order."""
    B, n = x.shape
    m, sps = segments(n, n_sets)
    tot = np.zeros(n_sets)
    with np.errstate(all="ignore"):
        for s in range(n_sets):
            for b in range(B):
                for g in range(sps):
                    lo = s * m + g * SEG
                    hi = min(lo + SEG, (s + 1) * m)
                    tot[s] = tot[s] + segment_sum(x[b, lo:hi], valid[b, lo:hi])
    return tot


def moments(cnt, S1, S2, exact=False):
    """The per-set scalars (float64 arrays ``[n_sets]``): mean, std, mean32, inv32, invc."""
    with np.errstate(all="ignore"):
        some = cnt > 0
        mean = np.where(some, S1 / np.where(some, cnt, 1.0), 0.0)
        q = (S2 - S1 * mean) / np.where(cnt >= 2, cnt - 1.0, 1.0)
        var = np.where(cnt >= 2, np.where(q < 0, 0.0, q), 0.0)
        std = np.sqrt(var)
        inv = 1.0 / (std + 1e-8)
        invc = np.where(some, 1.0 / np.where(some, cnt, 1.0), 0.0)
    T = np.float64 if exact else F
    return mean, std, mean.astype(T), inv.astype(T), invc.astype(T)


def head(head_new, head_old, noise, sigma_old, sigma_new, adv, ret, kind, value=None, shift=None, clip_lo=F(0.8), clip_hi=F(1.2),
         vf_coef=0.5, normalize=True, exact=False):
    """``ftl_ppo_head`` on ``[B, n, A]`` heads, ``[n_sets, A]`` sigmas, ``[B, n]`` adv / ret / kind / value: a dict of ``dhead`` ``[B, n, A]``,
    ``dvalue`` ``[B, n]`` (or None), ``dlog_std`` ``[n_sets, A]``, ``stats`` float64 ``[n_sets, STATS]`` and ``ratio`` ``[B, n]``."""
    T = np.float64 if exact else F
    B, n, A = head_new.shape
    n_sets = sigma_new.shape[0]
    assert n % n_sets == 0 and A in (1, 2)
    m, _ = segments(n, n_sets)
    valid = np.asarray(kind) != VOID
    a64 = np.asarray(adv, F).astype(np.float64) if not exact else np.asarray(adv, np.float64)
    ones = np.ones((B, n))
    cnt, S1, S2 = set_totals(ones, valid, n_sets), set_totals(a64, valid, n_sets), set_totals(a64 * a64, valid, n_sets)
    mean, std, mean32, inv32, invc = moments(cnt, S1, S2, exact)
    per_row = lambda v: np.broadcast_to(np.repeat(np.asarray(v), m, axis=0)[None], (B,) + (n,) + np.asarray(v).shape[1:]).reshape((B * n,) + np.asarray(v).shape[1:])
    shift = np.zeros((n_sets, A), T) if shift is None else shift
    o = rows(head_new.reshape(B * n, A), head_old.reshape(B * n, A), noise.reshape(B * n, A), per_row(sigma_old), per_row(sigma_new),
             per_row(shift), adv.reshape(-1), ret.reshape(-1), None if value is None else value.reshape(-1), per_row(mean32), per_row(inv32),
             per_row(invc), clip_lo, clip_hi, vf_coef, normalize, exact)
    flat = valid.reshape(-1)
    dhead = np.where(flat[:, None], o["dhead"], T(0.0)).astype(T).reshape(B, n, A)
    dvalue = None if value is None else np.where(flat, o["dvalue"], T(0.0)).astype(T).reshape(B, n)
    tot = lambda v: set_totals(np.asarray(v, np.float64).reshape(B, n), valid, n_sets)
    t_pl, t_vl, t_nd, t_cl = tot(o["pl"]), tot(o["vl"]), tot(o["nd"]), tot(o["clipped"].astype(np.float64))
    t_k = np.stack([tot(o["k"][:, j]) for j in range(A)], 1)
    stats = np.zeros((n_sets, STATS))
    with np.errstate(all="ignore"):
        some = cnt > 0
        div = lambda t: np.where(some, t / np.where(some, cnt, 1.0), 0.0)
        stats[:, 0], stats[:, 1], stats[:, 2] = cnt, mean, std
        stats[:, 3], stats[:, 5], stats[:, 6] = div(t_pl), div(t_nd), div(t_cl)
        stats[:, 4] = div(t_vl) if value is not None else 0.0
        stats[:, 7] = stats[:, 3] + np.float64(F(vf_coef) if not exact else vf_coef) * stats[:, 4]
    return dict(dhead=dhead, dvalue=dvalue, dlog_std=t_k.astype(T), stats=stats, ratio=o["ratio"].reshape(B, n), rows=o, valid=valid)


def workspace_bytes(B, n, n_sets):
    _, sps = segments(n, n_sets)
    return B * n_sets * sps * 72 + n_sets * 16


def crafted(A, sigma=0.37):
    """Rows at the edges of the row arithmetic, for one set with ``sigma_new == sigma_old == sigma`` and no shift, to be run with
    ``normalize=False`` so that ``a`` is ``adv``: a dict of ``head_new`` / ``head_old`` / ``noise`` ``[R, A]`` and ``adv`` / ``ret`` /
    ``value`` ``[R]``.  Rows 0 and 1 have ratios below and above 1 whose values serve as ``clip_lo`` and ``clip_hi`` (r exactly at the
    bounds); rows 2 .. 5 are the four combinations of the sign of ``a`` and the side of ``r``; 6 has ``a = 0``; 7 .. 9 have d > 0,
    d > 86 and d < -86; 10 and 11 have ``head_new == head_old`` (ratio within rounding of 1), 11 with a negative advantage."""
    s = F(sigma)
    # (noise_0, (head_old - head_new)_0 in units of sigma, adv)
    spec = [(0.5, 0.3, 1.0), (0.9, -0.5, 1.0),                 # r = exp(0.5 (0.25 - 0.64)) ~ 0.82; exp(0.5 (0.81 - 0.16)) ~ 1.38
            (1.5, -1.4, 2.0), (0.2, 1.5, 2.0), (1.5, -1.4, -2.0), (0.2, 1.5, -2.0),
            (0.7, 0.4, 0.0),
            (1.0, -0.5, 0.5), (14.0, -14.0, 0.25), (0.0, 14.0, -0.25),
            (0.8, 0.0, 1.5), (-1.3, 0.0, -1.5)]
    R_ = len(spec)
    noise, head_old, head_new = np.zeros((R_, A), F), np.zeros((R_, A), F), np.zeros((R_, A), F)
    adv = np.array([v[2] for v in spec], F)
    for i, (z, e, _) in enumerate(spec):
        noise[i, 0] = F(z)
        head_old[i, :] = F(0.25) + F(0.125) * F(i)
        head_new[i, :] = head_old[i, :]
        head_new[i, 0] = head_old[i, 0] - F(e) * s
        if A == 2:
            noise[i, 1] = F(0.1) * F(i % 3)
    ret = np.linspace(-1.0, 1.0, R_).astype(F)
    value = (ret + np.linspace(0.5, -0.5, R_).astype(F)).astype(F)
    return dict(head_new=head_new, head_old=head_old, noise=noise, adv=adv, ret=ret, value=value, sigma=np.full((1, A), s, F))
