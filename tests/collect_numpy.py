"""numpy twin of the trajectory collection (include/ftl.h: ftl_mlp_sample, ftl_collect_mlp's kinds, ftl_gae): the sampling heads on top of
``mlp_numpy`` (which stays as it is) and the advantage recursion as a plain loop over t.  Every float64 operation is written on its own
line, as the contract counts its roundings."""
import numpy as np

import mlp_numpy as M

STEP, TERMINATED, TRUNCATED, VOID = 0, 1, 2, 3


def box_sample(y, sigma, noise, lo, hi):
    """float64: the Box head of ``y`` (float32) with ``z = y + sigma * noise``; the product of two float32 is exact in float64."""
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(all="ignore"):
        p = np.asarray(sigma, np.float32).astype(np.float64) * np.asarray(noise, np.float32).astype(np.float64)
        z = np.asarray(y, np.float32).astype(np.float64) + p
        u = np.fmin(np.fmax(z, -1.0), 1.0)
        s = (u + 1.0) * 0.5
        a = lo + s * (hi - lo)
        return np.fmin(np.fmax(a, lo), hi)


def discrete_sample(y, noise):
    """int32: the first maximum of ``s = y + noise`` in float64; a NaN never beats anything."""
    with np.errstate(all="ignore"):
        s = np.asarray(y, np.float32).astype(np.float64) + np.asarray(noise, np.float32).astype(np.float64)
        k = np.zeros(s.shape[0], np.int32)
        rows = np.arange(s.shape[0])
        for j in range(1, 5):
            k = np.where(s[:, j] > s[rows, k], np.int32(j), k).astype(np.int32)
    return k


def sample_head(y, head, lo, hi, noise=None, sigma=None):
    """The encoded action of head outputs ``y`` [n, w] with ``noise`` [n, w] and ``sigma`` [n, w] (each env's own row); ``noise`` None is
    ``mlp_numpy.head_of``."""
    if noise is None:
        return M.head_of(y, head, lo, hi)
    if head == M.DISCRETE:
        return discrete_sample(y, noise)
    if head == M.BOX2:
        return np.stack([box_sample(y[:, j], sigma[:, j], noise[:, j], lo[j], hi[j]) for j in range(2)], 1)
    return box_sample(y[:, 0], sigma[:, 0], noise[:, 0], lo[-1], hi[-1])


def sample_population(params, widths, x, head, lo, hi, envs_per_set, noise=None, sigma=None, env_first=0):
    """(action, raw head [n, w] float32) of a population: row e of ``x`` under set (env_first + e) // envs_per_set, ``sigma`` [n_sets, w]."""
    sets = (env_first + np.arange(x.shape[0])) // envs_per_set
    y = np.zeros((x.shape[0], widths[-1]), np.float32)
    for s in np.unique(sets):
        y[sets == s] = M.raw_forward(params[s], widths, x[sets == s])
    return sample_head(y, head, lo, hi, noise, None if sigma is None else np.asarray(sigma, np.float32)[sets]), y


def gae(reward, kind, values, gamma, lam):
    """(adv, ret) float32 [T, n] of ``reward`` float64 [T, n], ``kind`` uint8 [T, n] and ``values`` float32 [T+1, n]."""
    adv, ret = gae_f64(reward, kind, values, gamma, lam)
    return adv.astype(np.float32), ret.astype(np.float32)


def gae_f64(reward, kind, values, gamma, lam):
    """``gae`` before the cast to float32: t from T-1 down to 0, the carry ``c`` per env, one float64 rounding per line."""
    reward, kind = np.asarray(reward, np.float64), np.asarray(kind, np.uint8)
    v = np.asarray(values, np.float32).astype(np.float64)
    T, n = reward.shape
    assert v.shape == (T + 1, n) and kind.shape == (T, n)
    gamma = np.float64(gamma)
    gl = gamma * np.float64(lam)
    adv, ret = np.zeros((T, n), np.float64), np.zeros((T, n), np.float64)
    c = np.zeros(n, np.float64)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            r, v0, v1, k = reward[t], v[t], v[t + 1], kind[t]
            x = gamma * v1
            y = r + x
            d = y - v0
            z = gl * c
            step = d + z
            term = r - v0
            c = np.where(k == VOID, 0.0, np.where(k == TERMINATED, term, np.where(k == TRUNCATED, d, step)))
            adv[t] = np.where(k == VOID, 0.0, c)
            ret[t] = np.where(k == VOID, 0.0, c + v0)
    return adv, ret
