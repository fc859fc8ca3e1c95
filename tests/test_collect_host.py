"""The numpy twin of the trajectory collection (tests/collect_numpy.py) against independent formulations; no GPU, no library."""
import numpy as np
import pytest

import collect_numpy as CN
import mlp_numpy as M

LO, HI = np.array([0.0, -0.57]), np.array([0.5, 0.57])


def _heads(seed, n, w):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((n, w)) * 1.5).astype(np.float32)
    y[0, 0], y[1, 0], y[2, 0], y[3, 0] = np.float32(-0.0), np.float32(np.nan), np.float32(np.inf), np.float32(2.0 ** -140)
    return y


@pytest.mark.parametrize("head, w", [(M.BOX2, 2), (M.TURN, 1), (M.DISCRETE, 5)])
def test_zero_noise_is_the_deterministic_head(head, w):
    y = _heads(head, 64, w)
    sigma = np.abs(_heads(10 + head, 64, w)) + np.float32(0.1)
    sigma[np.isnan(sigma) | np.isinf(sigma)] = 1.0
    want = M.head_of(y, head, LO, HI)
    for noise in (None, np.zeros_like(y), -np.zeros_like(y)):
        got = CN.sample_head(y, head, LO, HI, noise, sigma)
        assert got.dtype == want.dtype and np.array_equal(got, want)


def test_noise_moves_the_box_head_by_sigma_times_noise():
    y = np.array([[0.25, -0.5]], np.float32)
    sigma, noise = np.array([[0.5, 0.25]], np.float32), np.array([[1.0, -2.0]], np.float32)
    got = CN.sample_head(y, M.BOX2, LO, HI, noise, sigma)
    assert np.array_equal(got, M.head_of(np.array([[0.75, -1.0]], np.float32), M.BOX2, LO, HI))      # every value here is exact
    big = CN.sample_head(y, M.BOX2, LO, HI, np.array([[1e30, -1e30]], np.float32), sigma)
    assert np.array_equal(big, np.array([[HI[0], LO[1]]]))
    # the float64 sum keeps what a float32 sum would lose
    tiny = CN.box_sample(np.float32([1.0]), np.float32([1.0]), np.float32([-2.0 ** -30]), -1.0, 1.0)
    assert tiny[0] == ((1.0 - 2.0 ** -30) + 1.0) * 0.5 * 2.0 - 1.0 and tiny[0] < 1.0


def test_discrete_sample_takes_the_first_maximum_and_ignores_nan():
    y = np.zeros((4, 5), np.float32)
    noise = np.zeros((4, 5), np.float32)
    noise[0, 3] = 1.0                          # a Gumbel draw lifts 3
    noise[1, 2] = noise[1, 4] = 2.0            # a tie: the first wins
    noise[2, 1] = np.nan                       # a NaN never beats anything
    noise[2, 4] = 0.5
    noise[3, 0] = np.nan                       # ... and at index 0 nothing beats it (y_j > NaN is false): the rule of ftl_mlp_act
    noise[3, 2] = 9.0
    assert CN.discrete_sample(y, noise).tolist() == [3, 2, 4, 0]
    nan0 = np.zeros((1, 5), np.float32)
    nan0[0, 0] = np.nan
    assert M.discrete_head(nan0).tolist() == [0]


# ---------------------------------------------------------------- gae
def _case(seed, T, n):
    rng = np.random.default_rng(seed)
    reward = rng.standard_normal((T, n)) * rng.choice([1e-3, 1.0, 50.0], (T, n))
    values = (rng.standard_normal((T + 1, n)) * rng.choice([1e-2, 1.0, 20.0], (T + 1, n))).astype(np.float32)
    kind = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), (T, n))
    return reward, kind, values


def _gae_by_sums(reward, kind, values, gamma, lam):
    """Independent: A_t = sum_l (gamma * lam)^l delta_{t+l} over the rows up to and including the one that ends the episode (or the
    window), delta without bootstrap at a terminated row; a VOID row has no advantage and ends the sum of the rows before it."""
    T, n = reward.shape
    v = values.astype(np.float64)
    adv = np.zeros((T, n))
    for e in range(n):
        for t in range(T):
            if kind[t, e] == CN.VOID:
                continue
            w, total = 1.0, 0.0
            for u in range(t, T):
                k = kind[u, e]
                if k == CN.VOID:
                    break
                boot = 0.0 if k == CN.TERMINATED else gamma * v[u + 1, e]
                total += w * (reward[u, e] + boot - v[u, e])
                if k != CN.STEP:
                    break
                w *= gamma * lam
            adv[t, e] = total
    return adv, np.where(kind == CN.VOID, 0.0, adv + v[:-1])


@pytest.mark.parametrize("gamma, lam", [(1.0, 1.0), (0.99, 0.95), (0.0, 0.5)])
def test_gae_matches_the_sum_formulation(gamma, lam):
    """Tolerance from the operation count.  Both sides make at most 5 float64 roundings per row they pass (x, y, d, z, c here; a
    product, two sums, a weight and an accumulation there), at most T rows, each rounding at most 2^-53 of its result, and with gamma *
    lam <= 1 no step amplifies an earlier error.  Every intermediate is bounded by S = sum_t (|r_t| + 2 |v|max) of the env's column, so
    |twin - sums| <= 2 * 5 * T * 2^-53 * S."""
    T, n = 9, 40
    reward, kind, values = _case(3, T, n)
    adv, ret = CN.gae_f64(reward, kind, values, gamma, lam)
    wa, wr = _gae_by_sums(reward, kind, values, gamma, lam)
    S = (np.abs(reward) + 2 * np.abs(values).max(0)[None]).sum(0)
    tol = 2 * 5 * T * 2.0 ** -53 * S
    assert (np.abs(adv - wa) <= tol[None]).all() and (np.abs(ret - wr) <= tol[None] + 2.0 ** -53 * np.abs(wr)).all()
    a32, r32 = CN.gae(reward, kind, values, gamma, lam)
    assert a32.dtype == r32.dtype == np.float32 and np.array_equal(a32, adv.astype(np.float32)) and np.array_equal(r32, ret.astype(np.float32))
    assert (a32[kind == CN.VOID] == 0).all() and (r32[kind == CN.VOID] == 0).all()


def test_lambda_one_without_boundaries_is_the_return_to_go():
    """lambda = 1, every row a STEP: adv_t + v_t = sum_{u >= t} gamma^(u - t) r_u + gamma^(T - t) v_T, compared in float64 before the
    cast.  The recursion makes 5 roundings per row and the reference 3 (power, product, sum), over at most T rows, each at most 2^-53
    of a result bounded by S = sum |r| + 3 |v|max: tolerance 8 * T * 2^-53 * S."""
    T, n, gamma = 9, 33, 0.97
    reward, _, values = _case(4, T, n)
    kind = np.zeros((T, n), np.uint8)
    adv, ret = CN.gae_f64(reward, kind, values, gamma, 1.0)
    v = values.astype(np.float64)
    want = np.zeros((T, n))
    for t in range(T):
        want[t] = sum(gamma ** (u - t) * reward[u] for u in range(t, T)) + gamma ** (T - t) * v[T]
    S = np.abs(reward).sum(0) + 3 * np.abs(v).max(0)
    tol = 8 * T * 2.0 ** -53 * S
    assert (np.abs(ret - want) <= tol[None]).all(), np.abs(ret - want).max()
    assert (np.abs(adv - (want - v[:-1])) <= tol[None]).all()


def test_a_void_row_cuts_the_carry():
    T, n, cut = 9, 17, 5
    reward, _, values = _case(5, T, n)
    kind = np.zeros((T, n), np.uint8)
    kind[cut] = CN.VOID
    adv, ret = CN.gae(reward, kind, values, 0.99, 0.95)
    assert (adv[cut] == 0).all() and (ret[cut] == 0).all()
    # the rows before the cut are the advantages of that prefix alone: they bootstrap from values[cut] and see nothing behind it
    pa, pr = CN.gae(reward[:cut], kind[:cut], values[:cut + 1], 0.99, 0.95)
    assert np.array_equal(adv[:cut], pa) and np.array_equal(ret[:cut], pr)
    later = reward.copy()
    later[cut:] += 100.0
    a2, _ = CN.gae(later, kind, values, 0.99, 0.95)
    assert np.array_equal(a2[:cut], adv[:cut]) and not np.array_equal(a2[cut + 1:], adv[cut + 1:])
    # without the VOID row the carry passes
    a3, _ = CN.gae(later, np.zeros((T, n), np.uint8), values, 0.99, 0.95)
    assert not np.array_equal(a3[:cut], adv[:cut])
    # a terminated row does not bootstrap, a truncated one does
    kind[:] = CN.STEP
    kind[cut] = CN.TERMINATED
    at, _ = CN.gae_f64(reward, kind, values, 0.99, 0.95)
    kind[cut] = CN.TRUNCATED
    au, _ = CN.gae_f64(reward, kind, values, 0.99, 0.95)
    v = values.astype(np.float64)
    assert np.array_equal(at[cut], reward[cut] - v[cut]) and np.array_equal(au[cut], (reward[cut] + 0.99 * v[cut + 1]) - v[cut])
