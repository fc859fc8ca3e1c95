"""numpy twin of the backward pass of the MLP population (include/ftl.h, the ftl_mlp_backward block): the contract's order written out
with ``mlp_numpy.fmaf32``, per weight set.  The hidden layers are ``mlp_tanh_numpy.raw_forward``'s loop with every activation kept; the
deltas are the j-ordered chains from +0 times the activation's derivative; a weight gradient is, per span of ``abi.FTL_MLP_BWD_SPAN``
tiles of the set's block-major tile list, the chain from +0 over the 32 row slots of every tile (slots past a cut tile's end are +0 in
both factors), and the spans are summed in float64 in ascending order and rounded once.  The device is pinned to this bit for bit
(tests/test_gpu_mlp_backward.py)."""
import numpy as np

import mlp_numpy as M
import rnn_numpy as R
from continiousenvironment_follower_leader_amd import abi

F = np.float32
TILE, SPAN = abi.FTL_MLP_ENV_TILE, abi.FTL_MLP_BWD_SPAN


def hidden_forward(params, widths, x, activation):
    """[(acc_l, h_l)] of the hidden layers l = 1 .. L-1 of rows ``x`` under one weight set: the chains of ``ftl_mlp_forward``."""
    h, out = np.asarray(x, F), []
    ls = M.layers(np.asarray(params, F), widths)
    for W, b in ls[:-1]:
        acc = np.broadcast_to(b, (h.shape[0], W.shape[1])).astype(F)
        for k in range(W.shape[0]):
            acc = M.fmaf32(h[:, k:k + 1], W[k][None, :], acc)
        with np.errstate(all="ignore"):
            h = R.tanh32(acc) if activation == "tanh" else np.where(acc > 0, acc, F(0.0)).astype(F)
        out.append((acc, h))
    return out


def deltas(params, widths, x, dy, activation, relu_ge=False, tanh_two_roundings=False):
    """([h_0 .. h_{L-1}], [delta_1 .. delta_L]) of rows ``x`` with head gradients ``dy`` under one weight set.  ``relu_ge`` and
    ``tanh_two_roundings`` are NOT the contract: the ReLU derivative taken where acc >= 0 instead of acc > 0, and 1 - a * a with the
    product rounded before the subtraction instead of ``fmaf(-a, a, 1)``.  Tests re-run the twin with them to show that their rows reach
    the places where the difference shows."""
    ls = M.layers(np.asarray(params, F), widths)
    hid = hidden_forward(params, widths, x, activation)
    hs = [np.asarray(x, F)] + [h for _, h in hid]
    ds = [None] * len(ls)
    ds[-1] = np.asarray(dy, F)
    for l in range(len(ls) - 1, 0, -1):                        # ds[l] is delta of layer l + 1; ds[l - 1] follows from it through ls[l]
        W = ls[l][0]
        c = np.zeros((hs[0].shape[0], W.shape[0]), F)
        with np.errstate(all="ignore"):
            for j in range(W.shape[1]):
                c = M.fmaf32(W[:, j][None, :], ds[l][:, j:j + 1], c)
            acc, a = hid[l - 1]
            if activation == "tanh":
                d = (F(1.0) - (a * a).astype(F)).astype(F) if tanh_two_roundings else M.fmaf32(-a, a, F(1.0))
                ds[l - 1] = (c * d).astype(F)
            else:
                ds[l - 1] = np.where((acc >= 0) if relu_ge else (acc > 0), c, F(0.0)).astype(F)
    return hs, ds


def set_grad(params, widths, xb, dyb, activation="relu", **wrong):
    """float32 [param_count]: the gradient of one weight set whose rows are ``xb`` [B, rows, widths[0]] with head gradients ``dyb``
    [B, rows, widths[-1]] (its rows of every block, in block order)."""
    xb, dyb = np.asarray(xb, F), np.asarray(dyb, F)
    B, rows = xb.shape[:2]
    hs, ds = deltas(params, widths, xb.reshape(B * rows, -1), dyb.reshape(B * rows, -1), activation, **wrong)
    tiles = (rows + TILE - 1) // TILE
    slot = np.full((B, tiles * TILE), -1, np.int64)            # the row of every slot of the block-major tile list; -1 past a cut tile's end
    slot[:, :rows] = np.arange(B * rows).reshape(B, rows)
    slot = slot.reshape(-1)
    live = slot >= 0
    out = []
    for l in range(len(widths) - 1):
        a = np.zeros((slot.size, widths[l] + 1), F)            # h_{l-1} and the bias's 1.0; +0 in the dead slots
        a[live, :-1], a[live, -1] = hs[l][slot[live]], F(1.0)
        d = np.zeros((slot.size, widths[l + 1]), F)
        d[live] = ds[l][slot[live]]
        total = np.zeros((widths[l] + 1, widths[l + 1]), np.float64)
        with np.errstate(all="ignore"):
            for s0 in range(0, slot.size, SPAN * TILE):
                acc = np.zeros(total.shape, F)
                for r in range(s0, min(s0 + SPAN * TILE, slot.size)):
                    acc = M.fmaf32(a[r][:, None], d[r][None, :], acc)
                total = total + acc.astype(np.float64)
            out.append(total.astype(F).reshape(-1))
    return np.concatenate(out)


def population_grad(params, widths, x, dy, envs_per_set, env_first=0, activation="relu", fill=np.nan, **wrong):
    """float32 [n_sets, param_count]: ``set_grad`` of every set that rows ``x`` [B, n, widths[0]] touch under the rule
    (env_first + r) // envs_per_set; the rows of untouched sets hold ``fill``."""
    x, dy, params = np.asarray(x, F), np.asarray(dy, F), np.asarray(params, F)
    sets = (env_first + np.arange(x.shape[1])) // envs_per_set
    out = np.full(params.shape, fill, F)
    for s in np.unique(sets):
        out[s] = set_grad(params[s], widths, x[:, sets == s], dy[:, sets == s], activation, **wrong)
    return out


def workspace_bytes(widths, n_blocks, n, envs_per_set, env_first=0):
    """``ftl_sizeof_mlp_backward_workspace`` by its formula: the spans of every touched set times the parameter count times 4."""
    sets = (env_first + np.arange(n)) // envs_per_set
    spans = sum(-(-(n_blocks * -(-int((sets == s).sum()) // TILE)) // SPAN) for s in np.unique(sets))
    return spans * M.param_count(widths) * 4
