"""CPU checks of the backward pass of the MLP population (include/ftl.h: ``ftl_mlp_backward``, ``ftl_sizeof_mlp_backward_workspace``;
``mlp.backward``, ``mlp.Net``): the exports, every refusal that comes before any device work -- on a handle that never got a state, and
never with a call that would pass them all, so nothing here can launch --, the workspace query against its formula, the Python argument
checks on CPU tensors with the library patched out, and the twin (tests/mlp_backward_numpy.py) against torch float64 autograd inside a
bound derived from the operation count."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import mlp_backward_numpy as MB
import mlp_numpy as M
import rnn_numpy as R
import test_mlp_abi as A
from continiousenvironment_follower_leader_amd import _lib, abi, mlp
from test_mlp_abi import cfg_b, handle, lib  # noqa: F401  (fixtures)

F = np.float32
FAKE, N, W0 = A.FAKE, A.N, A.W0
U32, U64 = 2.0 ** -24, 2.0 ** -53
TANH32_ABS = 8.93e-8                        # include/ftl.h: tanh32 against the float64 value, absolute
LAST = b"workspace must be 4-byte aligned"  # the last check of ftl_mlp_backward: a call refused with it has passed every other one
BIG = 1 << 40


def _bwd(lib, h, net="x", n_blocks=2, n=N, x=FAKE, xb=None, dy=2 * FAKE, dyb=None, grad=3 * FAKE, ws=4 * FAKE, wsb=BIG):
    net = A._net() if net == "x" else net
    w0, wl = (net.width[0], net.width[max(0, min(net.n_layers, abi.FTL_MLP_MAX_LAYERS))]) if net is not None else (W0, 2)
    xb = n * w0 * 4 if xb is None else xb
    dyb = n * wl * 4 if dyb is None else dyb
    return lib.ftl_mlp_backward(h, C.byref(net) if net is not None else None, n_blocks, n, x, xb, dy, dyb, grad, ws, wsb, None)


def _passes_all_but_the_last(lib, h, **kw):
    """The call with a misaligned workspace: FTL_E_INVALID with the message of the last check, so every check before it let the call pass."""
    rc = _bwd(lib, h, ws=4 * FAKE + 1, **kw)
    return rc == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()


# ---------------------------------------------------------------- the exports
def test_symbols_declared_exported_and_listed(lib):
    hdr = A._header()
    for s in ("ftl_mlp_backward", "ftl_sizeof_mlp_backward_workspace"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s) and s in _lib.EXPORTS, s
    assert lib.ftl_mlp_backward.restype is C.c_int and len(lib.ftl_mlp_backward.argtypes) == 12
    assert lib.ftl_sizeof_mlp_backward_workspace.restype is C.c_int64
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no struct changed
    assert C.sizeof(abi.Mlp) == lib.ftl_sizeof_mlp() == 56
    assert int(re.search(r"#define\s+FTL_MLP_BWD_SPAN\s+(\d+)", hdr).group(1)) == abi.FTL_MLP_BWD_SPAN == MB.SPAN
    assert re.search(r"#define\s+FTL_MLP_BWD_MAX_IN\s+FTL_MLP_MAX_IN\b", hdr) and abi.FTL_MLP_BWD_MAX_IN == abi.FTL_MLP_MAX_IN >= 512


# ---------------------------------------------------------------- refusals before any device work
def test_null_arguments_are_named(lib, handle):
    h = handle
    for kw, hh, word in ((dict(), None, b": h"), (dict(net=None), h, b": net"), (dict(net=A._net(params=None)), h, b"net->params"),
                         (dict(x=None), h, b": x"), (dict(dy=None), h, b": dy"), (dict(grad=None), h, b": grad"), (dict(ws=None), h, b": workspace")):
        assert _bwd(lib, hh, **kw) == abi.FTL_E_INVALID, word
        err = lib.ftl_last_error()
        assert b"ftl_mlp_backward" in err and b"null" in err and err.endswith(word), (word, err)


def test_the_net_is_refused_as_ftl_mlp_act_refuses_it(lib, handle):
    h = handle
    own = (b"null", b"last weight set", b"H * W", b"head width")
    seen = 0
    for net, code, msg in A._bad_nets():
        if msg in (b"H * W", b"head width"):
            continue
        assert _bwd(lib, h, net=net) == code, msg
        err = lib.ftl_last_error()
        assert msg in err, (msg, err)
        if msg not in own:                                             # the very message of ftl_mlp_act, byte for byte
            assert A._act(lib, h, net=net) == code and lib.ftl_last_error() == err, (msg, err)
            seen += 1
    assert seen >= 9
    for bad in (2, -1, 7, 1 << 30):
        net = A._net(activation=bad)
        assert _bwd(lib, h, net=net) == abi.FTL_E_INVALID and b"activation" in lib.ftl_last_error(), bad
        err = lib.ftl_last_error()
        assert A._act(lib, h, net=net) == abi.FTL_E_INVALID and lib.ftl_last_error() == err
    for good in (abi.FTL_MLP_ACT_RELU, abi.FTL_MLP_ACT_TANH):
        assert _passes_all_but_the_last(lib, h, net=A._net(activation=good)), lib.ftl_last_error()


def test_every_net_inside_the_limits_passes(lib, handle):
    h = handle
    dense = [(W0, a, a, 2) for a in (8, 16, 32, 64, 128, 256)]             # the dense nets of the reference's Architecture.conf
    for widths in dense + [(W0, 64, 3), (W0, 256), (7, 1), (512, 64, 2), (4096, 256, 256, 256, 256)]:
        assert _passes_all_but_the_last(lib, h, net=A._net(widths)), (widths, lib.ftl_last_error())
    assert _bwd(lib, h, net=A._net((4097, 2))) == abi.FTL_E_UNSUPPORTED and b"MAX_IN" in lib.ftl_last_error()
    assert _bwd(lib, h, net=A._net((W0, 64, 257))) == abi.FTL_E_UNSUPPORTED and b"FTL_MLP_MAX_WIDTH" in lib.ftl_last_error()
    assert _bwd(lib, h, net=A._net((W0, 64, 0))) == abi.FTL_E_INVALID and b"at least 1" in lib.ftl_last_error()
    for kw, n, ok in ((dict(n_sets=2, envs_per_set=3), 6, True), (dict(n_sets=2, envs_per_set=3), 7, False),
                      (dict(n_sets=3, envs_per_set=4, env_first=7), 5, True), (dict(n_sets=3, envs_per_set=4, env_first=7), 6, False)):
        if ok:
            assert _passes_all_but_the_last(lib, h, net=A._net(**kw), n=n), (kw, n, lib.ftl_last_error())
        else:
            assert _bwd(lib, h, net=A._net(**kw), n=n) == abi.FTL_E_INVALID and b"last weight set" in lib.ftl_last_error(), (kw, n)


def test_counts_strides_workspace_and_alignment(lib, handle):
    h = handle
    for kw in (dict(n_blocks=0), dict(n_blocks=-1), dict(n=0), dict(n=-3)):
        assert _bwd(lib, h, xb=4096, dyb=4096, **kw) == abi.FTL_E_INVALID, kw
        assert b"n_blocks and n" in lib.ftl_last_error()
    assert _bwd(lib, h, n_blocks=65536) == abi.FTL_E_UNSUPPORTED and b"65,535" in lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, n_blocks=65535) and _passes_all_but_the_last(lib, h, n_blocks=1)
    big = A._net(n_sets=1, envs_per_set=1 << 30)
    assert _bwd(lib, h, net=big, n=1 << 30) == abi.FTL_E_UNSUPPORTED and b"tiles" in lib.ftl_last_error()
    many = A._net((7, 1), n_sets=1 << 25, envs_per_set=1)                      # 2^25 sets of one row: 2^25 spans
    assert _bwd(lib, h, net=many, n=1 << 25, n_blocks=1) == abi.FTL_E_UNSUPPORTED and b"spans" in lib.ftl_last_error()
    xb, dyb = N * W0 * 4, N * 2 * 4
    for kw, word in ((dict(xb=xb - 4), b"x_block_bytes"), (dict(xb=xb + 2), b"x_block_bytes"), (dict(xb=0), b"x_block_bytes"),
                     (dict(xb=-xb), b"x_block_bytes"), (dict(dyb=dyb - 4), b"dy_block_bytes"), (dict(dyb=dyb + 1), b"dy_block_bytes"),
                     (dict(dyb=0), b"dy_block_bytes"), (dict(x=FAKE + 2), b"x must be 4-byte aligned"), (dict(dy=2 * FAKE + 1), b"dy must be 4-byte aligned"),
                     (dict(grad=3 * FAKE + 3), b"grad must be 4-byte aligned")):
        assert _bwd(lib, h, **kw) == abi.FTL_E_INVALID, kw
        assert word in lib.ftl_last_error(), (kw, lib.ftl_last_error())
    for ws in (4 * FAKE + 1, 4 * FAKE + 2, 4 * FAKE + 3):
        assert _bwd(lib, h, ws=ws) == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()
    for kw in (dict(xb=xb + 4), dict(xb=10 * xb, dyb=3 * dyb), dict(dyb=dyb + 4)):      # padded blocks are fine
        assert _passes_all_but_the_last(lib, h, **kw), (kw, lib.ftl_last_error())
    need = lib.ftl_sizeof_mlp_backward_workspace(C.byref(A._net()), 2, N)
    assert need == 15874 * 4                                                  # 2 blocks of one cut tile: one span of the 180-64-64-2 net
    for wsb in (need - 1, need - 4, 0, -8):
        assert _bwd(lib, h, wsb=wsb) == abi.FTL_E_INVALID and b"workspace_bytes" in lib.ftl_last_error(), wsb
    assert _passes_all_but_the_last(lib, h, wsb=need)


def test_workspace_query_against_the_formula_by_hand(lib):
    q = lib.ftl_sizeof_mlp_backward_workspace
    count = 15874
    # (net, n_blocks, n) -> spans, counted by hand: tiles of 32 rows end at set boundaries, spans of 64 tiles per set
    cases = [(dict(n_sets=1, envs_per_set=1 << 20), 1, 15, 1),                 # one tile
             (dict(n_sets=1, envs_per_set=1 << 20), 70, 40, 3),                # 140 tiles of one set: 64 + 64 + 12
             (dict(n_sets=1, envs_per_set=1 << 20), 64, 32, 1), (dict(n_sets=1, envs_per_set=1 << 20), 65, 32, 2),
             (dict(n_sets=3, envs_per_set=11), 3, 33, 3),                      # 3 sets of 3 tiles
             (dict(n_sets=3, envs_per_set=11), 65, 33, 6),                     # 3 sets of 65 tiles: 2 spans each
             (dict(n_sets=4, envs_per_set=10, env_first=13), 3, 21, 3),        # 7 + 10 + 4 rows
             (dict(n_sets=4, envs_per_set=10, env_first=13), 33, 21, 3), (dict(n_sets=4, envs_per_set=40, env_first=5), 33, 85, 2 + 2 + 1),     # 35 + 40 + 10 rows: 66, 66 and 33 tiles
             (dict(n_sets=1024, envs_per_set=64), 32, 65536, 1024),            # the population of the measured table: a span a set
             (dict(n_sets=1, envs_per_set=65536), 32, 65536, 1024)]            # one set: 2,048 tiles a block
    for kw, B, n, spans in cases:
        assert q(C.byref(A._net(**kw)), B, n) == spans * count * 4 == MB.workspace_bytes((W0, 64, 64, 2), B, n, kw["envs_per_set"], kw.get("env_first", 0)), (kw, B, n)
    assert q(C.byref(A._net((7, 1), n_sets=1, envs_per_set=40)), 70, 40) == 3 * 8 * 4
    for net, B, n in ((None, 1, 1), (A._net(), 0, 1), (A._net(), 1, 0), (A._net(envs_per_set=0), 1, 1), (A._net(env_first=-1), 1, 1),
                      (A._net((W0, 257, 2)), 1, 1), (A._net((W0, 2), n_layers=0), 1, 1)):
        assert q(C.byref(net) if net is not None else None, B, n) == -1


# ---------------------------------------------------------------- the python surface
def test_python_surface(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("a library call before the argument checks were through")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(mlp, "_device_handle", no_library)
    p = inspect.signature(mlp.backward).parameters
    assert list(p) == ["widths", "params", "x", "dy", "activation", "out"] and p["activation"].default == "relu" and p["out"].default is None
    p = inspect.signature(mlp.Net.__init__).parameters
    assert list(p)[1:] == ["widths", "n_sets", "activation", "params", "device"]
    assert [p[k].default for k in list(p)[2:]] == [1, "relu", None, None]
    assert issubclass(mlp.Net, torch.nn.Module) and all(callable(getattr(mlp.Net, name)) for name in ("load", "module", "forward"))
    for name in ("module", "_hold"):                                                    # one base under Net and Critic: shared, not copied
        assert getattr(mlp.Net, name) is getattr(mlp.Critic, name) and name not in vars(mlp.Net) and name not in vars(mlp.Critic)
    assert mlp.Critic.load is mlp._Holder.load and "load" not in vars(mlp.Critic)      # (Net.load is the same under no_grad)

    widths = (5, 4, 3)
    count = abi.mlp_param_count(widths)
    params, x, dy = torch.zeros(2, count), torch.zeros(3, 6, 5), torch.zeros(3, 6, 3)
    bad = [dict(params=torch.zeros(2, count + 1)), dict(params=torch.zeros(count)), dict(params=torch.zeros(2, count, dtype=torch.float64)),
           dict(params=torch.zeros(2, 2 * count)[:, ::2]), dict(params=None),
           dict(x=torch.zeros(3, 6, 5, dtype=torch.float64)), dict(x=torch.zeros(3, 6, 4)), dict(x=None), dict(x=torch.zeros(3, 7, 5)),
           dict(x=torch.zeros(3, 6, 5, requires_grad=True)), dict(x=torch.zeros(0, 6, 5)),
           dict(dy=torch.zeros(3, 6, 4)), dict(dy=torch.zeros(6, 3)), dict(dy=torch.zeros(3, 6, 3, dtype=torch.float64)), dict(dy=None),
           dict(dy=torch.zeros(3, 6, 6)[:, :, ::2]), dict(dy=torch.zeros(3, 6, 3, requires_grad=True)),
           dict(out=torch.zeros(2, count + 1)), dict(out=torch.zeros(count)), dict(out=torch.zeros(2, count, dtype=torch.float64)),
           dict(activation="gelu"), dict(activation=1), dict(widths=(5,)), dict(widths=(5, 0, 3)), dict(widths=(4, 4, 3))]
    for over in bad:
        with pytest.raises(ValueError):
            mlp.backward(**dict(dict(widths=widths, params=params, x=x, dy=dy), **over))
    for w, xs in (((5, 257, 3), (2, 5)), ((4097, 3), (2, 4097)), ((5, 4, 4, 4, 4, 3), (2, 5))):
        with pytest.raises(NotImplementedError):
            mlp.backward(w, torch.zeros(1, 1), torch.zeros(*xs), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="GPU"):                               # every argument fine but the device: still no library call
        mlp.backward(widths, params, x, dy)
    with pytest.raises(ValueError, match="GPU"):
        mlp.backward(widths, params, x, dy, "tanh", torch.zeros(2, count))
    with pytest.raises(ValueError, match="backward"):                          # forward() keeps its refusal, word for word
        mlp.forward(widths, params.clone().requires_grad_(), x)

    # Net
    with pytest.raises(ValueError):
        mlp.Net((5,), device="cpu")
    with pytest.raises(NotImplementedError):
        mlp.Net((5, 257, 1), device="cpu")
    with pytest.raises(ValueError, match="activation"):
        mlp.Net((5, 4, 1), activation="gelu", device="cpu")
    with pytest.raises(ValueError, match="n_sets"):
        mlp.Net((5, 4, 1), n_sets=0, device="cpu")
    with pytest.raises(ValueError, match="params"):
        mlp.Net((5, 4, 1), n_sets=2, params=torch.zeros(1, abi.mlp_param_count((5, 4, 1))))
    net = mlp.Net(widths, n_sets=2, device="cpu")
    assert net.activation == "relu" and [tuple(q.shape) for q in net.parameters()] == [(2, count)] and isinstance(net.params, torch.nn.Parameter)
    assert net.params.dtype == torch.float32 and not net.params.detach().any()
    shared = torch.zeros(2, count)
    net = mlp.Net(widths, n_sets=2, activation="tanh", params=shared)
    assert net.params.data_ptr() == shared.data_ptr()                          # the policy's or the critic's own tensor
    torch.manual_seed(5)
    module = mlp.torch_module(widths, "tanh")
    assert net.load(module) is net and torch.equal(shared[0], mlp.params_from_torch(module)[2]) and torch.equal(shared[1], shared[0])
    assert torch.equal(mlp.params_from_torch(net.module(1))[2], shared[1])
    with pytest.raises(ValueError):
        net.load(mlp.torch_module(widths, "relu"))
    with pytest.raises(IndexError):
        net.module(2)
    with pytest.raises(ValueError, match="grad"):
        net(torch.zeros(3, 6, 5, requires_grad=True))
    with pytest.raises(ValueError, match="GPU"):
        net(torch.zeros(3, 6, 5))


# ---------------------------------------------------------------- the twin against float64 autograd
def f64_grad_and_bound(params, widths, xb, dyb, activation):
    """(twin gradient, float64 gradient g64, bound) of one weight set on rows xb [B, rows, W0] with head gradients dyb, for the loss
    sum(dy * head): g64 is torch float64 autograd through ``mlp.torch_module``; bound >= |twin - g64| elementwise, derived from the operation
    count on the twin's own intermediates.  u = 2^-24, g(K) = K u / (1 - K u); a hat marks the twin's float32 value, E a bound of its error:
      forward   as tests/test_mlp_tanh_host.py::_f64_and_bound: E_acc = g32(K) S32 + K 2^-150 + E_h |W| + g64(K + 1) S64; tanh adds 8.93e-8
                (tanh32) + 2^-52 (np.tanh) and is 1-Lipschitz; the ReLU adds nothing.
      c         the chain over the J outputs of the next layer: E_c = g32(J) |delta^| |W|^T + J 2^-150 + E_delta |W|^T + g64(J + 1) (...).
      tanh      d^ = fmaf(-a^, a^, 1), one rounding of 1 - a^2 <= 1: E_d = u + 2 E_a (|a| <= 1) + 4 u64; delta^ = fl(c^ d^):
                E_delta = u |c^ d^| + 2^-150 + E_c |d^| + (|c^| + E_c) E_d.
      relu      where |acc^| > E_acc both selects agree: E_delta = E_c there, 0 where both drop it; where |acc^| <= E_acc the selects may
                differ and the whole value is the error: |c^| + E_c.
      sums      a span's chain has R <= 2,048 slots: g32(R) |A^|^T |D^| + R 2^-150 per word in all, the float64 sum of the spans and its
                one rounding u |g^| + 2^-150; the inputs |A^|^T E_D + E_A^T (|D^| + E_D); float64's own g64(rows + 2) (...)."""
    params, xb, dyb = np.asarray(params, F), np.asarray(xb, F), np.asarray(dyb, F)
    twin = MB.set_grad(params, widths, xb, dyb, activation)
    B, rows = xb.shape[:2]
    x, dy = xb.reshape(B * rows, -1), dyb.reshape(B * rows, -1)
    mod = mlp.torch_module(widths, activation, torch.from_numpy(params)).double()
    (mod(torch.from_numpy(x).double()) * torch.from_numpy(dy).double()).sum().backward()
    g64 = np.concatenate([np.concatenate([lin.weight.grad.numpy().T.reshape(-1), lin.bias.grad.numpy()]) for lin in mod[::2]])
    ls = M.layers(params, widths)
    L = len(ls)
    g = lambda K, u: K * u / (1 - K * u)
    # forward: the twin's values and their error bounds
    hid = MB.hidden_forward(params, widths, x, activation)
    hs, Eh, Eacc = [x.astype(np.float64)], [np.zeros(x.shape)], []
    h64 = x.astype(np.float64)
    for l in range(L - 1):
        W64, b64, K = ls[l][0].astype(np.float64), ls[l][1].astype(np.float64), ls[l][0].shape[0]
        S32, S64 = np.abs(hs[-1]) @ np.abs(W64) + np.abs(b64), np.abs(h64) @ np.abs(W64) + np.abs(b64)
        E = g(K, U32) * S32 + K * 2.0 ** -150 + Eh[-1] @ np.abs(W64) + g(K + 1, U64) * S64
        Eacc.append(E)
        acc64 = h64 @ W64 + b64
        h64 = np.tanh(acc64) if activation == "tanh" else np.maximum(acc64, 0)
        hs.append(hid[l][1].astype(np.float64))
        Eh.append(E + TANH32_ABS + 2.0 ** -52 if activation == "tanh" else E)
    # backward: the deltas and their error bounds
    _, ds = MB.deltas(params, widths, x, dy, activation)
    Ed = [None] * L
    Ed[L - 1] = np.zeros(dy.shape)
    for l in range(L - 1, 0, -1):
        W64, J = np.abs(ls[l][0].astype(np.float64)), ls[l][0].shape[1]
        dabs = np.abs(ds[l].astype(np.float64))
        c = np.zeros((x.shape[0], ls[l][0].shape[0]), F)
        for j in range(J):
            c = M.fmaf32(ls[l][0][:, j][None, :], ds[l][:, j:j + 1], c)
        cabs = np.abs(c.astype(np.float64))
        Ec = g(J, U32) * (dabs @ W64.T) + J * 2.0 ** -150 + Ed[l] @ W64.T + g(J + 1, U64) * ((dabs + Ed[l]) @ W64.T)
        acc, a = hid[l - 1][0].astype(np.float64), hid[l - 1][1].astype(np.float64)
        if activation == "tanh":
            dhat = np.abs(M.fmaf32(-hid[l - 1][1], hid[l - 1][1], F(1.0)).astype(np.float64))
            Edd = U32 + 2 * Eh[l] + 4 * U64
            Ed[l - 1] = U32 * cabs * dhat + 2.0 ** -150 + Ec * dhat + (cabs + Ec) * Edd
        else:
            Ed[l - 1] = np.where(np.abs(acc) <= Eacc[l - 1], cabs + Ec, np.where(acc > 0, Ec, 0.0))
    # the sums over the rows
    slots = B * (-(-rows // MB.TILE)) * MB.TILE
    R = min(slots, MB.SPAN * MB.TILE)
    n = x.shape[0]
    out = []
    for l in range(L):
        Aabs = np.concatenate([np.abs(hs[l]), np.ones((n, 1))], 1)
        EA = np.concatenate([Eh[l], np.zeros((n, 1))], 1)
        Dabs = np.abs(ds[l].astype(np.float64))
        S = Aabs.T @ Dabs
        out.append((g(R, U32) * S + slots * 2.0 ** -150 + Aabs.T @ Ed[l] + EA.T @ (Dabs + Ed[l]) + g(n + 2, U64) * ((Aabs + EA).T @ (Dabs + Ed[l]))).reshape(-1))
    bound = np.concatenate(out)
    bound = bound + U32 * (np.abs(g64) + bound) + 2.0 ** -150
    return twin, g64, bound


BOUND_CASES = [((7, 1), 0), ((65, 17, 3), 1), ((20, 64, 64, 2), 2)]


@pytest.mark.parametrize("scale", [0.1, 0.5])
@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("widths, seed", BOUND_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_twin_within_the_derived_bound_of_float64_autograd(widths, seed, activation, scale):
    rng = np.random.default_rng(100 + seed)
    B, rows = 2 * MB.SPAN // 2 + 1, 40                                         # two tiles a block (32 + 8 rows): 64 + 64 + 2 tiles, three spans
    assert -(-(B * 2) // MB.SPAN) == 3
    p = (rng.standard_normal(M.param_count(widths)) * scale).astype(F)
    x = M.nasty_inputs(rng, B * rows, widths[0]).reshape(B, rows, widths[0])
    dy = rng.standard_normal((B, rows, widths[-1])).astype(F)
    dy[rng.random((B, rows)) < 0.2] = 0.0
    twin, g64, bound = f64_grad_and_bound(p, widths, x, dy, activation)
    err = np.abs(twin.astype(np.float64) - g64)
    print("widths %s %s scale %.1f: max error %.3e, bound there %.3e, largest bound %.3e, max |g| %.3e"
          % (widths, activation, scale, err.max(), bound[err.argmax()], bound.max(), np.abs(g64).max()))
    assert np.isfinite(g64).all() and (np.abs(g64) > 0).mean() > 0.2 and (err <= bound).all(), float((err - bound).max())


def test_a_set_alone_equals_the_middle_set_of_three():
    widths = (65, 17, 3)
    rng = np.random.default_rng(9)
    p = (rng.standard_normal((3, M.param_count(widths))) * 0.3).astype(F)
    x = M.nasty_inputs(rng, 3 * 33, widths[0]).reshape(3, 33, widths[0])
    dy = rng.standard_normal((3, 33, 3)).astype(F)
    for act in ("relu", "tanh"):
        whole = MB.population_grad(p, widths, x, dy, 11, activation=act)
        alone = MB.population_grad(p[1:2], widths, x[:, 11:22], dy[:, 11:22], 11, activation=act)
        assert np.array_equal(whole[1].view(np.uint32), alone[0].view(np.uint32)) and not np.array_equal(whole[0], whole[1])
        part = MB.population_grad(p, widths, x[:, 11:22], dy[:, 11:22], 11, env_first=11, activation=act, fill=F(7.0))
        assert np.array_equal(part[1].view(np.uint32), alone[0].view(np.uint32)) and (part[[0, 2]] == 7).all()


# ---------------------------------------------------------------- constructed rows: the derivative's edges (shared with the GPU tests)
def relu_edge_case():
    """(widths, params [1, count], x [16, 4], dy [16, 2], classes): a (4, 6, 2) ReLU net whose hidden pre-activations are, by unit: exactly
    +0 on the even rows and 1.0 on the odd ones (a one-hot weight on an input that is 0 or 1); exactly -0 (weights and bias -0, inputs >= 0);
    a positive float32 subnormal (kept: acc > 0) and a negative one; 0.5 + and -0.5 + a small term.  The contract drops +0 and -0 and
    keeps the positive subnormal; a select on acc >= 0 keeps the zeros, a device that flushed subnormals would drop the kept one."""
    widths = (4, 6, 2)
    p = np.zeros((1, M.param_count(widths)), F)
    (W0_, b0), (W1, b1) = M.layers(p[0], widths)
    rng = np.random.default_rng(21)
    W0_[0, 0] = 1.0
    W0_[:, 1], b0[1] = F(-0.0), F(-0.0)
    W0_[2, 2], W0_[3, 3] = 1.0, -1.0
    W0_[1, 4], b0[4], W0_[1, 5], b0[5] = 0.25, 0.5, 0.25, -0.5
    W1[:], b1[:] = (rng.standard_normal(W1.shape) + 2).astype(F), 0.1
    x = np.zeros((16, 4), F)
    x[1::2, 0] = 1.0
    x[:, 1] = rng.random(16, dtype=F)
    x[:, 2] = M._sub((1 << 19) + 37 * np.arange(16) + 1)
    x[:, 3] = M._sub((1 << 18) + 5 * np.arange(16) + 1)
    dy = (rng.standard_normal((16, 2)) + 1).astype(F)
    acc = MB.hidden_forward(p[0], widths, x, "relu")[0][0]
    sub = F(2.0 ** -126)
    assert (acc[::2, 0] == 0).all() and not np.signbit(acc[::2, 0]).any() and (acc[1::2, 0] == 1).all()
    assert (acc[:, 1] == 0).all() and np.signbit(acc[:, 1]).all()
    assert ((acc[:, 2] > 0) & (acc[:, 2] < sub)).all() and ((acc[:, 3] < 0) & (acc[:, 3] > -sub)).all()
    return widths, p, x, dy, ("+0", "-0", "+subnormal", "-subnormal", "positive", "negative")


def tanh_edge_case():
    """(widths, params [1, count], x [16, 4], dy [16, 2]): a (4, 6, 2) tanh net with two units saturated to exactly +1 and -1 by their
    biases (d = fmaf(-1, 1, 1) = +0: nothing flows back through them) and four ordinary ones, where fmaf(-a, a, 1) and 1 - fl(a * a)
    differ in the last bit on most rows."""
    widths = (4, 6, 2)
    rng = np.random.default_rng(22)
    p = (rng.standard_normal((1, M.param_count(widths))) * 0.5).astype(F)
    (W0_, b0), _ = M.layers(p[0], widths)
    W0_[:, 0], b0[0], W0_[:, 1], b0[1] = 0.0, 10.0, 0.0, -10.0
    x = rng.standard_normal((16, 4)).astype(F)
    dy = rng.standard_normal((16, 2)).astype(F)
    a = MB.hidden_forward(p[0], widths, x, "tanh")[0][1]
    assert (a[:, 0] == 1).all() and (a[:, 1] == -1).all() and (np.abs(a[:, 2:]) < 1).all()
    assert R.tanh32(F(10.0)) == 1
    return widths, p, x, dy


def test_the_edge_cases_discriminate():
    widths, p, x, dy, _ = relu_edge_case()
    want = MB.set_grad(p[0], widths, x[None], dy[None], "relu")
    assert not np.array_equal(want.view(np.uint32), MB.set_grad(p[0], widths, x[None], dy[None], "relu", relu_ge=True).view(np.uint32))
    W0g = M.layers(want, widths)[0]
    assert (W0g[1][[1, 3, 5]] == 0).all() and W0g[1][2] != 0 and W0g[1][0] != 0 and W0g[1][4] != 0      # db_1: -0, -sub, negative drop out
    widths, p, x, dy = tanh_edge_case()
    want = MB.set_grad(p[0], widths, x[None], dy[None], "tanh")
    assert not np.array_equal(want.view(np.uint32), MB.set_grad(p[0], widths, x[None], dy[None], "tanh", tanh_two_roundings=True).view(np.uint32))
    W0g = M.layers(want, widths)[0]
    assert (W0g[1][:2] == 0).all() and (W0g[1][2:] != 0).all()
