"""CPU checks of the forward pass on caller-supplied rows (include/ftl.h: ``ftl_mlp_forward``; ``mlp.forward``, ``MlpPolicy.forward``,
``mlp.Critic``): the export, every refusal that comes before any device work -- on a handle that never got a state, and never with a
call that would pass them all, so nothing here can launch --, the Python names and their argument checks on CPU tensors, and the
``Critic`` round trip through ``params_from_torch`` / ``torch_module`` with the twin's value inside the derived float64 bound."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import mlp_tanh_numpy as MT
import test_mlp_abi as A
import test_mlp_tanh_host as TH
from continiousenvironment_follower_leader_amd import _lib, abi, mlp
from test_mlp_abi import cfg_b, handle, lib  # noqa: F401  (fixtures)

FAKE, N, W0 = A.FAKE, A.N, A.W0
LAST = b"y must be 4-byte aligned"          # the last check of ftl_mlp_forward: a call refused with it has passed every other one


def _fwd(lib, h, net="x", n_blocks=2, n=N, x=FAKE, xb=None, y=2 * FAKE, yb=None):
    net = A._net() if net == "x" else net
    w0, wl = (net.width[0], net.width[max(0, min(net.n_layers, abi.FTL_MLP_MAX_LAYERS))]) if net is not None else (W0, 2)
    xb = n * w0 * 4 if xb is None else xb
    yb = n * wl * 4 if yb is None else yb
    return lib.ftl_mlp_forward(h, C.byref(net) if net is not None else None, n_blocks, n, x, xb, y, yb, None)


def _passes_all_but_the_last(lib, h, **kw):
    """The call with a misaligned y: FTL_E_INVALID with the message of the last check, so every check before it let the call pass."""
    rc = _fwd(lib, h, y=2 * FAKE + 1, **kw)
    return rc == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()


# ---------------------------------------------------------------- the export
def test_symbol_declared_exported_and_listed(lib):
    hdr = A._header()
    assert re.search(r"\bftl_mlp_forward\s*\(", hdr)
    assert hasattr(lib, "ftl_mlp_forward") and "ftl_mlp_forward" in _lib.EXPORTS
    assert lib.ftl_mlp_forward.restype is C.c_int and len(lib.ftl_mlp_forward.argtypes) == 9
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no struct changed
    assert C.sizeof(abi.Mlp) == lib.ftl_sizeof_mlp() == 56
    assert mlp.FORWARD_MAX_BLOCKS == 65535


# ---------------------------------------------------------------- refusals before any device work
def test_null_arguments_are_named(lib, handle):
    h = handle
    for kw, hh, word in ((dict(), None, b": h"), (dict(net=None), h, b": net"), (dict(net=A._net(params=None)), h, b"net->params"),
                         (dict(x=None), h, b": x"), (dict(y=None), h, b": y")):
        assert _fwd(lib, hh, **kw) == abi.FTL_E_INVALID, word
        err = lib.ftl_last_error()
        assert b"ftl_mlp_forward" in err and b"null" in err and err.endswith(word), (word, err)


def test_the_net_is_refused_as_ftl_mlp_act_refuses_it(lib, handle):
    h = handle
    own = (b"null", b"last weight set", b"H * W", b"head width")      # not the net's own, worded for rows, or not refused here at all
    seen = 0
    for net, code, msg in A._bad_nets():
        if msg in (b"H * W", b"head width"):
            continue
        assert _fwd(lib, h, net=net) == code, msg
        err = lib.ftl_last_error()
        assert msg in err, (msg, err)
        if msg not in own:                                             # the very message of ftl_mlp_act
            assert A._act(lib, h, net=net) == code and lib.ftl_last_error() == err, (msg, err)
            seen += 1
    assert seen >= 9
    for bad in (2, -1, 7, 1 << 30):
        net = A._net(activation=bad)
        assert _fwd(lib, h, net=net) == abi.FTL_E_INVALID and b"activation" in lib.ftl_last_error(), bad
        err = lib.ftl_last_error()
        assert A._act(lib, h, net=net) == abi.FTL_E_INVALID and lib.ftl_last_error() == err
    for good in (abi.FTL_MLP_ACT_RELU, abi.FTL_MLP_ACT_TANH):
        assert _passes_all_but_the_last(lib, h, net=A._net(activation=good)), lib.ftl_last_error()


def test_any_head_width_and_no_policy_obs_rule(lib, handle):
    h = handle
    for widths in ((W0, 64, 3), (W0, 64, 256), (W0, 256), (W0, 64, 64, 1), (7, 1), (W0 - 1, 64, 2), (4096, 256, 256, 256, 256)):
        assert _passes_all_but_the_last(lib, h, net=A._net(widths)), (widths, lib.ftl_last_error())
    for widths in ((W0, 64, 3), (W0, 64, 256)):                        # the policy stack does refuse these, for their width
        assert A._act(lib, h, net=A._net(widths)) == abi.FTL_E_INVALID and b"head width" in lib.ftl_last_error()
    assert _fwd(lib, h, net=A._net((W0, 64, 257))) == abi.FTL_E_UNSUPPORTED and b"FTL_MLP_MAX_WIDTH" in lib.ftl_last_error()
    assert _fwd(lib, h, net=A._net((W0, 64, 0))) == abi.FTL_E_INVALID and b"at least 1" in lib.ftl_last_error()


def test_the_last_row_picks_the_last_set(lib, handle):
    h = handle
    for kw, n, ok in ((dict(n_sets=2, envs_per_set=3), 6, True), (dict(n_sets=2, envs_per_set=3), 7, False),
                      (dict(n_sets=3, envs_per_set=4, env_first=7), 5, True), (dict(n_sets=3, envs_per_set=4, env_first=7), 6, False),
                      (dict(n_sets=1, envs_per_set=40), 40, True), (dict(n_sets=1, envs_per_set=40), 41, False),
                      (dict(n_sets=1, envs_per_set=1 << 30), 1 << 24, True)):      # the handle's own env count plays no part
        if ok:
            assert _passes_all_but_the_last(lib, h, net=A._net(**kw), n=n), (kw, n, lib.ftl_last_error())
        else:
            assert _fwd(lib, h, net=A._net(**kw), n=n) == abi.FTL_E_INVALID, (kw, n)
            assert b"last row" in lib.ftl_last_error() and b"last weight set" in lib.ftl_last_error()


def test_counts_strides_and_alignment(lib, handle):
    h = handle
    for kw in (dict(n_blocks=0), dict(n_blocks=-1), dict(n=0), dict(n=-3)):
        assert _fwd(lib, h, xb=4096, yb=4096, **kw) == abi.FTL_E_INVALID, kw
        assert b"n_blocks and n" in lib.ftl_last_error()
    assert _fwd(lib, h, n_blocks=65536) == abi.FTL_E_UNSUPPORTED and b"65,535" in lib.ftl_last_error()
    assert _fwd(lib, h, n_blocks=1 << 30) == abi.FTL_E_UNSUPPORTED
    assert _passes_all_but_the_last(lib, h, n_blocks=65535) and _passes_all_but_the_last(lib, h, n_blocks=1)
    big = A._net(n_sets=1, envs_per_set=1 << 30)
    assert _fwd(lib, h, net=big, n=1 << 30) == abi.FTL_E_UNSUPPORTED and b"tiles" in lib.ftl_last_error()      # 2^25 tiles of 256 threads
    assert _passes_all_but_the_last(lib, h, net=big, n=((1 << 24) - 1) * 32)
    xb, yb = N * W0 * 4, N * 2 * 4
    for kw, word in ((dict(xb=xb - 4), b"x_block_bytes"), (dict(xb=xb + 2), b"x_block_bytes"), (dict(xb=0), b"x_block_bytes"),
                     (dict(xb=-xb), b"x_block_bytes"), (dict(yb=yb - 4), b"y_block_bytes"), (dict(yb=yb + 1), b"y_block_bytes"),
                     (dict(yb=0), b"y_block_bytes"), (dict(x=FAKE + 2), b"x must be 4-byte aligned"), (dict(x=FAKE + 1), b"x must be 4-byte aligned")):
        assert _fwd(lib, h, **kw) == abi.FTL_E_INVALID, kw
        assert word in lib.ftl_last_error(), (kw, lib.ftl_last_error())
    for y in (2 * FAKE + 1, 2 * FAKE + 2, 2 * FAKE + 3):
        assert _fwd(lib, h, y=y) == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()
    for kw in (dict(xb=xb + 4), dict(xb=10 * xb, yb=3 * yb), dict(yb=yb + 4)):          # padded blocks are fine
        assert _passes_all_but_the_last(lib, h, **kw), (kw, lib.ftl_last_error())
    # a block stride of the single-width head: one float a row
    assert _fwd(lib, h, net=A._net((W0, 64, 1)), yb=N * 4 - 4) == abi.FTL_E_INVALID and b"y_block_bytes" in lib.ftl_last_error()


# ---------------------------------------------------------------- the python surface
def test_python_surface(cfg_b, monkeypatch):
    class FakeObs:
        shape = (6, 5, 36)

    class FakeBatch:
        n, device, policy_obs, cfg = 6, torch.device("cpu"), FakeObs(), cfg_b
    pol = mlp.MlpPolicy(FakeBatch(), (180, 8, 2), n_sets=2, activation="tanh")

    def no_library(*a, **k):
        raise AssertionError("a library call before the argument checks were through")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(mlp, "_device_handle", no_library)
    p = inspect.signature(mlp.forward).parameters
    assert list(p) == ["widths", "params", "x", "activation", "out"] and p["activation"].default == "relu" and p["out"].default is None
    p = inspect.signature(mlp.MlpPolicy.forward).parameters
    assert list(p)[1:] == ["x", "out"] and p["out"].default is None
    p = inspect.signature(mlp.Critic.__init__).parameters
    assert list(p)[1:] == ["widths", "n_sets", "activation", "params", "device"]
    assert [p[k].default for k in list(p)[2:]] == [1, "tanh", None, None]
    for name in ("values", "load", "module"):
        assert callable(getattr(mlp.Critic, name))
    assert mlp.check_net_widths([180, 64, 7]) == (180, 64, 7)

    widths = (5, 4, 3)
    count = abi.mlp_param_count(widths)
    params, x = torch.zeros(2, count), torch.zeros(3, 6, 5)
    bad = [dict(params=torch.zeros(2, count + 1)), dict(params=torch.zeros(count)), dict(params=torch.zeros(2, count, dtype=torch.float64)),
           dict(params=torch.zeros(2, 2 * count)[:, ::2]), dict(params=torch.zeros(0, count)), dict(params=None),
           dict(x=torch.zeros(3, 6, 5, dtype=torch.float64)), dict(x=torch.zeros(3, 6, 4)), dict(x=torch.zeros(5)), dict(x=None),
           dict(x=torch.zeros(3, 5, 6).transpose(1, 2)), dict(x=torch.zeros(3, 12, 5)[:, ::2]), dict(x=torch.zeros(0, 6, 5)),
           dict(x=torch.zeros(3, 0, 5)), dict(x=torch.zeros(3, 7, 5)),                                  # 2 sets do not divide 7 rows
           dict(x=torch.zeros(3, 6, 5, requires_grad=True)),
           dict(out=torch.zeros(3, 6, 4)), dict(out=torch.zeros(3, 6)), dict(out=torch.zeros(3, 6, 3, dtype=torch.float64)),
           dict(out=torch.zeros(3, 6, 6)[:, :, ::2]), dict(out=torch.zeros(18, 3)), dict(activation="gelu"), dict(activation=1),
           dict(widths=(5,)), dict(widths=(5, 0, 3)), dict(widths=(4, 4, 3))]
    for over in bad:
        kw = dict(dict(widths=widths, params=params, x=x), **over)
        with pytest.raises(ValueError):
            mlp.forward(**kw)
    with pytest.raises(ValueError, match="divide"):
        mlp.forward(widths, params, torch.zeros(3, 7, 5))
    for w, xs in (((5, 257, 3), (2, 5)), ((4097, 3), (2, 4097)), ((5, 4, 4, 4, 4, 3), (2, 5))):
        with pytest.raises(NotImplementedError):
            mlp.forward(w, torch.zeros(1, 1), torch.zeros(*xs))
    with pytest.raises(NotImplementedError, match="blocks"):
        mlp.forward((2, 1), torch.zeros(1, 3), torch.zeros(257, 256, 1, 2))
    with pytest.raises(ValueError, match="GPU"):                               # every argument fine but the device: still no library call
        mlp.forward(widths, params, x)
    with pytest.raises(ValueError, match="GPU"):
        mlp.forward(widths, params, x, "tanh", torch.zeros(3, 6, 3))

    # Critic
    for w in ((5, 4, 3), (5, 2), (5,)):
        with pytest.raises(ValueError):
            mlp.Critic(w, device="cpu")
    with pytest.raises(NotImplementedError):
        mlp.Critic((5, 257, 1), device="cpu")
    with pytest.raises(ValueError, match="activation"):
        mlp.Critic((5, 4, 1), activation="gelu", device="cpu")
    with pytest.raises(ValueError, match="n_sets"):
        mlp.Critic((5, 4, 1), n_sets=0, device="cpu")
    with pytest.raises(ValueError, match="params"):
        mlp.Critic((5, 4, 1), n_sets=2, params=torch.zeros(1, abi.mlp_param_count((5, 4, 1))))
    crit = mlp.Critic((5, 4, 1), n_sets=2, device="cpu")
    assert crit.activation == "tanh" and tuple(crit.params.shape) == (2, 29) and crit.params.dtype == torch.float32 and not crit.params.any()
    with pytest.raises(ValueError, match="out"):
        crit.values(torch.zeros(3, 6, 5), out=torch.zeros(3, 5))
    with pytest.raises(ValueError, match="GPU"):
        crit.values(torch.zeros(3, 6, 5))
    with pytest.raises(ValueError, match="GPU"):
        crit.values(torch.zeros(3, 6, 5), out=torch.zeros(3, 6))
    with pytest.raises(ValueError):
        crit.values(torch.zeros(3, 7, 5))

    # MlpPolicy.forward: the policy's own widths, sets and activation, the batch's N
    for xs in ((3, 5, 180), (180,), (3, 12, 180)):
        with pytest.raises(ValueError, match="N = 6"):
            pol.forward(torch.zeros(*xs))
    with pytest.raises(ValueError):
        pol.forward(torch.zeros(3, 6, 179))
    with pytest.raises(ValueError, match="GPU"):
        pol.forward(torch.zeros(3, 6, 180))


# ---------------------------------------------------------------- Critic: load / module round trip, and the loaded row under the twin
def test_critic_round_trip_and_the_twin_within_the_derived_bound():
    widths = (180, 64, 1)
    torch.manual_seed(11)
    module = mlp.torch_module(widths, "tanh")
    w, act, row = mlp.params_from_torch(module)
    assert (w, act) == (widths, "tanh")
    crit = mlp.Critic(widths, n_sets=2, device="cpu")
    assert crit.load(module) is crit
    assert torch.equal(crit.params[0], row) and torch.equal(crit.params[1], row)             # every set
    for s in (0, 1):
        w2, act2, row2 = mlp.params_from_torch(crit.module(s))
        assert (w2, act2) == (widths, "tanh") and torch.equal(row2, row)
    other = mlp.torch_module(widths, "tanh")
    crit.load(other, 1)                                                                      # one set
    assert torch.equal(crit.params[0], row) and torch.equal(crit.params[1], mlp.params_from_torch(other)[2]) and not torch.equal(crit.params[1], row)
    for bad in (mlp.torch_module((180, 32, 1), "tanh"), mlp.torch_module(widths, "relu"), mlp.torch_module((180, 64, 2), "tanh")):
        with pytest.raises(ValueError):
            crit.load(bad)
    with pytest.raises(IndexError):
        crit.load(module, 2)
    with pytest.raises(IndexError):
        crit.module(2)
    # the twin on the loaded row against float64, inside the bound tests/test_mlp_tanh_host.py derives from the operation count
    x = torch.randn(24, widths[0])
    p = crit.params.numpy()
    y = MT.population_raw(p, widths, x.numpy(), 12)                                          # rows 0 .. 11 under set 0, 12 .. 23 under set 1
    for s in (0, 1):
        rows = slice(12 * s, 12 * s + 12)
        again, y64, bound = TH._f64_and_bound(p[s], widths, x.numpy()[rows])
        assert np.array_equal(again.view(np.uint32), y[rows].view(np.uint32))
        err = np.abs(y[rows].astype(np.float64) - y64)
        print("set %d: max error %.3e, bound there %.3e, largest bound %.3e" % (s, err.max(), bound.flat[err.argmax()], bound.max()))
        assert np.isfinite(y64).all() and (err <= bound).all(), (s, float((err - bound).max()))
