"""C-ABI checks of the recurrent policy that need no GPU (include/ftl.h: ftl_rnn_param_count, ftl_rnn_act, ftl_rollout_rnn,
ftl_collect_rnn): exports, the ctypes mirrors of ftl_rnn and ftl_rnn_collect_buffers against the header compiled for the host, the
constants and flags, the parameter count against a by-hand sum, every refusal that comes before any device work with its message, and
the wrapper's refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

import test_collect_abi as CA
import test_mlp_abi as A
from continiousenvironment_follower_leader_amd import _lib, abi
from test_mlp_abi import cfg_b, handle, lib  # noqa: F401  (fixtures)

ROOT = A.ROOT
SYMBOLS = ("ftl_sizeof_rnn", "ftl_sizeof_rnn_collect_buffers", "ftl_rnn_param_count", "ftl_rnn_act", "ftl_rollout_rnn", "ftl_collect_rnn")
FAKE, N, W0 = A.FAKE, A.N, A.W0
BOTH = abi.FTL_RNN_PREV_ACTION | abi.FTL_RNN_PREV_REWARD


def _net(widths=(W0, 64, 64, 2), cell=64, flags=BOTH, **over):
    net = abi.Rnn()
    net.params, net.n_sets, net.n_layers, net.env_first, net.envs_per_set = FAKE, 1, len(widths) - 2, 0, N
    for l, w in enumerate(widths[:abi.FTL_MLP_MAX_LAYERS + 1]):
        net.width[l] = w
    net.cell, net.flags, net.state = cell, flags, FAKE
    ok = 1 <= cell <= abi.FTL_RNN_MAX_CELL and 3 <= len(widths) <= abi.FTL_MLP_MAX_LAYERS + 1 and not flags & ~3
    net.set_stride = abi.rnn_param_count(widths, cell, flags) if ok else 1 << 40
    net.state_stride = abi.rnn_widths(widths, cell, flags & 3)[3] if len(widths) >= 2 else 1
    for k, v in over.items():
        setattr(net, k, v)
    A._KEEP.append(net)
    return net


def _buffers(widths=(W0, 64, 64, 2), cell=64, flags=BOTH, T=3, **over):
    rb = abi.RnnCollectBuffers()
    src = CA._buffers(widths)
    for name, _ in abi.CollectBuffers._fields_:
        setattr(rb.b, name, getattr(src, name))
    rb.state, rb.state_step_bytes, rb.state_steps = FAKE, N * abi.rnn_widths(widths, cell, flags)[3] * 4, T
    for k, v in over.items():
        setattr(rb.b if hasattr(rb.b, k) else rb, k, v)
    A._KEEP.append(rb)
    return rb


def _act(lib, h, out="x", net="x", noise=None, sigma=None, head=FAKE, obs=FAKE, state_rec=None, action=FAKE, flags=0):
    out, net = A._outputs() if out == "x" else out, _net() if net == "x" else net
    return lib.ftl_rnn_act(h, C.byref(out) if out is not None else None, C.byref(net) if net is not None else None, noise, sigma, head, obs,
                           state_rec, action, flags, None)


def _rollout(lib, h, out="x", ro="x", net="x", T=3, actions=None, step_bytes=0, flags=0):
    out, ro, net = A._outputs() if out == "x" else out, A._ro() if ro == "x" else ro, _net() if net == "x" else net
    return lib.ftl_rollout_rnn(h, T, 0.9, C.byref(out) if out is not None else None, C.byref(ro) if ro is not None else None,
                               C.byref(net) if net is not None else None, actions, step_bytes, flags, None)


def _collect(lib, h, out="x", net="x", b="x", T=3, flags=abi.FTL_STEP_NEXT_RESET):
    out, net, b = A._outputs() if out == "x" else out, _net() if net == "x" else net, _buffers(T=T) if b == "x" else b
    return lib.ftl_collect_rnn(h, T, C.byref(out) if out is not None else None, C.byref(net) if net is not None else None,
                               C.byref(b) if b is not None else None, flags, None)


def _bad_nets():
    """(net, code, a word of the message) of every refusal of the net and its state."""
    I, U = abi.FTL_E_INVALID, abi.FTL_E_UNSUPPORTED
    return [(_net(params=None), I, b"null"),
            (_net(n_layers=0), I, b"n_layers"),
            (_net((W0, 8, 8, 8, 8, 2)[:5], n_layers=4), U, b"trunk layers"),
            (_net((W0, 0, 2)), I, b"width"),
            (_net((W0, 257, 2)), U, b"FTL_MLP_MAX_WIDTH"),
            (_net((4097, 8, 2)), U, b"FTL_MLP_MAX_IN"),
            (_net(cell=0), I, b"cell"),
            (_net(cell=129), U, b"FTL_RNN_MAX_CELL"),
            (_net(cell=256), U, b"FTL_RNN_MAX_CELL"),
            (_net(flags=4), I, b"ftl_rnn.flags"),
            (_net((W0, 8, 3)), I, b"head width"),
            (_net(params=FAKE + 2), I, b"4-byte aligned"),
            (_net(set_stride=abi.rnn_param_count((W0, 64, 64, 2), 64, BOTH) - 1), I, b"set_stride"),
            (_net(n_sets=0), I, b"n_sets"),
            (_net(envs_per_set=N - 1), I, b"last weight set"),
            (_net((W0 + 1, 8, 2)), I, b"H * W"),
            (_net(state=None), I, b"state is NULL"),
            (_net(state=FAKE + 2), I, b"state must be 4-byte aligned"),
            (_net(state_stride=2 * 64 + 2), I, b"state_stride below S"),
            (_net(flags=0, state_stride=2 * 64), I, b"state_stride below S")]


# ---------------------------------------------------------------- exports, the mirrors, the constants
def test_symbols_declared_exported_and_listed(lib):
    hdr = A._header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s
    for f in ("ftl_rnn.hpp", "ftl_rnn_math.hpp"):
        assert any(s.endswith(f) for s in _lib.SOURCES), f
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no existing struct changed
    for name in ("FTL_RNN_MAX_CELL", "FTL_RNN_PREV_ACTION", "FTL_RNN_PREV_REWARD", "FTL_RNN_ZERO_ON_OUT_DONE"):
        assert int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, hdr).group(1)) == getattr(abi, name), name
    assert abi.FTL_RNN_MAX_CELL == 128
    src = open(os.path.join(ROOT, "continiousenvironment_follower_leader_amd", "csrc", "ftl_rnn.hpp")).read()
    assert int(re.search(r"#define\s+FTL_RNN_PASS_CELLS\s+(\d+)", src).group(1)) == abi.FTL_RNN_PASS_CELLS
    assert 4 * abi.FTL_RNN_PASS_CELLS == abi.FTL_MLP_MAX_WIDTH


@pytest.mark.parametrize("struct, mirror", [("ftl_rnn", abi.Rnn), ("ftl_rnn_collect_buffers", abi.RnnCollectBuffers)])
def test_mirror_matches_the_header(lib, tmp_path, struct, mirror):
    names = [f[0] for f in mirror._fields_]
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), A._header(), re.S).group(1)
    declared = []
    for d in body.split(";"):
        if d.strip():
            declared += [re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", part.strip()).group(1) for part in d.split(",")]
    assert declared == names
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ftl.h"', "int main(void) {", '    printf("%%zu\\n", sizeof(%s));' % struct]
    src += ['    printf("%%zu\\n", offsetof(%s, %s));' % (struct, n) for n in names]
    src += ["    return 0;", "}"]
    (tmp_path / "off.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "off.cpp"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(mirror) == getattr(lib, "ftl_sizeof_" + struct[4:])()
    assert got[1:] == [getattr(mirror, n).offset for n in names]
    if struct == "ftl_rnn":                                          # ftl_mlp's fields first, at ftl_mlp's offsets
        assert names[:len(abi.Mlp._fields_)] == [f[0] for f in abi.Mlp._fields_]
        assert all(getattr(abi.Rnn, f[0]).offset == getattr(abi.Mlp, f[0]).offset for f in abi.Mlp._fields_)


def test_param_count(lib):
    def by_hand(w, c, fl):
        A_ = w[-1]
        P, R = (A_ if fl & 1 else 0), (1 if fl & 2 else 0)
        n = sum((a + 1) * b for a, b in zip(w[:-2], w[1:-1]))        # the trunk
        U = w[-2] + P + R + c
        return n + U * 4 * c + 4 * c + c * A_ + A_

    def count(w, c, fl):
        return lib.ftl_rnn_param_count((C.c_int32 * len(w))(*w), len(w) - 2, c, fl)
    for w in ((180, 64, 64, 2), (180, 70, 33, 5), (180, 20, 1), (4096, 256, 256, 256, 5), (7, 1, 2)):
        for c in (1, 63, 64, 65, 128):
            for fl in (0, 1, 2, 3):
                assert count(w, c, fl) == by_hand(w, c, fl) == abi.rnn_param_count(w, c, fl), (w, c, fl)
    assert by_hand((180, 64, 64, 2), 64, 3) == 181 * 64 + 65 * 64 + (64 + 2 + 1 + 64) * 256 + 256 + 64 * 2 + 2
    assert abi.rnn_widths((180, 64, 64, 2), 64, 3) == (2, 1, 131, 131) and abi.rnn_widths((180, 33, 5), 63, 1) == (5, 0, 101, 132)
    for w, c, fl in (((180, 64, 2), 129, 3), ((180, 64, 2), 0, 3), ((180, 64, 2), 256, 3), ((180, 64, 3), 8, 3), ((180, 257, 2), 8, 3),
                     ((180, 8, 8, 8, 8, 2), 8, 3), ((180, 64, 2), 8, 4), ((4097, 8, 2), 8, 0)):
        assert count(w, c, fl) == -1, (w, c, fl)
    assert lib.ftl_rnn_param_count(None, 1, 8, 0) == -1
    assert lib.ftl_rnn_param_count((C.c_int32 * 2)(180, 2), 0, 8, 0) == -1


# ---------------------------------------------------------------- refusals before any device work
def test_act_argument_checks(lib, handle):
    h = handle
    assert _act(lib, None) == abi.FTL_E_INVALID
    assert _act(lib, h, out=None) == abi.FTL_E_INVALID
    assert _act(lib, h, net=None) == abi.FTL_E_INVALID
    assert _act(lib, h, action=None) == abi.FTL_E_INVALID
    for net, code, msg in _bad_nets():
        assert _act(lib, h, net=net) == code, msg
        assert msg in lib.ftl_last_error(), (msg, lib.ftl_last_error())
    assert _act(lib, h, out=A._outputs(policy_obs=None)) == abi.FTL_E_INVALID and b"policy_obs" in lib.ftl_last_error()
    assert _act(lib, h, flags=2) == abi.FTL_E_INVALID and b"FTL_RNN_ZERO_ON_OUT_DONE" in lib.ftl_last_error()
    for widths in ((W0, 8, 2), (W0, 8, 1)):                                     # a Box head with noise but no sigma
        assert _act(lib, h, net=_net(widths), noise=FAKE) == abi.FTL_E_INVALID and b"sigma" in lib.ftl_last_error()
    for kw in (dict(noise=FAKE + 2, sigma=FAKE), dict(noise=FAKE, sigma=FAKE + 1), dict(head=FAKE + 2), dict(obs=FAKE + 3), dict(state_rec=FAKE + 2)):
        assert _act(lib, h, **kw) == abi.FTL_E_INVALID, kw
        assert b"4-byte aligned" in lib.ftl_last_error()
    assert _act(lib, h, action=FAKE + 4) == abi.FTL_E_INVALID and b"action" in lib.ftl_last_error()
    # every argument fine: only the state of the ENV is missing
    for kw in (dict(), dict(noise=FAKE, sigma=FAKE), dict(head=None, obs=None, state_rec=FAKE), dict(flags=abi.FTL_RNN_ZERO_ON_OUT_DONE),
               dict(net=_net((W0, 20, 5), cell=128, flags=1), noise=FAKE), dict(net=_net((W0, 64, 1), cell=1, flags=0)),
               dict(net=_net((W0, 256, 256, 256, 5), cell=128))):
        assert _act(lib, h, **kw) == abi.FTL_E_STATE, (kw, lib.ftl_last_error())
        assert b"ftl_bind_state" in lib.ftl_last_error()


def test_rollout_argument_checks(lib, handle):
    h = handle
    assert _rollout(lib, None) == abi.FTL_E_INVALID
    for kw in (dict(out=None), dict(ro=None), dict(net=None), dict(ro=A._ro(ret=None))):
        assert _rollout(lib, h, **kw) == abi.FTL_E_INVALID, kw
    assert _rollout(lib, h, T=0) == abi.FTL_E_INVALID and b"T must be positive" in lib.ftl_last_error()
    assert _rollout(lib, h, flags=abi.FTL_STEP_NO_SENSORS) == abi.FTL_E_INVALID and b"policy_obs" in lib.ftl_last_error()
    for flags in (abi.FTL_RNN_ZERO_ON_OUT_DONE, abi.FTL_STEP_NEXT_RESET):         # (bit 1 is FTL_STEP_AUTO_RESET to a loop: mode BEFORE has no loop)
        assert _rollout(lib, h, flags=flags) == abi.FTL_E_INVALID, flags
        assert b"no flag" in lib.ftl_last_error()
    for net, code, msg in _bad_nets():
        assert _rollout(lib, h, net=net) == code, msg
        assert msg in lib.ftl_last_error(), (msg, lib.ftl_last_error())
    assert _rollout(lib, h, actions=FAKE, step_bytes=N * 16 - 8) == abi.FTL_E_INVALID and b"step_bytes below" in lib.ftl_last_error()
    assert _rollout(lib, h, actions=FAKE + 4, step_bytes=N * 16) == abi.FTL_E_INVALID and b"aligned" in lib.ftl_last_error()
    for kw in (dict(), dict(actions=FAKE, step_bytes=N * 16)):
        assert _rollout(lib, h, **kw) == abi.FTL_E_STATE and b"ftl_bind_state" in lib.ftl_last_error()


def test_collect_argument_checks(lib, handle):
    h = handle
    assert _collect(lib, None) == abi.FTL_E_INVALID
    for kw in (dict(out=None), dict(net=None), dict(b=None)):
        assert _collect(lib, h, **kw) == abi.FTL_E_INVALID, kw
    for flags, words in CA.REFUSED_FLAGS:                                        # the same flags with the same messages
        assert _collect(lib, h, flags=flags) == abi.FTL_E_INVALID, flags
        for w in words:
            assert w in lib.ftl_last_error(), (flags, w, lib.ftl_last_error())
    assert _collect(lib, h, flags=abi.FTL_RNN_ZERO_ON_OUT_DONE) == abi.FTL_E_INVALID                 # = FTL_STEP_AUTO_RESET: refused
    for T in (0, -2):
        assert _collect(lib, h, T=T) == abi.FTL_E_INVALID and b"T must be positive" in lib.ftl_last_error()
    for net, code, msg in _bad_nets():
        assert _collect(lib, h, net=net) == code, msg
        assert msg in lib.ftl_last_error(), (msg, lib.ftl_last_error())
    for field in ("obs", "head", "action", "reward", "kind", "state"):
        assert _collect(lib, h, b=_buffers(**{field: None})) == abi.FTL_E_INVALID
        assert field.encode() in lib.ftl_last_error() and b"missing" in lib.ftl_last_error()
    assert _collect(lib, h, b=_buffers(state_steps=2)) == abi.FTL_E_INVALID and b"state_steps must be 1 or T" in lib.ftl_last_error()
    assert _collect(lib, h, b=_buffers(state_steps=0)) == abi.FTL_E_INVALID
    S = abi.rnn_widths((W0, 64, 64, 2), 64, BOTH)[3]
    for over in (dict(obs_step_bytes=N * W0 * 4 - 4), dict(kind_step_bytes=N - 1), dict(state_step_bytes=N * S * 4 - 4),
                 dict(noise=FAKE, sigma=FAKE, noise_step_bytes=N * 2 * 4 - 4)):
        assert _collect(lib, h, b=_buffers(**over)) == abi.FTL_E_INVALID, over
        assert b"step_bytes below" in lib.ftl_last_error()
    for over in (dict(obs=FAKE + 2), dict(reward=FAKE + 4), dict(state=FAKE + 2), dict(state_step_bytes=N * S * 4 + 2)):
        assert _collect(lib, h, b=_buffers(**over)) == abi.FTL_E_INVALID, over
        assert b"aligned" in lib.ftl_last_error()
    assert _collect(lib, h, b=_buffers(noise=FAKE)) == abi.FTL_E_INVALID and b"sigma" in lib.ftl_last_error()
    for flags in (0, abi.FTL_STEP_NEXT_RESET):
        for b in (_buffers(), _buffers(noise=FAKE, sigma=FAKE), _buffers(state_steps=1, state_step_bytes=0)):
            assert _collect(lib, h, b=b, flags=flags) == abi.FTL_E_STATE, lib.ftl_last_error()
            assert b"ftl_bind_state" in lib.ftl_last_error()


# ---------------------------------------------------------------- the python surface
def test_python_surface_needs_no_device(cfg_b):
    import inspect
    from continiousenvironment_follower_leader_amd import mlp, rnn
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    p = inspect.signature(rnn.RecurrentPolicy.__init__).parameters
    assert list(p)[1:] == ["batch", "widths", "cell", "n_sets", "params", "prev_action", "prev_reward", "auto_reset"]
    assert p["prev_action"].default is True and p["prev_reward"].default is True and p["auto_reset"].default == "next_step"
    p = inspect.signature(rnn.RecurrentPolicy.collect).parameters
    assert list(p)[1:] == ["T", "noise", "sigma", "auto_reset", "out", "record_state"] and p["record_state"].default is False
    for cls in (VecGame, PipelinedVecGame):
        assert list(inspect.signature(cls.rollout_rnn).parameters)[1:] == ["policy", "T", "gamma", "record"]
        assert list(inspect.signature(cls.collect_rnn).parameters)[1:] == ["policy", "T", "noise", "sigma", "auto_reset", "out", "record_state"]
    assert issubclass(rnn.RecurrentPolicy, mlp.MlpPolicy)
    assert rnn.RecurrentPolicy.rollout is mlp.MlpPolicy.rollout and "rollout" not in vars(rnn.RecurrentPolicy)     # shared, not copied
    assert rnn.RecurrentPolicy._bind is mlp.MlpPolicy._bind and rnn.RecurrentPolicy._collect is mlp.MlpPolicy._collect
    assert rnn.RecurrentCritic.cell_weights is rnn.Net.cell_weights and rnn.RecurrentCritic._hold is rnn.Net._hold

    class FakeBatch:
        n, device, policy_obs = 6, "cpu", None
    FakeBatch.cfg = cfg_b
    for name in ("rollout_rnn", "collect_rnn"):
        with pytest.raises(ValueError, match="RecurrentPolicy of this batch"):
            getattr(VecGame, name)(FakeBatch(), object(), 3)
    R = rnn.RecurrentPolicy
    with pytest.raises(ValueError, match="widths"):
        R(FakeBatch(), (180, 2), 8)
    with pytest.raises(ValueError, match="head"):
        R(FakeBatch(), (180, 8, 5), 8)
    with pytest.raises(NotImplementedError):
        R(FakeBatch(), (180, 8, 8, 8, 8, 2), 8)
    with pytest.raises(NotImplementedError):
        R(FakeBatch(), (180, 257, 2), 8)
    with pytest.raises(NotImplementedError, match="128"):
        R(FakeBatch(), (180, 8, 2), 256)
    with pytest.raises(ValueError, match="cell"):
        R(FakeBatch(), (180, 8, 2), 0)
    with pytest.raises(ValueError, match="auto_reset"):
        R(FakeBatch(), (180, 8, 2), 8, auto_reset="never")
    with pytest.raises(ValueError, match="policy_obs"):
        R(FakeBatch(), (180, 8, 2), 8)
