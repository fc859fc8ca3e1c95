"""CPU checks of the recurrent net on a recorded sequence (include/ftl.h: ``ftl_rnn_forward``; ``rnn.forward``,
``RecurrentPolicy.forward``, ``rnn.RecurrentCritic``): the export and the mirror of ``ftl_rnn_sequence`` against the header compiled for
the host, every refusal that comes before any device work -- on a handle that never got a state, and never with a call that would pass
them all, so nothing here can launch --, the Python argument checks on CPU tensors with the library patched out, the sequence twin
(tests/rnn_seq_numpy.py) against ``torch.nn.LSTMCell`` in float64, and the wrong variants of the twin on the inputs of the GPU cases."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mlp_numpy as M
import rnn_numpy as R
import rnn_seq_numpy as RS
import test_mlp_abi as A
import test_rnn_abi as RA
from continiousenvironment_follower_leader_amd import _lib, abi, mlp, rnn
from test_mlp_abi import cfg_b, handle, lib  # noqa: F401  (fixtures)

ROOT = A.ROOT
FAKE, N, W0 = A.FAKE, A.N, A.W0
BOTH = RA.BOTH
LAST = b"head must be 4-byte aligned"       # the last check of ftl_rnn_forward: a call refused with it has passed every other one
F = np.float32


def _seq(widths=(W0, 64, 64, 2), cell=64, n=N, **over):
    A_ = widths[-1]
    s = abi.RnnSequence()
    s.obs, s.action, s.reward, s.kind, s.reward0, s.head = FAKE, 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE, 6 * FAKE
    s.obs_block_bytes, s.action_block_bytes = n * widths[0] * 4, n * (16 if A_ == 2 else 8 if A_ == 1 else 4)
    s.reward_block_bytes, s.kind_block_bytes, s.head_block_bytes, s.h_block_bytes = n * 8, n, n * A_ * 4, n * cell * 4
    for k, v in over.items():
        setattr(s, k, v)
    A._KEEP.append(s)
    return s


def _fwd(lib, h, net="x", seq="x", n_blocks=3, n=N):
    net, seq = RA._net() if net == "x" else net, _seq(n=n) if seq == "x" else seq
    return lib.ftl_rnn_forward(h, C.byref(net) if net is not None else None, n_blocks, n, C.byref(seq) if seq is not None else None, None)


def _passes_all_but_the_last(lib, handle_, net="x", n_blocks=3, n=N, widths=(W0, 64, 64, 2), cell=64, **over):
    """The call with a misaligned head: FTL_E_INVALID with the message of the last check, so every check before it let the call pass."""
    rc = _fwd(lib, handle_, net=net, seq=_seq(widths, cell, n, **dict(over, head=6 * FAKE + 1)), n_blocks=n_blocks, n=n)
    return rc == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()


# ---------------------------------------------------------------- the export and the mirror
def test_symbol_declared_exported_and_listed(lib):
    hdr = A._header()
    for s in ("ftl_rnn_forward", "ftl_sizeof_rnn_sequence"):
        assert re.search(r"\b%s\s*\(" % s, hdr) and hasattr(lib, s) and s in _lib.EXPORTS, s
    assert lib.ftl_rnn_forward.restype is C.c_int and len(lib.ftl_rnn_forward.argtypes) == 6
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no struct changed
    assert C.sizeof(abi.Rnn) == lib.ftl_sizeof_rnn() and abi.FTL_RNN_MAX_CELL == 128
    src = open(os.path.join(ROOT, "continiousenvironment_follower_leader_amd", "csrc", "ftl_rnn.hpp")).read()
    assert re.search(r"__global__[^;{]*\bftl_rnn_forward_kernel\s*\(", src) and re.search(r"__global__[^;{]*\bftl_rnn_kernel\s*\(", src)


def test_mirror_matches_the_header(lib, tmp_path):
    struct, mirror = "ftl_rnn_sequence", abi.RnnSequence
    names = [f[0] for f in mirror._fields_]
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), A._header(), re.S).group(1)
    declared = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert declared == names
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ftl.h"', "int main(void) {", '    printf("%%zu\\n", sizeof(%s));' % struct]
    src += ['    printf("%%zu\\n", offsetof(%s, %s));' % (struct, n) for n in names]
    src += ["    return 0;", "}"]
    (tmp_path / "off.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "off.cpp"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(mirror) == lib.ftl_sizeof_rnn_sequence()
    assert got[1:] == [getattr(mirror, n).offset for n in names]


# ---------------------------------------------------------------- refusals before any device work
def test_null_arguments_are_named(lib, handle):
    h = handle
    for kw, hh, word in ((dict(), None, b": h"), (dict(net=None), h, b": net"), (dict(net=RA._net(params=None)), h, b"net->params"),
                         (dict(seq=None), h, b": seq"), (dict(seq=_seq(obs=None)), h, b"seq->obs"), (dict(seq=_seq(head=None)), h, b"seq->head"),
                         (dict(seq=_seq(kind=None)), h, b"seq->kind"), (dict(seq=_seq(action=None)), h, b"seq->action"),
                         (dict(seq=_seq(reward=None)), h, b"seq->reward")):
        assert _fwd(lib, hh, **kw) == abi.FTL_E_INVALID, word
        err = lib.ftl_last_error()
        assert b"ftl_rnn_forward" in err and b"null" in err and word in err, (word, err)
    # what the net does not read may be NULL; a single block reads no record at all
    assert _passes_all_but_the_last(lib, h, net=RA._net(flags=abi.FTL_RNN_PREV_REWARD), action=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, net=RA._net(flags=abi.FTL_RNN_PREV_ACTION), reward=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, net=RA._net(flags=0), action=None, reward=None, reward0=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, n_blocks=1, action=None, reward=None, kind=None, reward0=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, reward0=None, h=7 * FAKE, state_out=8 * FAKE, state_at=2), lib.ftl_last_error()


def test_the_net_is_refused_as_ftl_rnn_act_refuses_it(lib, handle):
    h = handle
    own = (b"null", b"last weight set", b"H * W")                      # not the net's own, worded for rows, or not refused here at all
    seen = 0
    for net, code, msg in RA._bad_nets():
        if msg == b"H * W":
            assert _passes_all_but_the_last(lib, h, net=net, widths=(W0 + 1, 8, 2)), lib.ftl_last_error()      # policy_obs plays no part
            continue
        assert _fwd(lib, h, net=net) == code, msg
        err = lib.ftl_last_error()
        assert msg in err, (msg, err)
        if msg not in own:                                             # the very message of ftl_rnn_act
            assert RA._act(lib, h, net=net) == code and lib.ftl_last_error() == err, (msg, err)
            seen += 1
    assert seen >= 16
    assert _fwd(lib, h, net=RA._net(envs_per_set=N - 1)) == abi.FTL_E_INVALID and b"the last row" in lib.ftl_last_error()
    for bad in (abi.FTL_MLP_ACT_TANH, 2, -1):                          # the trunk is ReLU: the existing message
        net = RA._net(activation=bad)
        assert _fwd(lib, h, net=net) == abi.FTL_E_UNSUPPORTED and b"trunk is ReLU" in lib.ftl_last_error(), bad
        err = lib.ftl_last_error()
        assert RA._act(lib, h, net=net) == abi.FTL_E_UNSUPPORTED and lib.ftl_last_error() == err
    for cell in (129, 256):
        assert _fwd(lib, h, net=RA._net(cell=cell)) == abi.FTL_E_UNSUPPORTED and b"FTL_RNN_MAX_CELL" in lib.ftl_last_error()
    # the limits and the other heads pass
    for widths, cell, flags in (((W0, 256, 256, 256, 5), 128, BOTH), ((W0, 64, 1), 1, 0), ((65, 20, 5), 33, 1), ((4096, 8, 1), 128, 2)):
        assert _passes_all_but_the_last(lib, h, net=RA._net(widths, cell, flags), widths=widths, cell=cell), (widths, lib.ftl_last_error())


def test_the_last_row_picks_the_last_set(lib, handle):
    h = handle
    for kw, n, ok in ((dict(n_sets=2, envs_per_set=3), 6, True), (dict(n_sets=2, envs_per_set=3), 7, False),
                      (dict(n_sets=3, envs_per_set=4, env_first=7), 5, True), (dict(n_sets=3, envs_per_set=4, env_first=7), 6, False),
                      (dict(n_sets=1, envs_per_set=40), 40, True), (dict(n_sets=1, envs_per_set=40), 41, False)):      # the handle's env count plays no part
        if ok:
            assert _passes_all_but_the_last(lib, h, net=RA._net(**kw), n=n), (kw, n, lib.ftl_last_error())
        else:
            assert _fwd(lib, h, net=RA._net(**kw), n=n) == abi.FTL_E_INVALID, (kw, n)
            assert b"last row" in lib.ftl_last_error() and b"last weight set" in lib.ftl_last_error()


def test_counts_strides_and_alignment(lib, handle):
    h = handle
    for kw in (dict(n_blocks=0), dict(n_blocks=-1), dict(n=0), dict(n=-3)):
        assert _fwd(lib, h, seq=_seq(), **kw) == abi.FTL_E_INVALID, kw
        assert b"n_blocks and n" in lib.ftl_last_error()
    assert _fwd(lib, h, n_blocks=65536) == abi.FTL_E_UNSUPPORTED and b"65,535" in lib.ftl_last_error()
    assert _fwd(lib, h, n_blocks=1 << 30) == abi.FTL_E_UNSUPPORTED
    assert _passes_all_but_the_last(lib, h, n_blocks=65535) and _passes_all_but_the_last(lib, h, n_blocks=1)
    big = RA._net(n_sets=1, envs_per_set=1 << 30)
    assert _fwd(lib, h, net=big, seq=_seq(n=1 << 30), n=1 << 30) == abi.FTL_E_UNSUPPORTED and b"tiles" in lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, net=big, n=((1 << 24) - 1) * 32)
    ob, ab, rb, kb, hb, cb = N * W0 * 4, N * 16, N * 8, N, N * 2 * 4, N * 64 * 4
    for over, word in ((dict(obs_block_bytes=ob - 4), b"obs_block_bytes"), (dict(obs_block_bytes=ob + 2), b"obs_block_bytes"),
                       (dict(obs_block_bytes=0), b"obs_block_bytes"), (dict(obs_block_bytes=-ob), b"obs_block_bytes"),
                       (dict(action_block_bytes=ab - 8), b"action_block_bytes"), (dict(action_block_bytes=ab + 4), b"action_block_bytes"),
                       (dict(reward_block_bytes=rb - 8), b"reward_block_bytes"), (dict(reward_block_bytes=rb + 4), b"reward_block_bytes"),
                       (dict(kind_block_bytes=kb - 1), b"kind_block_bytes"), (dict(kind_block_bytes=0), b"kind_block_bytes"),
                       (dict(head_block_bytes=hb - 4), b"head_block_bytes"), (dict(head_block_bytes=hb + 1), b"head_block_bytes"),
                       (dict(h=7 * FAKE, h_block_bytes=cb - 4), b"h_block_bytes"), (dict(h=7 * FAKE, h_block_bytes=cb + 2), b"h_block_bytes"),
                       (dict(state_out=8 * FAKE, state_at=3), b"state_at"), (dict(state_out=8 * FAKE, state_at=-1), b"state_at"),
                       (dict(obs=FAKE + 2), b"obs must be 4-byte aligned"), (dict(action=2 * FAKE + 4), b"action not aligned"),
                       (dict(reward=3 * FAKE + 4), b"reward must be 8-byte aligned"), (dict(reward0=5 * FAKE + 4), b"reward0 must be 8-byte aligned"),
                       (dict(h=7 * FAKE + 2), b"h must be 4-byte aligned"), (dict(state_out=8 * FAKE + 2), b"state_out must be 4-byte aligned")):
        assert _fwd(lib, h, seq=_seq(**over)) == abi.FTL_E_INVALID, over
        assert word in lib.ftl_last_error(), (over, lib.ftl_last_error())
    for head in (6 * FAKE + 1, 6 * FAKE + 2, 6 * FAKE + 3):
        assert _fwd(lib, h, seq=_seq(head=head)) == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()
    # padded blocks are fine; state_at is not looked at without state_out; the action element of Discrete(5) is 4 bytes
    for over in (dict(obs_block_bytes=ob + 4), dict(obs_block_bytes=10 * ob, head_block_bytes=3 * hb, kind_block_bytes=kb + 1),
                 dict(action_block_bytes=ab + 8, reward_block_bytes=rb + 8), dict(state_at=99), dict(state_out=8 * FAKE, state_at=0),
                 dict(state_out=8 * FAKE, state_at=2), dict(h=7 * FAKE, h_block_bytes=cb + 4)):
        assert _passes_all_but_the_last(lib, h, **over), (over, lib.ftl_last_error())
    d5 = (W0, 64, 5)
    assert _passes_all_but_the_last(lib, h, net=RA._net(d5), widths=d5, action=2 * FAKE + 4, action_block_bytes=N * 4 + 4), lib.ftl_last_error()
    assert _fwd(lib, h, net=RA._net(d5), seq=_seq(d5, action=2 * FAKE + 2)) == abi.FTL_E_INVALID and b"action not aligned" in lib.ftl_last_error()
    assert _fwd(lib, h, net=RA._net(d5), seq=_seq(d5, action_block_bytes=N * 4 - 4)) == abi.FTL_E_INVALID and b"action_block_bytes" in lib.ftl_last_error()


# ---------------------------------------------------------------- the python surface
def test_python_surface(cfg_b, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("a library call before the argument checks were through")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(rnn, "_device_handle", no_library)
    p = inspect.signature(rnn.forward).parameters
    assert list(p) == ["widths", "cell", "params", "obs", "action", "reward", "kind", "state", "reward0", "prev_action", "prev_reward", "out",
                       "h_out", "state_out", "state_at"]
    assert [p[k].default for k in list(p)[4:]] == [None, None, None, None, None, True, True, None, None, None, 0]
    p = inspect.signature(rnn.RecurrentPolicy.forward).parameters
    assert list(p)[1:3] == ["traj", "reward0"] and p["reward0"].default is None
    p = inspect.signature(rnn.RecurrentCritic.__init__).parameters
    assert list(p)[1:7] == ["widths", "cell", "n_sets", "prev_reward", "params", "device"]
    assert [p[k].default for k in list(p)[3:7]] == [1, True, None, None]
    p = inspect.signature(rnn.RecurrentCritic.values).parameters
    assert list(p)[1:4] == ["traj", "state", "reward0"] and p["state"].default is None and p["reward0"].default is None
    for name in ("cell_weights", "head_weights", "layer", "load_lstm_cell"):
        assert getattr(rnn.RecurrentCritic, name) is getattr(rnn.RecurrentPolicy, name)

    widths, cell, B, n = (5, 4, 2), 3, 4, 6
    Pw, Rw, U, S = abi.rnn_widths(widths, cell, BOTH)
    count = abi.rnn_param_count(widths, cell, BOTH)
    good = dict(widths=widths, cell=cell, params=torch.zeros(2, count), obs=torch.zeros(B, n, 5), action=torch.zeros(B - 1, n, 2, dtype=torch.float64),
                reward=torch.zeros(B - 1, n, dtype=torch.float64), kind=torch.zeros(B - 1, n, dtype=torch.uint8))
    f64, u8 = torch.float64, torch.uint8
    bad = [dict(params=torch.zeros(2, count + 1)), dict(params=torch.zeros(count)), dict(params=torch.zeros(2, count, dtype=f64)),
           dict(params=torch.zeros(2, 2 * count)[:, ::2]), dict(params=torch.zeros(0, count)), dict(params=None),
           dict(prev_action=False), dict(prev_reward=False),                                   # the param count follows the flags
           dict(obs=torch.zeros(B, n, 5, dtype=f64)), dict(obs=torch.zeros(B, n, 4)), dict(obs=torch.zeros(n, 5)), dict(obs=None),
           dict(obs=torch.zeros(B, 5, n).transpose(1, 2)), dict(obs=torch.zeros(0, n, 5)), dict(obs=torch.zeros(B, 0, 5)), dict(obs=torch.zeros(B, 7, 5)),
           dict(obs=torch.zeros(B, n, 5, requires_grad=True)),
           dict(action=None), dict(action=torch.zeros(B - 1, n, 2)), dict(action=torch.zeros(B - 1, n, dtype=f64)), dict(action=torch.zeros(B - 2, n, 2, dtype=f64)),
           dict(action=torch.zeros(B - 1, n, dtype=torch.int32)), dict(action=torch.zeros(B - 1, 2, n, dtype=f64).transpose(1, 2)),
           dict(reward=None), dict(reward=torch.zeros(B - 1, n)), dict(reward=torch.zeros(B - 2, n, dtype=f64)), dict(reward=torch.zeros(B - 1, n + 1, dtype=f64)),
           dict(kind=None), dict(kind=torch.zeros(B - 1, n, dtype=torch.int32)), dict(kind=torch.zeros(B - 2, n, dtype=u8)), dict(kind=torch.zeros(n, dtype=u8)),
           dict(state=torch.zeros(n, S + 1)), dict(state=torch.zeros(n, S, dtype=f64)), dict(state=torch.zeros(n + 1, S)), dict(state=torch.zeros(n, 2 * S)[:, ::2]),
           dict(reward0=torch.zeros(n)), dict(reward0=torch.zeros(n + 1, dtype=f64)), dict(reward0=torch.zeros(n, 1, dtype=f64)),
           dict(out=torch.zeros(B, n, 3)), dict(out=torch.zeros(B, n)), dict(out=torch.zeros(B, n, 2, dtype=f64)), dict(out=torch.zeros(B, n, 4)[:, :, ::2]),
           dict(h_out=torch.zeros(B, n, cell + 1)), dict(h_out=torch.zeros(B, n, cell, dtype=f64)), dict(h_out=torch.zeros(B - 1, n, cell)),
           dict(state_out=torch.zeros(n, S + 1)), dict(state_out=torch.zeros(n, S, dtype=f64)),
           dict(state_out=torch.zeros(n, S), state_at=B), dict(state_out=torch.zeros(n, S), state_at=-1),
           dict(widths=(5, 2)), dict(widths=(5, 0, 2)), dict(widths=(5, 4, 3)), dict(widths=(4, 4, 2)), dict(cell=0)]
    for over in bad:
        with pytest.raises(ValueError):
            rnn.forward(**dict(good, **over))
    with pytest.raises(ValueError, match="divide"):
        rnn.forward(**dict(good, obs=torch.zeros(B, 7, 5)))
    for w, c in (((5, 257, 2), 3), ((4097, 4, 2), 3), ((5, 4, 4, 4, 4, 2), 3), ((5, 4, 2), 129), ((5, 4, 2), 256)):
        with pytest.raises(NotImplementedError):
            rnn.forward(w, c, torch.zeros(1, 1), torch.zeros(2, 2, w[0]))
    with pytest.raises(NotImplementedError, match="blocks"):
        rnn.forward((2, 1, 1), 1, torch.zeros(1, abi.rnn_param_count((2, 1, 1), 1, 0)), torch.zeros(65536, 1, 2), prev_action=False, prev_reward=False,
                    kind=torch.zeros(65535, 1, dtype=u8))
    # every argument fine but the device: still no library call.  The T-block records of a trajectory pass for B = T and B = T + 1, the
    # records may be left out where the net or a single block does not read them
    ok = [dict(), dict(obs=torch.zeros(B - 1, n, 5)), dict(state=torch.zeros(n, S), reward0=torch.zeros(n, dtype=f64), out=torch.zeros(B, n, 2),
                                                         h_out=torch.zeros(B, n, cell), state_out=torch.zeros(n, S), state_at=B - 1),
          dict(obs=torch.zeros(1, n, 5), action=None, reward=None, kind=None),
          dict(params=torch.zeros(2, abi.rnn_param_count(widths, cell, 0)), prev_action=False, prev_reward=False, action=None, reward=None)]
    for over in ok:
        with pytest.raises(ValueError, match="GPU"):
            rnn.forward(**dict(good, **over))

    # RecurrentCritic
    for w in ((5, 4, 2), (5, 4, 5), (5, 1), (5,)):
        with pytest.raises(ValueError):
            rnn.RecurrentCritic(w, 3, device="cpu")
    with pytest.raises(NotImplementedError):
        rnn.RecurrentCritic((5, 257, 1), 3, device="cpu")
    with pytest.raises(NotImplementedError, match="128"):
        rnn.RecurrentCritic((5, 4, 1), 129, device="cpu")
    with pytest.raises(ValueError, match="cell"):
        rnn.RecurrentCritic((5, 4, 1), 0, device="cpu")
    with pytest.raises(ValueError, match="n_sets"):
        rnn.RecurrentCritic((5, 4, 1), 3, n_sets=0, device="cpu")
    with pytest.raises(ValueError, match="params"):
        rnn.RecurrentCritic((5, 4, 1), 3, n_sets=2, params=torch.zeros(1, abi.rnn_param_count((5, 4, 1), 3, 2)))
    crit = rnn.RecurrentCritic((5, 4, 1), 3, n_sets=2, device="cpu")
    assert (crit.P, crit.R, crit.U, crit.S) == abi.rnn_widths((5, 4, 1), 3, abi.FTL_RNN_PREV_REWARD) == (0, 1, 8, 7)
    assert tuple(crit.params.shape) == (2, abi.rnn_param_count((5, 4, 1), 3, 2)) and not crit.params.any()
    Wg, bg = crit.cell_weights()
    Wy, by = crit.head_weights()
    W, b = crit.layer(0)
    assert tuple(Wg.shape) == (2, 8, 12) and tuple(bg.shape) == (2, 12) and tuple(Wy.shape) == (2, 3, 1) and tuple(by.shape) == (2, 1)
    assert tuple(W.shape) == (2, 5, 4) and tuple(b.shape) == (2, 4)
    lstm = torch.nn.LSTMCell(5, 3)
    crit.load_lstm_cell(1, lstm)
    assert torch.equal(Wg[1, :5], lstm.weight_ih.detach().t()) and torch.equal(Wg[1, 5:], lstm.weight_hh.detach().t()) and not Wg[0].any()
    with pytest.raises(ValueError, match="inputs"):
        crit.load_lstm_cell(0, torch.nn.LSTMCell(6, 3))
    T = 3
    traj = mlp.Trajectory(torch.zeros(T + 1, n, 5), torch.zeros(T, n, 2), torch.zeros(T, n, 2, dtype=f64), torch.zeros(T, n, dtype=f64),
                          torch.zeros(T, n, dtype=u8))
    with pytest.raises(ValueError, match="GPU"):
        crit.values(traj)
    with pytest.raises(ValueError, match="out"):
        crit.values(traj, out=(torch.zeros(T, n), torch.zeros(n, crit.S)))
    with pytest.raises(ValueError, match="state"):
        crit.values(traj, state=torch.zeros(n, crit.S + 1), out=(torch.zeros(T + 1, n), torch.zeros(n, crit.S)))
    with pytest.raises(ValueError):
        crit.values(torch.zeros(T + 1, n, 5))
    # prev_action: only where an action is one float64 (a constant_follower_speed config)
    crit_a = rnn.RecurrentCritic((5, 4, 1), 3, device="cpu", prev_action=True)
    assert (crit_a.P, crit_a.S) == (1, 8)
    with pytest.raises(ValueError, match="constant_follower_speed"):
        crit_a.values(traj)
    traj.action = torch.zeros(T, n, dtype=f64)
    with pytest.raises(ValueError, match="GPU"):
        crit_a.values(traj)

    # RecurrentPolicy.forward: the policy's own net on its own trajectory
    class FakeObs:
        shape = (6, 5, 36)

    class FakeBatch:
        n, device, policy_obs, cfg = 6, torch.device("cpu"), FakeObs(), cfg_b
    monkeypatch.undo()
    pol = rnn.RecurrentPolicy(FakeBatch(), (180, 8, 2), 4, n_sets=2)
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(rnn, "_device_handle", no_library)
    tr = mlp.Trajectory(torch.zeros(T + 1, 6, 180), torch.zeros(T, 6, 2), torch.zeros(T, 6, 2, dtype=f64), torch.zeros(T, 6, dtype=f64),
                        torch.zeros(T, 6, dtype=u8))
    with pytest.raises(ValueError, match="state"):
        pol.forward(tr)
    tr.state = torch.zeros(1, 6, pol.S)
    with pytest.raises(ValueError, match="GPU"):
        pol.forward(tr)
    with pytest.raises(ValueError, match="reward0"):
        pol.forward(tr, torch.zeros(6))
    with pytest.raises(ValueError, match="out"):
        pol.forward(tr, out=torch.zeros(T + 1, 6, 2))
    tr.obs = torch.zeros(T + 1, 5, 180)
    with pytest.raises(ValueError, match="N = 6"):
        pol.forward(tr)


# ---------------------------------------------------------------- the twin against torch.nn.LSTMCell in float64
@pytest.mark.parametrize("scale", [0.1, 0.5])
def test_sequence_twin_against_torch_lstmcell(scale):
    """A 64-unit cell over 12 blocks with ``kind`` all STEP: the sequence twin's heads against torch.nn.LSTMCell (and Linear) in float64
    on the same weights and the same record.  The bound is the measured one of tests/test_rnn_host.py: 8 x the largest head difference
    between the twin and a float64 numpy evaluation of the same net with libm on these inputs (DESIGN 8.21 records the values)."""
    rng = np.random.default_rng(int(scale * 100) + 3)
    widths, cell, flags, n, B = (24, 32, 2), 64, BOTH, 8, 12
    P, Rw, U, S = R.dims(widths, cell, flags)
    p = (rng.standard_normal(R.param_count(widths, cell, flags)) * scale).astype(F)
    obs = rng.random((B, n, widths[0]), dtype=F)
    action, reward, reward0 = rng.standard_normal((B - 1, n, 2)) * 0.7, rng.standard_normal((B - 1, n)), rng.standard_normal(n)
    kind = np.zeros((B - 1, n), np.uint8)
    state = np.zeros((n, S), F)
    got = RS.forward(p[None], widths, cell, flags, obs, state, action, reward, kind, reward0)
    assert (got["read"][1:, :, -1] == 1).all() and (got["read"][0] == 0).all()
    trunk, Wg, bg, Wy, by = R.split(p, widths, cell, flags)
    (W0_, b0), = M.layers(trunk, widths[:-1])
    lin, head = torch.nn.Linear(widths[0], widths[1]).double(), torch.nn.Linear(cell, 2).double()
    lstm = torch.nn.LSTMCell(U - cell, cell).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(W0_.T.astype(np.float64))), lin.bias.copy_(torch.from_numpy(b0.astype(np.float64)))
        head.weight.copy_(torch.from_numpy(Wy.T.astype(np.float64))), head.bias.copy_(torch.from_numpy(by.astype(np.float64)))
        lstm.weight_ih.copy_(torch.from_numpy(Wg[:U - cell].T.astype(np.float64))), lstm.weight_hh.copy_(torch.from_numpy(Wg[U - cell:].T.astype(np.float64)))
        lstm.bias_ih.copy_(torch.from_numpy(bg.astype(np.float64))), lstm.bias_hh.zero_()
    st64 = np.zeros((n, S))
    h_t, c_t = torch.zeros(n, cell, dtype=torch.float64), torch.zeros(n, cell, dtype=torch.float64)
    measured = vs_torch = 0.0
    for b in range(B):
        rew = reward0 if b == 0 else reward[b - 1]
        y64, h64, c64 = R.f64_forward(p, widths, cell, flags, obs[b], st64, rew)
        measured = max(measured, float(np.abs(got["head"][b].astype(np.float64) - y64).max()))
        with torch.no_grad():
            a_prev = torch.from_numpy(got["read"][b][:, 2 * cell:2 * cell + P].astype(np.float64))
            r_prev = torch.from_numpy(np.where(got["read"][b][:, -1] != 0, rew.astype(F), 0).astype(np.float64))[:, None]
            u = torch.cat([torch.relu(lin(torch.from_numpy(obs[b].astype(np.float64)))), a_prev, r_prev], 1)
            h_t, c_t = lstm(u, (h_t, c_t))
            vs_torch = max(vs_torch, float((head(h_t) - torch.from_numpy(got["head"][b].astype(np.float64))).abs().max()))
        if b + 1 < B:
            st64 = np.concatenate([h64, c64, got["read"][b + 1][:, 2 * cell:].astype(np.float64)], 1)      # (the recorded action and live, as a replay has them)
    print("scale %g: sequence twin vs float64 libm %.3e, vs torch float64 %.3e, bound %.3e" % (scale, measured, vs_torch, 8 * measured))
    assert 0 < measured < 1e-4
    assert vs_torch <= 8 * measured
    # the sequence twin is rnn_numpy.decide block by block (bit for bit)
    st = state
    lo, hi = np.array([0.0, -1.0]), np.array([1.0, 1.0])
    for b in range(3):
        r = R.decide(p, widths, cell, flags, obs[b], st, reward0 if b == 0 else reward[b - 1], np.zeros(n, bool), M.BOX2, lo, hi)
        assert np.array_equal(r["head"].view(np.uint32), got["head"][b].view(np.uint32)) and np.array_equal(r["read"].view(np.uint32), got["read"][b].view(np.uint32))
        st = r["state"].copy()
        st[:, 2 * cell:2 * cell + P] = action[b].astype(F)         # the record's action in place of the head map's
        assert np.array_equal(st[:, :2 * cell].view(np.uint32), got["read"][b + 1][:, :2 * cell].view(np.uint32))


# ---------------------------------------------------------------- the GPU cases can see every rule
def test_wrong_variants_change_the_heads_on_the_gpu_inputs():
    """On the synthetic inputs of tests/test_gpu_rnn_forward.py (a subset of its nets: the patterns do not depend on the net) each wrong
    variant of the twin -- no wipe after VOID, r_prev fed whatever live is, libm's exp -- changes at least one head."""
    checked = 0
    for (trunk, cell), A_, w0, n, n_sets in ((((20,), 32), 2, 65, 15, 1), (((33,), 63), 5, 65, 33, 3), (((64,), 1), 1, 65, 15, 1)):
        for flags in (BOTH, 0, R.PREV_ACTION, R.PREV_REWARD):
            case = RS.synthetic(trunk, cell, A_, w0, n, n_sets, flags)
            RS.assert_patterns(case["rec"], case["state"])
            args = (case["params"], case["widths"], cell, flags, case["rec"]["obs"], case["state"], case["rec"]["action"], case["rec"]["reward"],
                    case["rec"]["kind"], case["rec"]["reward0"], n // n_sets)
            exact = RS.forward(*args)["head"].view(np.uint32)
            variants = [dict(wipe=False), dict(exp=R.exp_libm)] + ([dict(gate_reward=False)] if flags & R.PREV_REWARD else [])
            for v in variants:
                wrong = RS.forward(*args, **v)["head"].view(np.uint32)
                assert (wrong != exact).any(), (cell, A_, flags, v)
                if "gate_reward" in v:
                    assert (wrong[0] != exact[0]).any() and (wrong[1:] != exact[1:]).any()       # at block 0 (live 0 in the state) and after a VOID
                checked += 1
    assert checked >= 30
