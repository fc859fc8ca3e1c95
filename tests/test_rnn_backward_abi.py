"""CPU checks of the backward pass of the recurrent net (include/ftl.h: ``ftl_rnn_backward``, ``ftl_sizeof_rnn_backward_workspace``,
``ftl_rnn_gradient``; ``rnn.backward``, ``rnn.Net``): the exports and the struct's mirror against the header compiled for the host, the
workspace query against a by-hand count of groups and spans, every refusal that comes before any device work -- on a handle that never got
a state, and never with a call that would pass them all, so nothing here can launch --, the Python argument checks on CPU tensors with
the library patched out, the wrong variants of the twin (tests/rnn_backward_numpy.py) on the inputs of the GPU cases, the twin's set
independence, and the twin against torch float64 autograd through the replay of INTEGRATION.md."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mlp_numpy as M
import rnn_backward_numpy as RB
import rnn_numpy as R
import rnn_seq_numpy as RS
import test_mlp_abi as A
import test_rnn_abi as RA
import test_rnn_forward_abi as FA
from continiousenvironment_follower_leader_amd import _lib, abi, mlp, rnn
from test_mlp_abi import cfg_b, handle, lib  # noqa: F401  (fixtures)

ROOT = A.ROOT
FAKE, N, W0 = A.FAKE, A.N, A.W0
BOTH = RA.BOTH
LAST = b"grad must be 4-byte aligned"       # the last check of ftl_rnn_backward: a call refused with it has passed every other one
F = np.float32
U32 = 2.0 ** -24
BIG = 1 << 44
# The float32 twin against torch float64 autograd (test_float32_twin_close_to_float64_autograd): the largest error of a gradient tensor
# relative to its largest magnitude, measured over that test's eight cases, is 1.50e-6 (5.2e-7 .. 1.5e-6).  No operation-count bound was
# derived: the error of a block passes through the gate product of every later block, sums of |W| of order 10 here, so a worst-case
# bound grows by that factor a block and says nothing after 12.  8 times the measured value is allowed, a margin for seed-to-seed spread.
F32_MEASURED = 1.5e-6
F32_BOUND = 8 * F32_MEASURED


def _grad(widths=(W0, 64, 64, 2), n=N, **over):
    g = abi.RnnGradient()
    g.dhead, g.grad, g.workspace, g.workspace_bytes = 6 * FAKE, 7 * FAKE, 8 * FAKE, BIG
    g.dhead_block_bytes = n * widths[-1] * 4
    for k, v in over.items():
        setattr(g, k, v)
    A._KEEP.append(g)
    return g


def _bwd(lib, h, net="x", seq="x", g="x", n_blocks=3, n=N):
    net, seq, g = RA._net() if net == "x" else net, FA._seq(n=n, head=None) if seq == "x" else seq, _grad(n=n) if g == "x" else g
    return lib.ftl_rnn_backward(h, C.byref(net) if net is not None else None, n_blocks, n, C.byref(seq) if seq is not None else None,
                                C.byref(g) if g is not None else None, None)


def _passes_all_but_the_last(lib, handle_, net="x", n_blocks=3, n=N, widths=(W0, 64, 64, 2), cell=64, gover=None, **over):
    """The call with a misaligned grad: FTL_E_INVALID with the message of the last check, so every check before it let the call pass."""
    rc = _bwd(lib, handle_, net=net, seq=FA._seq(widths, cell, n, **dict(over, head=None)), g=_grad(widths, n, **dict(gover or {}, grad=7 * FAKE + 1)),
              n_blocks=n_blocks, n=n)
    return rc == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()


# ---------------------------------------------------------------- the exports and the mirror
def test_symbols_declared_exported_and_listed(lib):
    hdr = A._header()
    for s in ("ftl_rnn_backward", "ftl_sizeof_rnn_backward_workspace", "ftl_sizeof_rnn_gradient"):
        assert re.search(r"\b%s\s*\(" % s, hdr) and hasattr(lib, s) and s in _lib.EXPORTS, s
    assert lib.ftl_rnn_backward.restype is C.c_int and len(lib.ftl_rnn_backward.argtypes) == 7
    assert lib.ftl_sizeof_rnn_backward_workspace.restype is C.c_int64
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no struct changed
    assert C.sizeof(abi.Rnn) == lib.ftl_sizeof_rnn() and C.sizeof(abi.RnnSequence) == lib.ftl_sizeof_rnn_sequence()
    assert int(re.search(r"#define\s+FTL_RNN_BWD_SPAN\s+(\d+)", hdr).group(1)) == abi.FTL_RNN_BWD_SPAN == RB.SPAN == 64
    src = open(os.path.join(ROOT, "continiousenvironment_follower_leader_amd", "csrc", "ftl_rnn.hpp")).read()
    assert re.search(r"__global__[^;{]*\bftl_rnn_backward_kernel\s*\(", src)
    assert int(re.search(r"#define\s+FTL_RNN_PASS_CELLS\s+(\d+)", src).group(1)) == abi.FTL_RNN_PASS_CELLS == RB.PASS


def test_mirror_matches_the_header(lib, tmp_path):
    struct, mirror = "ftl_rnn_gradient", abi.RnnGradient
    names = [f[0] for f in mirror._fields_]
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), A._header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert declared == names
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ftl.h"', "int main(void) {", '    printf("%%zu\\n", sizeof(%s));' % struct]
    src += ['    printf("%%zu\\n", offsetof(%s, %s));' % (struct, n) for n in names]
    src += ["    return 0;", "}"]
    (tmp_path / "off.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "off.cpp"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(mirror) == lib.ftl_sizeof_rnn_gradient()
    assert got[1:] == [getattr(mirror, n).offset for n in names]


# ---------------------------------------------------------------- the workspace query
def test_workspace_query_against_a_count_by_hand(lib):
    checked = 0
    widths, cell = (20, 16, 2), 8
    for flags in (BOTH, 0):
        for eps, n_sets in ((16, 3), (40, 2), (700, 1), (33, 2)):
            for env_first in (0, 7, eps - 1):
                for n in (1, 15, 32, 33, eps, eps + 1, 2 * eps - env_first):
                    if n < 1 or (env_first + n - 1) // eps >= n_sets:
                        continue
                    for B in (1, 2, 3, 5, 21, 32, 63, 64, 65, 70, 128, 129):
                        net = RA._net(widths, cell, flags, n_sets=n_sets, envs_per_set=eps, env_first=env_first)
                        want = RB.workspace_bytes(widths, cell, flags, B, n, eps, env_first)
                        assert lib.ftl_sizeof_rnn_backward_workspace(C.byref(net), B, n) == want, (flags, eps, env_first, n, B)
                        checked += 1
    assert checked > 400
    # the groups and spans of the cases the GPU tests name
    assert RB.plan(70, 40, 40) == (2, 4)                         # G = 1: a tile is a group of 70 pairs, spans of 64 + 6
    assert RB.plan(3, 22 * 32 + 5, 22 * 32 + 5) == (2, 2)         # G = 21: 23 tiles are two groups, 63 and 6 pairs
    assert RB.plan(64, 33, 33) == (2, 2) and RB.plan(65, 33, 33) == (2, 4)
    assert RB.plan(32, 65536, 64) == (1024, 1024) and RB.plan(32, 65536, 65536) == (1024, 1024)       # T = 32: one span a set of 64 envs
    net = RA._net()
    for bad in ((None, 1, 1), (net, 0, 1), (net, 1, 0), (net, -1, 5), (RA._net(envs_per_set=0), 1, 1), (RA._net(env_first=-1), 1, 1),
                (RA._net(cell=129), 1, 1), (RA._net((W0, 257, 2)), 1, 1), (RA._net(flags=4), 1, 1), (RA._net((W0, 64, 3)), 1, 1)):
        assert lib.ftl_sizeof_rnn_backward_workspace(C.byref(bad[0]) if bad[0] is not None else None, bad[1], bad[2]) == -1


# ---------------------------------------------------------------- refusals before any device work
def test_null_arguments_are_named(lib, handle):
    h = handle
    for kw, hh, word in ((dict(), None, b": h"), (dict(net=None), h, b": net"), (dict(net=RA._net(params=None)), h, b"net->params"),
                         (dict(seq=None), h, b": seq"), (dict(g=None), h, b": g"), (dict(seq=FA._seq(obs=None)), h, b"seq->obs"),
                         (dict(g=_grad(dhead=None)), h, b"g->dhead"), (dict(g=_grad(grad=None)), h, b"g->grad"),
                         (dict(g=_grad(workspace=None)), h, b"g->workspace"),
                         (dict(seq=FA._seq(kind=None)), h, b"seq->kind"), (dict(seq=FA._seq(action=None)), h, b"seq->action"),
                         (dict(seq=FA._seq(reward=None)), h, b"seq->reward")):
        assert _bwd(lib, hh, **kw) == abi.FTL_E_INVALID, word
        err = lib.ftl_last_error()
        assert b"ftl_rnn_backward" in err and b"null" in err and word in err, (word, err)
    # head, h and state_out play no part; what the net does not read may be NULL; a single block reads no record at all
    assert _passes_all_but_the_last(lib, h), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, h=None, state_out=None, state_at=99), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, net=RA._net(flags=abi.FTL_RNN_PREV_REWARD), action=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, net=RA._net(flags=abi.FTL_RNN_PREV_ACTION), reward=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, net=RA._net(flags=0), action=None, reward=None, reward0=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, n_blocks=1, action=None, reward=None, kind=None, reward0=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, gover=dict(dstate_in=9 * FAKE, dstate_out=10 * FAKE)), lib.ftl_last_error()


def test_the_net_is_refused_as_ftl_rnn_forward_refuses_it(lib, handle):
    h = handle
    seen = 0
    for net, code, msg in RA._bad_nets():
        if msg in (b"H * W", b"null"):
            continue
        assert _bwd(lib, h, net=net) == code, msg
        err = lib.ftl_last_error()
        assert msg in err, (msg, err)
        assert FA._fwd(lib, h, net=net) == code and lib.ftl_last_error() == err, (msg, err)       # the very message of ftl_rnn_forward
        seen += 1
    assert seen >= 16
    for bad in (abi.FTL_MLP_ACT_TANH, 2, -1):                          # the trunk is ReLU: the existing message
        assert _bwd(lib, h, net=RA._net(activation=bad)) == abi.FTL_E_UNSUPPORTED and b"trunk is ReLU" in lib.ftl_last_error(), bad
    # the limits: 180-256-256 with 128 cells and a head of 5 runs; three trunk layers of 256 ask for more LDS than a workgroup can have
    for widths, cell, flags in (((W0, 256, 256, 5), 128, BOTH), ((W0, 64, 1), 1, 0), ((65, 20, 5), 33, 1), ((4096, 8, 1), 128, 2),
                                ((W0, 128, 128, 128, 5), 128, BOTH)):
        assert _passes_all_but_the_last(lib, h, net=RA._net(widths, cell, flags), widths=widths, cell=cell), (widths, lib.ftl_last_error())
        assert abi.rnn_backward_lds_bytes(widths, cell, flags) <= abi.FTL_RNN_BWD_MAX_LDS, widths
    assert abi.rnn_backward_lds_bytes((W0, 256, 256, 5), 128, BOTH) == 152832 and abi.rnn_backward_lds_bytes((W0, 64, 64, 2), 64, BOTH) == 88064
    wide = (W0, 256, 256, 256, 5)
    assert abi.rnn_backward_lds_bytes(wide, 128, BOTH) > abi.FTL_RNN_BWD_MAX_LDS and abi.rnn_backward_lds_bytes(wide, 64, BOTH) > abi.FTL_RNN_BWD_MAX_LDS
    for cell in (128, 64):
        assert _bwd(lib, h, net=RA._net(wide, cell), seq=FA._seq(wide, cell, head=None), g=_grad(wide)) == abi.FTL_E_UNSUPPORTED
        assert b"160 KiB" in lib.ftl_last_error()


def test_counts_strides_workspace_and_alignment(lib, handle):
    h = handle
    for kw in (dict(n_blocks=0), dict(n_blocks=-1), dict(n=0), dict(n=-3)):
        assert _bwd(lib, h, seq=FA._seq(), g=_grad(), **kw) == abi.FTL_E_INVALID, kw
        assert b"n_blocks and n" in lib.ftl_last_error()
    assert _bwd(lib, h, n_blocks=65536) == abi.FTL_E_UNSUPPORTED and b"65,535" in lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, n_blocks=65535) and _passes_all_but_the_last(lib, h, n_blocks=1)
    big = RA._net(n_sets=1, envs_per_set=1 << 30)
    assert _bwd(lib, h, net=big, seq=FA._seq(n=1 << 30), g=_grad(n=1 << 30), n=1 << 30) == abi.FTL_E_UNSUPPORTED and b"tiles" in lib.ftl_last_error()
    many = RA._net(n_sets=1, envs_per_set=1 << 29)                      # 2^24 tiles of one set at B = 64: a span each
    assert _bwd(lib, h, net=many, seq=FA._seq(n=1 << 29), g=_grad(n=1 << 29), n=1 << 29, n_blocks=64) == abi.FTL_E_UNSUPPORTED
    assert b"spans" in lib.ftl_last_error()
    ob, ab, rb, kb, db = N * W0 * 4, N * 16, N * 8, N, N * 2 * 4
    for over, word in ((dict(obs_block_bytes=ob - 4), b"obs_block_bytes"), (dict(obs_block_bytes=ob + 2), b"obs_block_bytes"),
                       (dict(action_block_bytes=ab - 8), b"action_block_bytes"), (dict(action_block_bytes=ab + 4), b"action_block_bytes"),
                       (dict(reward_block_bytes=rb - 8), b"reward_block_bytes"), (dict(reward_block_bytes=rb + 4), b"reward_block_bytes"),
                       (dict(kind_block_bytes=kb - 1), b"kind_block_bytes"), (dict(obs=FAKE + 2), b"obs must be 4-byte aligned"),
                       (dict(action=2 * FAKE + 4), b"action not aligned"), (dict(reward=3 * FAKE + 4), b"reward must be 8-byte aligned"),
                       (dict(reward0=5 * FAKE + 4), b"reward0 must be 8-byte aligned")):
        assert _bwd(lib, h, seq=FA._seq(**over)) == abi.FTL_E_INVALID, over
        assert word in lib.ftl_last_error(), (over, lib.ftl_last_error())
    need = lib.ftl_sizeof_rnn_backward_workspace(C.byref(RA._net()), 3, N)
    assert need == RB.workspace_bytes((W0, 64, 64, 2), 64, BOTH, 3, N, N) > 0
    for over, word in ((dict(dhead_block_bytes=db - 4), b"dhead_block_bytes"), (dict(dhead_block_bytes=db + 2), b"dhead_block_bytes"),
                       (dict(workspace_bytes=need - 1), b"workspace_bytes"), (dict(workspace_bytes=0), b"workspace_bytes"),
                       (dict(dhead=6 * FAKE + 2), b"dhead must be 4-byte aligned"), (dict(dstate_in=9 * FAKE + 1), b"dstate_in must be 4-byte aligned"),
                       (dict(dstate_out=9 * FAKE + 2), b"dstate_out must be 4-byte aligned"), (dict(workspace=8 * FAKE + 2), b"workspace must be 4-byte aligned")):
        assert _bwd(lib, h, g=_grad(**over)) == abi.FTL_E_INVALID, over
        assert word in lib.ftl_last_error(), (over, lib.ftl_last_error())
    for grad in (7 * FAKE + 1, 7 * FAKE + 2, 7 * FAKE + 3):
        assert _bwd(lib, h, g=_grad(grad=grad)) == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, gover=dict(workspace_bytes=need, dhead_block_bytes=3 * db), obs_block_bytes=10 * ob)


# ---------------------------------------------------------------- the python surface
def test_python_surface(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("a library call before the argument checks were through")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(rnn, "_device_handle", no_library)
    p = inspect.signature(rnn.backward).parameters
    assert list(p) == ["widths", "cell", "params", "obs", "dhead", "action", "reward", "kind", "state", "reward0", "prev_action", "prev_reward",
                       "out", "dstate_in", "dstate_out"]
    assert [p[k].default for k in list(p)[5:]] == [None, None, None, None, None, True, True, None, None, None]
    p = inspect.signature(rnn.Net.__init__).parameters
    assert list(p)[1:] == ["widths", "cell", "n_sets", "prev_action", "prev_reward", "params", "device"]
    assert [p[k].default for k in list(p)[3:]] == [1, True, True, None, None]
    for name in ("cell_weights", "head_weights", "layer", "load_lstm_cell"):
        assert getattr(rnn.Net, name) is getattr(rnn.RecurrentPolicy, name)

    widths, cell, B, n = (5, 4, 2), 3, 4, 6
    S = abi.rnn_widths(widths, cell, BOTH)[3]
    count = abi.rnn_param_count(widths, cell, BOTH)
    f64, u8 = torch.float64, torch.uint8
    good = dict(widths=widths, cell=cell, params=torch.zeros(2, count), obs=torch.zeros(B, n, 5), dhead=torch.zeros(B, n, 2),
                action=torch.zeros(B - 1, n, 2, dtype=f64), reward=torch.zeros(B - 1, n, dtype=f64), kind=torch.zeros(B - 1, n, dtype=u8))
    bad = [dict(params=torch.zeros(2, count + 1)), dict(params=torch.zeros(2, count, dtype=f64)), dict(params=None), dict(prev_action=False),
           dict(params=torch.zeros(2, count, requires_grad=True)), dict(obs=torch.zeros(B, n, 5, requires_grad=True)),
           dict(obs=torch.zeros(B, n, 4)), dict(obs=torch.zeros(B, 7, 5)), dict(obs=None),
           dict(dhead=None), dict(dhead=torch.zeros(B, n, 3)), dict(dhead=torch.zeros(B - 1, n, 2)), dict(dhead=torch.zeros(B, n, 2, dtype=f64)),
           dict(dhead=torch.zeros(B, n, 4)[:, :, ::2]), dict(dhead=torch.zeros(B, n, 2, requires_grad=True)),
           dict(action=None), dict(action=torch.zeros(B - 1, n, 2)), dict(reward=None), dict(kind=None), dict(kind=torch.zeros(B - 2, n, dtype=u8)),
           dict(state=torch.zeros(n, S + 1)), dict(reward0=torch.zeros(n)),
           dict(out=torch.zeros(2, count + 1)), dict(out=torch.zeros(1, count)), dict(out=torch.zeros(2, count, dtype=f64)),
           dict(dstate_in=torch.zeros(n, 2 * cell + 1)), dict(dstate_in=torch.zeros(n, 2 * cell, dtype=f64)), dict(dstate_out=torch.zeros(n + 1, 2 * cell)),
           dict(dstate_out=torch.zeros(n, 4 * cell)[:, ::2]), dict(widths=(5, 2)), dict(widths=(5, 4, 3)), dict(cell=0)]
    for over in bad:
        with pytest.raises(ValueError):
            rnn.backward(**dict(good, **over))
    for w, c in (((5, 257, 2), 3), ((4097, 4, 2), 3), ((5, 4, 4, 4, 4, 2), 3), ((5, 4, 2), 129)):
        with pytest.raises(NotImplementedError):
            rnn.backward(w, c, torch.zeros(1, 1), torch.zeros(2, 2, w[0]), torch.zeros(2, 2, 2))
    wide = (5, 256, 256, 256, 2)                                   # inside ftl_rnn's limits, beyond the LDS of the backward kernel
    with pytest.raises(NotImplementedError, match="LDS"):
        rnn.backward(wide, 128, torch.zeros(1, abi.rnn_param_count(wide, 128, 0)), torch.zeros(1, n, 5), torch.zeros(1, n, 2), prev_action=False,
                     prev_reward=False)
    ok = [dict(), dict(state=torch.zeros(n, S), reward0=torch.zeros(n, dtype=f64), out=torch.zeros(2, count), dstate_in=torch.zeros(n, 2 * cell),
                       dstate_out=torch.zeros(n, 2 * cell)),
          dict(obs=torch.zeros(1, n, 5), dhead=torch.zeros(1, n, 2), action=None, reward=None, kind=None)]
    for over in ok:
        with pytest.raises(ValueError, match="GPU"):
            rnn.backward(**dict(good, **over))

    # rnn.Net: an nn.Module with one parameter that shares the given tensor's storage, and the views of the policy
    shared = torch.zeros(2, count)
    net = rnn.Net(widths, cell, n_sets=2, params=shared, device="cpu")
    assert isinstance(net, torch.nn.Module) and [tuple(q.shape) for q in net.parameters()] == [(2, count)]
    assert net.params.data_ptr() == shared.data_ptr() and net.params.requires_grad
    assert (net.P, net.R, net.U, net.S) == abi.rnn_widths(widths, cell, BOTH)
    Wg, bg = net.cell_weights()
    assert tuple(Wg.shape) == (2, net.U, 4 * cell) and tuple(net.head_weights()[0].shape) == (2, cell, 2) and tuple(net.layer(0)[0].shape) == (2, 5, 4)
    for kw in (dict(n_sets=0), dict(params=torch.zeros(1, count)), dict(params=torch.zeros(2, count, dtype=f64)), dict(widths=(5, 4, 3)), dict(cell=0)):
        with pytest.raises(ValueError):
            rnn.Net(**dict(dict(widths=widths, cell=cell, n_sets=2, device="cpu"), **kw))
    with pytest.raises(NotImplementedError):
        rnn.Net(widths, 129, device="cpu")
    seq = (good["obs"], good["action"], good["reward"], good["kind"])
    with pytest.raises(ValueError, match="GPU"):
        net(seq)
    with pytest.raises(ValueError, match="Trajectory"):
        net(good["obs"])
    with pytest.raises(ValueError, match="grad"):
        net((good["obs"].clone().requires_grad_(),) + seq[1:])
    traj = mlp.Trajectory(torch.zeros(B + 1, n, 5), torch.zeros(B, n, 2), torch.zeros(B, n, 2, dtype=f64), torch.zeros(B, n, dtype=f64),
                          torch.zeros(B, n, dtype=u8))
    with pytest.raises(ValueError, match="collect_rnn"):
        net(traj)
    traj.state = torch.zeros(1, n, S)
    with pytest.raises(ValueError, match="GPU"):
        net(traj)
    with pytest.raises(ValueError, match="reward0"):
        net(traj, reward0=torch.zeros(n))


# ---------------------------------------------------------------- the twin: variants, set independence
def gpu_case(trunk, cell, A_, w0, n, n_sets, flags, B, dstate=True):
    """The inputs of a case of tests/test_gpu_rnn_backward.py, a pure function of its parameters: the synthetic record of the forward
    tests cut to B blocks, head gradients with rows of zeros, and a gradient of the last block's state."""
    case = RS.synthetic(trunk, cell, A_, w0, n, n_sets, flags)
    rec = case["rec"]
    rng = np.random.default_rng(7 + cell + 10 * A_ + flags + n + w0 + 1000 * B)
    dy = rng.standard_normal((B, n, A_)).astype(F)
    dy[rng.random((B, n)) < 0.2] = 0.0
    dy[:, 1] = 0.0                                               # a row left out of every block
    rec = dict(obs=rec["obs"][:B], action=rec["action"][:B - 1], reward=rec["reward"][:B - 1], kind=rec["kind"][:B - 1], reward0=rec["reward0"])
    return dict(case, rec=rec, dhead=dy, dstate_in=(rng.standard_normal((n, 2 * cell)) * 0.3).astype(F) if dstate else None)


def twin(case, cell, flags, n_sets, **kw):
    rec, n = case["rec"], case["rec"]["obs"].shape[1]
    B = rec["obs"].shape[0]
    return RB.population_grad(case["params"], case["widths"], cell, flags, rec["obs"], case["dhead"], case["state"], rec["action"] if B > 1 else None,
                              rec["reward"] if B > 1 else None, rec["kind"] if B > 1 else None, rec["reward0"], kw.pop("envs_per_set", n // n_sets),
                              dstate_in=case["dstate_in"], **kw)


def test_wrong_variants_change_the_gradient_on_the_gpu_inputs():
    """On the inputs of the GPU cases (a subset of the nets: the patterns do not depend on the net) each wrong variant of the twin -- the
    carry not cut at VOID, dc_next dropped, i * (1 - i) in two roundings, libm's exp -- changes at least one gradient word."""
    checked = 0
    for (trunk, cell), A_, w0, n, n_sets in ((((20,), 32), 2, 65, 15, 1), (((33,), 63), 5, 65, 33, 3), (((64,), 1), 1, 65, 15, 1)):
        for flags in (BOTH, 0):
            case = gpu_case(trunk, cell, A_, w0, n, n_sets, flags, 5)
            RS.assert_patterns(case["rec"], case["state"])
            exact = twin(case, cell, flags, n_sets)[0].view(np.uint32)
            assert np.isfinite(exact.view(F)).all()
            for v in (dict(no_void_cut=True), dict(drop_dc_next=True), dict(two_roundings=True), dict(exp=R.exp_libm)):
                wrong = twin(case, cell, flags, n_sets, **v)[0].view(np.uint32)
                assert (wrong != exact).any(), (cell, A_, flags, v)
                checked += 1
    assert checked == 24


def test_a_set_alone_equals_the_middle_set_of_three():
    (trunk, cell), A_, w0, n, n_sets, flags = ((33,), 63), 2, 65, 33, 3, BOTH
    case = gpu_case(trunk, cell, A_, w0, n, n_sets, flags, 5)
    whole, dso = twin(case, cell, flags, n_sets)
    rows = slice(11, 22)
    rec = {k: (v[:, rows] if k != "reward0" else v[rows]) for k, v in case["rec"].items()}
    alone = dict(case, params=case["params"][1:2], rec=rec, dhead=case["dhead"][:, rows], state=case["state"][rows], dstate_in=case["dstate_in"][rows])
    g1, d1 = twin(alone, cell, flags, 1)
    assert np.array_equal(g1[0].view(np.uint32), whole[1].view(np.uint32)) and np.array_equal(d1.view(np.uint32), dso[rows].view(np.uint32))
    assert not np.array_equal(whole[0], whole[1]) and np.abs(whole[1]).sum() > 0


# ---------------------------------------------------------------- the twin against torch float64 autograd through the replay
def replay64(p, widths, cell, flags, rec, state, dhead):
    """d sum(dhead * head) / d params in float64 by torch autograd through the replay of INTEGRATION.md (a ``Sequential`` trunk, an
    ``LSTMCell`` and a ``Linear`` head under the device's state rule), in the layout of ``params``."""
    P, Rw, U, S = R.dims(widths, cell, flags)
    C_, B = cell, rec["obs"].shape[0]
    tr, Wg, bg, Wy, by = R.split(np.asarray(p, F), widths, cell, flags)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    lins = []
    for W, b in M.layers(tr, widths[:-1]):
        lin = torch.nn.Linear(W.shape[0], W.shape[1]).double()
        with torch.no_grad():
            lin.weight.copy_(t64(W.T)), lin.bias.copy_(t64(b))
        lins.append(lin)
    trunk = torch.nn.Sequential(*[m for lin in lins for m in (lin, torch.nn.ReLU())])
    cell_m, head = torch.nn.LSTMCell(U - C_, C_).double(), torch.nn.Linear(C_, widths[-1]).double()
    with torch.no_grad():
        cell_m.weight_ih.copy_(t64(Wg[:U - C_].T)), cell_m.weight_hh.copy_(t64(Wg[U - C_:].T)), cell_m.bias_ih.copy_(t64(bg)), cell_m.bias_hh.zero_()
        head.weight.copy_(t64(Wy.T)), head.bias.copy_(t64(by))
    st = t64(state)
    h, c, a_prev, live = st[:, :C_], st[:, C_:2 * C_], st[:, 2 * C_:2 * C_ + P], st[:, -1:]
    heads = []
    for t in range(B):
        parts = [trunk(t64(rec["obs"][t])), a_prev]
        if Rw:
            r = torch.from_numpy(np.asarray(rec["reward0"] if t == 0 else rec["reward"][t - 1]))
            parts.append(r.float().double()[:, None] * (live != 0))          # the reward the step before returned, as float32
        h, c = cell_m(torch.cat(parts, 1), (h, c))
        heads.append(head(h))
        if t + 1 < B:
            keep = t64(rec["kind"][t] != RS.VOID)[:, None]                    # the state is zeroed after every VOID row
            h, c, live = h * keep, c * keep, keep
            a_prev = torch.from_numpy(np.asarray(rec["action"][t])).float().double().reshape(len(keep), -1)[:, :P] * keep
    (torch.stack(heads) * t64(dhead)).sum().backward()
    g = [torch.cat([lin.weight.grad.t().reshape(-1), lin.bias.grad]) for lin in lins]
    g += [torch.cat([cell_m.weight_ih.grad.t(), cell_m.weight_hh.grad.t()]).reshape(-1), cell_m.bias_ih.grad,
          torch.cat([head.weight.grad.t().reshape(-1), head.bias.grad])]
    return torch.cat(g).numpy()


def tensors(widths, cell, flags):
    """The slices of one weight set, tensor by tensor: the trunk's W and b, W_g, b_g, W_y, b_y."""
    out, off = [], 0
    for a, b in zip(widths[:-2], widths[1:-1]):
        out += [slice(off, off + a * b), slice(off + a * b, off + (a + 1) * b)]
        off += (a + 1) * b
    U = R.dims(widths, cell, flags)[2]
    for k in (U * 4 * cell, 4 * cell, cell * widths[-1], widths[-1]):
        out.append(slice(off, off + k))
        off += k
    assert off == R.param_count(widths, cell, flags)
    return out


# (head, flags) -> seed: the first of 300 + 10 * head + flags + 40 k at which autograd_case's condition holds (searched on the CPU)
SEEDS = {(2, 3): 323, (2, 0): 320, (2, 1): 321, (2, 2): 322, (1, 3): 353, (1, 0): 310, (1, 1): 311, (1, 2): 312}


def autograd_case(A_, flags):
    """B = 12, C = 64, a record of ``rnn_seq_numpy.record`` with the patterns of the zero rule; the seed is one at which no trunk
    pre-activation lies within its forward error bound of zero (asserted), so a flipped ReLU select is not part of the comparison."""
    widths, cell, B, n = (24, 20, 16, A_), 64, 12, 8
    seed = SEEDS[A_, flags]
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(R.param_count(widths, cell, flags)) * 0.3).astype(F)
    rec = RS.record(seed + 1, B, n, widths[0], A_)
    rec["obs"] = rng.random((B, n, widths[0]), dtype=F)
    state = RS.random_state(seed + 2, n, R.dims(widths, cell, flags)[3])
    RS.assert_patterns(rec, state)
    dhead = rng.standard_normal((B, n, A_)).astype(F)
    dhead[rng.random((B, n)) < 0.2] = 0.0
    # the trunk's pre-activations and their error bound against exact arithmetic, as DESIGN.md 8.18 / 8.22 count it: a chain of K fmaf
    # is within g(K + 1) of the sum of magnitudes, and the input's own error passes through |W|
    g = lambda k: k * U32 / (1 - k * U32)
    h, E = rec["obs"].reshape(B * n, -1).astype(np.float64), None
    for W, b in M.layers(R.split(p, widths, cell, flags)[0].astype(np.float64), widths[:-1]):
        acc = h @ W + b
        E = g(W.shape[0] + 1) * (np.abs(h) @ np.abs(W) + np.abs(b)) + (0.0 if E is None else E @ np.abs(W))
        assert (np.abs(acc) > E).all(), (seed, float((np.abs(acc) / E).min()))
        h = np.maximum(acc, 0.0)                                 # (the ReLU is 1-Lipschitz: E carries over)
    return widths, cell, B, n, p, rec, state, dhead


@pytest.mark.parametrize("flags", [BOTH, 0, R.PREV_ACTION, R.PREV_REWARD])
@pytest.mark.parametrize("A_", [2, 1])
def test_exact_twin_equals_float64_autograd(A_, flags):
    """The contract's order in float64 with libm against torch float64 autograd on sum(dhead * head): the same derivative, so the two
    differ by float64 rounding over some 1e5 operations only: 1e-9 of the largest gradient magnitude of each tensor."""
    widths, cell, B, n, p, rec, state, dhead = autograd_case(A_, flags)
    g64 = replay64(p, widths, cell, flags, rec, state, dhead)
    got, _ = RB.set_grad(p, widths, cell, flags, rec["obs"], dhead, state, rec["action"], rec["reward"], rec["kind"], rec["reward0"], exact=True)
    assert got.dtype == np.float64
    for sl in tensors(widths, cell, flags):
        top = np.abs(g64[sl]).max()
        assert top > 0 and np.abs(got[sl] - g64[sl]).max() <= 1e-9 * top, (sl, float(np.abs(got[sl] - g64[sl]).max()), float(top))


@pytest.mark.parametrize("flags", [BOTH, 0, R.PREV_ACTION, R.PREV_REWARD])
@pytest.mark.parametrize("A_", [2, 1])
def test_float32_twin_close_to_float64_autograd(A_, flags):
    """The float32 twin against the same float64 gradient, per tensor relative to its largest magnitude: within F32_BOUND, 8 x the
    largest value measured over these eight cases (the constant's comment has the figure)."""
    widths, cell, B, n, p, rec, state, dhead = autograd_case(A_, flags)
    g64 = replay64(p, widths, cell, flags, rec, state, dhead)
    got, _ = RB.set_grad(p, widths, cell, flags, rec["obs"], dhead, state, rec["action"], rec["reward"], rec["kind"], rec["reward0"])
    assert got.dtype == F
    worst = max(float(np.abs(got[sl].astype(np.float64) - g64[sl]).max() / np.abs(g64[sl]).max()) for sl in tensors(widths, cell, flags))
    print("head %d flags %d: float32 twin vs torch float64, worst tensor %.3e of its largest gradient (allowed %.3e)" % (A_, flags, worst, F32_BOUND))
    assert 0 < worst <= F32_BOUND
