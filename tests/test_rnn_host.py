"""CPU tests of the recurrent policy's arithmetic (include/ftl.h, the ftl_rnn_act block): the twin's exp32 / sig32 / tanh32
(tests/rnn_numpy.py) against float64 numpy, csrc/ftl_rnn_math.hpp compiled for the host against the twin bit for bit, and the twin's cell
against torch.nn.LSTMCell in float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import mlp_numpy as M
import rnn_numpy as R
from continiousenvironment_follower_leader_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _grid():
    """The points the contract's accuracy figures were measured on: 4 M in [-100, 100], 2 M normal draws x 3, 200 k around 0."""
    rng = np.random.default_rng(7)
    return np.concatenate([np.linspace(-100.0, 100.0, 4_000_000).astype(F), (rng.standard_normal(2_000_000) * 3).astype(F),
                           (rng.standard_normal(200_000) * 1e-3).astype(F)])


def test_twin_transcendentals_against_float64():
    x = _grid()
    worst = dict(exp=0.0, sig=0.0, tanh=0.0)
    for lo in range(0, x.size, 1 << 20):
        v = x[lo:lo + (1 << 20)]
        a = -np.abs(v)
        want = np.exp(np.fmax(a, F(-86.0)).astype(np.float64))
        ulp = np.spacing(want.astype(F)).astype(np.float64)
        worst["exp"] = max(worst["exp"], float(np.max(np.abs(R.exp32(a).astype(np.float64) - want) / ulp)))
        v64 = v.astype(np.float64)
        worst["sig"] = max(worst["sig"], float(np.max(np.abs(R.sig32(v).astype(np.float64) - 1.0 / (1.0 + np.exp(-v64))))))
        worst["tanh"] = max(worst["tanh"], float(np.max(np.abs(R.tanh32(v).astype(np.float64) - np.tanh(v64)))))
    print("exp32 %.3f ulp, sig32 %.3e, tanh32 %.3e" % (worst["exp"], worst["sig"], worst["tanh"]))
    assert worst["exp"] <= 1.0
    assert worst["sig"] <= 2.0 ** -23 and worst["tanh"] <= 2.0 ** -23


def test_twin_edges():
    v = R.edge_values()
    s, t = R.sig32(v), R.tanh32(v)
    nan = np.isnan(v)
    assert nan.sum() == 1 and np.isnan(s[nan]).all() and np.isnan(t[nan]).all() and not np.isnan(s[~nan]).any() and not np.isnan(t[~nan]).any()
    assert R.sig32(F(0.0)) == F(0.5) and R.sig32(F(-0.0)) == F(0.5) and R.sig32(F(np.inf)) == F(1.0)
    assert R.sig32(F(-np.inf)) == R.exp32(F(-86.0)) / (F(1.0) + R.exp32(F(-86.0))) > 0           # the clamp, not 0
    assert R.tanh32(F(np.inf)) == F(1.0) and R.tanh32(F(-1e30)) == F(-1.0)
    z = R.tanh32(np.array([0.0, -0.0], F))
    assert (z == 0).all() and np.signbit(z).tolist() == [False, True]
    assert R.tanh32(F(2.0 ** -149)) == 0 and R.tanh32(F(1e-8)) == 0                              # the accepted cancellation near 0
    assert (R.sig32(v[~nan]) != R.sig32(v[~nan], R.exp_libm)).any()                              # the values tell exp32 from libm's exp


@pytest.fixture(scope="module")
def host_math(tmp_path_factory):
    """csrc/ftl_rnn_math.hpp compiled for the host with -ffp-contract=off into a small library."""
    d = tmp_path_factory.mktemp("rnn_math")
    src = d / "rnn_math.cpp"
    src.write_text('#include "ftl_rnn_math.hpp"\n'
                   'extern "C" void rnn_math(const float* x, float* e, float* s, float* t, long n) {\n'
                   "    for (long i = 0; i < n; i++) {\n"
                   "        e[i] = ftlrnnmath::exp32(-fabsf(x[i])); s[i] = ftlrnnmath::sig32(x[i]); t[i] = ftlrnnmath::tanh32(x[i]);\n"
                   "    }\n}\n")
    so = str(d / "librnn_math.so")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I", os.path.join(ROOT, "continiousenvironment_follower_leader_amd", "csrc"), str(src), "-o", so])
    lib = C.CDLL(so)
    lib.rnn_math.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    lib.rnn_math.restype = None
    return lib


def test_header_equals_the_twin_bit_for_bit(host_math):
    rng = np.random.default_rng(11)
    x = np.concatenate([R.edge_values(), np.linspace(-100, 100, 60_001).astype(F), (rng.standard_normal(60_000) * 3).astype(F),
                        (rng.standard_normal(10_000) * 1e-3).astype(F),
                        rng.integers(0, 1 << 32, 20_000, dtype=np.uint64).astype(np.uint32).view(F)])          # any bit pattern, NaNs included
    x = np.ascontiguousarray(x, F)
    assert x.size >= 100_000
    e, s, t = (np.empty_like(x) for _ in range(3))
    host_math.rnn_math(x.ctypes.data, e.ctypes.data, s.ctypes.data, t.ctypes.data, x.size)
    for name, got, want in (("exp32", e, R.exp32(-np.abs(x))), ("sig32", s, R.sig32(x)), ("tanh32", t, R.tanh32(x))):
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (name, int(bad.sum()), x[bad][:5], got[bad][:5], want[bad][:5])


@pytest.mark.parametrize("scale", [0.1, 0.5])
def test_cell_against_torch_lstmcell(scale):
    """A 64-unit cell over 12 steps: the twin's head against torch.nn.LSTMCell (and Linear) in float64 on the same weights, with the twin's
    actions and the rewards fed back as a PPO replay feeds them.  The bound is 8 x the largest head difference between the exact twin
    and a float64 numpy evaluation of the same net with libm, measured here on these inputs (DESIGN 8.18 records the values)."""
    rng = np.random.default_rng(int(scale * 100))
    widths, cell, flags, n, T = (24, 32, 2), 64, R.PREV_ACTION | R.PREV_REWARD, 8, 12
    P, Rw, U, S = R.dims(widths, cell, flags)
    p = (rng.standard_normal(R.param_count(widths, cell, flags)) * scale).astype(F)
    xs = rng.random((T, n, widths[0]), dtype=F)
    rewards = rng.standard_normal((T, n))
    lo, hi = np.array([0.0, -1.0]), np.array([1.0, 1.0])
    trunk, Wg, bg, Wy, by = R.split(p, widths, cell, flags)
    (W0, b0), = M.layers(trunk, widths[:-1])
    lin, head = torch.nn.Linear(widths[0], widths[1]).double(), torch.nn.Linear(cell, 2).double()
    lstm = torch.nn.LSTMCell(U - cell, cell).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(W0.T.astype(np.float64))), lin.bias.copy_(torch.from_numpy(b0.astype(np.float64)))
        head.weight.copy_(torch.from_numpy(Wy.T.astype(np.float64))), head.bias.copy_(torch.from_numpy(by.astype(np.float64)))
        lstm.weight_ih.copy_(torch.from_numpy(Wg[:U - cell].T.astype(np.float64))), lstm.weight_hh.copy_(torch.from_numpy(Wg[U - cell:].T.astype(np.float64)))
        lstm.bias_ih.copy_(torch.from_numpy(bg.astype(np.float64))), lstm.bias_hh.zero_()
    state = np.zeros((n, S), F)
    st64 = np.zeros((n, S))
    h_t, c_t = torch.zeros(n, cell, dtype=torch.float64), torch.zeros(n, cell, dtype=torch.float64)
    measured = vs_torch = 0.0
    for t in range(T):
        r = R.decide(p, widths, cell, flags, xs[t], state, rewards[t], np.zeros(n, bool), M.BOX2, lo, hi)
        y64, h64, c64 = R.f64_forward(p, widths, cell, flags, xs[t], st64, rewards[t])
        measured = max(measured, float(np.abs(r["head"].astype(np.float64) - y64).max()))
        with torch.no_grad():
            a_prev = torch.from_numpy(state[:, 2 * cell:2 * cell + P].astype(np.float64))
            r_prev = torch.from_numpy(np.where(state[:, -1] != 0, rewards[t].astype(F), 0).astype(np.float64))[:, None]
            u = torch.cat([torch.relu(lin(torch.from_numpy(xs[t].astype(np.float64)))), a_prev, r_prev], 1)
            h_t, c_t = lstm(u, (h_t, c_t))
            vs_torch = max(vs_torch, float((head(h_t) - torch.from_numpy(r["head"].astype(np.float64))).abs().max()))
        state = r["state"]
        assert (state[:, -1] == 1).all()
        st64 = np.concatenate([h64, c64, state[:, 2 * cell:].astype(np.float64)], 1)              # (the recorded action and live, as a replay has them)
    print("scale %g: twin vs float64 libm %.3e, twin vs torch float64 %.3e, bound %.3e" % (scale, measured, vs_torch, 8 * measured))
    assert 0 < measured < 1e-4
    assert vs_torch <= 8 * measured
