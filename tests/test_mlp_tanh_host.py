"""CPU checks of the tanh hidden activation of the MLP policy (include/ftl.h: ``ftl_mlp.activation``, FTL_MLP_ACT_*): the twin
(tests/mlp_tanh_numpy.py) against ``mlp_numpy`` and against float64, the struct layouts against the numbers they had before the field got
its name, the refusals of both values' misuse before any device work, the torch helpers of ``mlp.py`` and the wrapper's argument check."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mlp_numpy as M
import mlp_tanh_numpy as MT
import test_collect_abi as CA
import test_mlp_abi as A
import test_rnn_abi as RA
from continiousenvironment_follower_leader_amd import _lib, abi, mlp
from test_mlp_abi import cfg_b, handle, lib  # noqa: F401  (fixtures)

ROOT = A.ROOT
U32, U64 = 2.0 ** -24, 2.0 ** -53          # unit roundoffs of float32 and float64
TANH32_ABS = 8.93e-8                       # csrc/ftl_rnn_math.hpp, include/ftl.h: tanh32 against the float64 value, absolute
SHAPES = [((180, 64, 64, 2), 0.1), ((180, 17, 2), 1.0), ((180, 33, 16, 31, 5), 0.3), ((180, 1), 1.0)]


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize("widths, scale", SHAPES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_relu_branch_is_mlp_numpy(widths, scale):
    rng = np.random.default_rng(len(widths))
    p, x = M.nasty_params(rng, 2, widths, scale), M.nasty_inputs(rng, 12, widths[0])
    for s in range(2):
        a, b = MT.raw_forward(p[s], widths, x, "relu"), M.raw_forward(p[s], widths, x)
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    lo, hi = np.array([0.0, -0.5]), np.array([0.25, 0.5])
    if widths[-1] == 2:
        assert np.array_equal(MT.population(p, widths, x, M.BOX2, lo, hi, 6, activation="relu"), M.population(p, widths, x, M.BOX2, lo, hi, 6))
        assert not np.array_equal(MT.population(p, widths, x, M.BOX2, lo, hi, 6), M.population(p, widths, x, M.BOX2, lo, hi, 6))


def _f64_and_bound(params, widths, x):
    """(float64 evaluation y64, bound) of one weight set on float32 rows x, with bound >= |twin - y64| elementwise, derived from the
    operation count.  Per layer of K inputs, with x^ the twin's float32 inputs of the layer, E their error bounds and S = |x^| |W| + |b|:
      the chain     K fmaf, one rounding each, from the bias: |acc^ - (x^ W + b)| <= g32(K) * S, g(K) = K u / (1 - K u); a result in the
                    subnormal range is rounded to a multiple of 2^-149 instead: + K * 2^-150;
      the inputs    |x^ W - x W| <= E |W|;
      float64       the reference's own matmul and bias add, K + 1 roundings: g64(K + 1) * S64;
      tanh          hidden layers: |tanh32(acc^) - tanh(acc)| <= 8.93e-8 (the header's absolute error of tanh32 at acc^) + |acc^ - acc|
                    (tanh is 1-Lipschitz) + 2^-52 (np.tanh, below one ulp of a value of at most 1).
    The head has no activation: its bound is the pre-activation's."""
    ls = M.layers(np.asarray(params, np.float32), widths)
    h32, h64 = np.asarray(x, np.float32), np.asarray(x, np.float32).astype(np.float64)
    E = np.zeros_like(h64)
    for l, (W, b) in enumerate(ls):
        K = W.shape[0]
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        acc32 = np.broadcast_to(b, (h32.shape[0], W.shape[1])).astype(np.float32)
        for k in range(K):
            acc32 = M.fmaf32(h32[:, k:k + 1], W[k][None, :], acc32)
        acc64 = h64 @ W64 + b64
        S32 = np.abs(h32.astype(np.float64)) @ np.abs(W64) + np.abs(b64)
        S64 = np.abs(h64) @ np.abs(W64) + np.abs(b64)
        g32, g64 = K * U32 / (1 - K * U32), (K + 1) * U64 / (1 - (K + 1) * U64)
        E = g32 * S32 + K * 2.0 ** -150 + E @ np.abs(W64) + g64 * S64
        if l + 1 < len(ls):
            h32, h64 = MT.ACTIVATIONS["tanh"](acc32), np.tanh(acc64)
            E = E + TANH32_ABS + 2.0 ** -52
        else:
            h32, h64 = acc32, acc64
    return h32, h64, E


@pytest.mark.parametrize("widths, scale", SHAPES[:3], ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tanh_twin_within_the_derived_bound_of_float64(widths, scale):
    rng = np.random.default_rng(7 + len(widths))
    p, x = M.nasty_params(rng, 2, widths, scale), M.nasty_inputs(rng, 24, widths[0])
    for s in range(2):
        y = MT.raw_forward(p[s], widths, x, "tanh")
        again, y64, bound = _f64_and_bound(p[s], widths, x)
        assert np.array_equal(y.view(np.uint32), again.view(np.uint32))            # the bound was derived on the twin's own intermediates
        err = np.abs(y.astype(np.float64) - y64)
        print("widths %s set %d: max error %.3e, bound there %.3e, largest bound %.3e, max |y| %.3e"
              % (widths, s, err.max(), bound.flat[err.argmax()], bound.max(), np.abs(y64).max()))
        assert np.isfinite(y64).all() and (err <= bound).all(), (widths, s, float((err - bound).max()))


# ---------------------------------------------------------------- the contract's numbers
MLP_OFFSETS = dict(params=0, set_stride=8, n_sets=16, n_layers=20, width=24, env_first=44, envs_per_set=48, activation=52)
RNN_OFFSETS = dict(MLP_OFFSETS, cell=56, flags=60, state=64, state_stride=72)


@pytest.mark.parametrize("struct, mirror, want, size", [("ftl_mlp", abi.Mlp, MLP_OFFSETS, 56), ("ftl_rnn", abi.Rnn, RNN_OFFSETS, 80)])
def test_layouts_are_the_ones_before_the_field_had_a_name(lib, tmp_path, struct, mirror, want, size):
    """sizeof and every offset of ftl_mlp and ftl_rnn, from the header compiled for the host and from the ctypes mirror, against the
    numbers of the layout in which ``activation`` was ``_pad`` (offset 52 of 56 bytes)."""
    names = [f[0] for f in mirror._fields_]
    assert names == list(want)
    assert C.sizeof(mirror) == size and {n: getattr(mirror, n).offset for n in names} == want
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ftl.h"', "int main(void) {", '    printf("%%zu\\n", sizeof(%s));' % struct]
    src += ['    printf("%%zu\\n", offsetof(%s, %s));' % (struct, n) for n in names] + ["    return 0;", "}"]
    (tmp_path / "off.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "off.cpp"), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got[0] == size == getattr(lib, "ftl_sizeof_" + struct[4:])()
    assert got[1:] == [want[n] for n in names]


def test_constants_mirror_the_header():
    hdr = A._header()
    for name, value in (("FTL_MLP_ACT_RELU", 0), ("FTL_MLP_ACT_TANH", 1)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == getattr(abi, name) == value, name
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4
    assert mlp.ACTIVATIONS == dict(relu=abi.FTL_MLP_ACT_RELU, tanh=abi.FTL_MLP_ACT_TANH)
    assert abi.Mlp().activation == abi.FTL_MLP_ACT_RELU                     # a zeroed struct means what it meant


# ---------------------------------------------------------------- refusals before any device work
def test_mlp_entry_points_refuse_an_unknown_activation(lib, handle):
    h = handle
    calls = dict(ftl_mlp_act=lambda net: A._act(lib, h, net=net), ftl_mlp_sample=lambda net: CA._sample(lib, h, net=net),
                 ftl_rollout_mlp=lambda net: A._rollout(lib, h, net=net), ftl_collect_mlp=lambda net: CA._collect(lib, h, net=net))
    for name, call in calls.items():
        for bad in (2, -1, 7, 1 << 30):
            assert call(A._net(activation=bad)) == abi.FTL_E_INVALID, (name, bad)
            assert b"activation" in lib.ftl_last_error(), (name, lib.ftl_last_error())
        for good in (abi.FTL_MLP_ACT_RELU, abi.FTL_MLP_ACT_TANH):          # every argument fine: only the state is missing
            assert call(A._net(activation=good)) == abi.FTL_E_STATE, (name, good)
            assert b"ftl_bind_state" in lib.ftl_last_error()


def test_rnn_entry_points_accept_relu_only(lib, handle):
    h = handle
    calls = dict(ftl_rnn_act=lambda net: RA._act(lib, h, net=net), ftl_rollout_rnn=lambda net: RA._rollout(lib, h, net=net),
                 ftl_collect_rnn=lambda net: RA._collect(lib, h, net=net))
    for name, call in calls.items():
        for bad in (abi.FTL_MLP_ACT_TANH, 2, -1):
            assert call(RA._net(activation=bad)) == abi.FTL_E_UNSUPPORTED, (name, bad)
            assert b"ReLU" in lib.ftl_last_error(), (name, lib.ftl_last_error())
        assert call(RA._net(activation=abi.FTL_MLP_ACT_RELU)) == abi.FTL_E_STATE, name


# ---------------------------------------------------------------- the torch helpers
@pytest.mark.parametrize("activation", ["relu", "tanh"])
def test_torch_helpers_round_trip(activation):
    widths = (7, 5, 3, 2)
    torch.manual_seed(3)
    module = mlp.torch_module(widths, activation)
    assert [type(m).__name__ for m in module] == ["Linear", activation.capitalize().replace("Relu", "ReLU"), "Linear",
                                                  activation.capitalize().replace("Relu", "ReLU"), "Linear"]
    w, act, row = mlp.params_from_torch(module)
    assert w == widths and act == activation and row.dtype == torch.float32 and tuple(row.shape) == (abi.mlp_param_count(widths),)
    assert row.device.type == "cpu" and not row.requires_grad
    for (W, b), lin in zip(M.layers(row.numpy(), widths), module[::2]):     # W_l is weight.T ([in][out]), then b_l
        assert np.array_equal(W, lin.weight.detach().numpy().T) and np.array_equal(b, lin.bias.detach().numpy())
    back = mlp.torch_module(widths, activation, row)
    w2, act2, row2 = mlp.params_from_torch(back)
    assert (w2, act2) == (widths, activation) and torch.equal(row2, row)
    x = torch.randn(9, widths[0])
    assert torch.equal(back(x), module(x))
    # the module computes what the twin computes, up to torch's own summation order
    y = MT.raw_forward(row.numpy(), widths, x.numpy(), activation)
    assert np.allclose(y, module(x).detach().numpy(), rtol=0, atol=1e-5)
    assert mlp.params_from_torch(torch.nn.Sequential(torch.nn.Linear(4, 2)))[:2] == ((4, 2), "relu")


def test_torch_helpers_refuse_what_ftl_mlp_cannot_hold():
    nn = torch.nn
    L = nn.Linear
    for bad in (nn.Sequential(L(4, 3), nn.ReLU(), L(3, 3), nn.Tanh(), L(3, 2)),            # mixed
                nn.Sequential(L(4, 3), nn.Sigmoid(), L(3, 2)),
                nn.Sequential(L(4, 3), nn.ReLU(), L(3, 2), nn.Tanh()),                     # the last layer is not linear
                nn.Sequential(L(4, 3), L(3, 2)),
                nn.Sequential(L(4, 3), nn.ReLU(), L(4, 2)),                                # widths do not chain
                nn.Sequential(L(4, 3), nn.ReLU(), L(3, 2, bias=False)),
                nn.Sequential(), L(4, 2)):
        with pytest.raises(ValueError):
            mlp.params_from_torch(bad)
    with pytest.raises(ValueError, match="mixed"):
        mlp.params_from_torch(nn.Sequential(L(4, 3), nn.ReLU(), L(3, 3), nn.Tanh(), L(3, 2)))
    with pytest.raises(ValueError, match="activation"):
        mlp.torch_module((4, 3, 2), "gelu")
    with pytest.raises(ValueError, match="params_row"):
        mlp.torch_module((4, 3, 2), "tanh", torch.zeros(5))
    with pytest.raises(ValueError):
        mlp.torch_module((4,), "tanh")


# ---------------------------------------------------------------- the wrapper's argument
def test_policy_checks_its_activation(cfg_b):
    class FakeObs:
        shape = (6, 5, 36)

    class FakeBatch:
        n, device, policy_obs, cfg = 6, torch.device("cpu"), FakeObs(), cfg_b
    for bad in ("gelu", "TANH", "", None, 1, abi.FTL_MLP_ACT_TANH):
        with pytest.raises(ValueError, match="activation"):
            mlp.MlpPolicy(FakeBatch(), (180, 64, 2), activation=bad)
    with pytest.raises(TypeError):
        mlp.MlpPolicy(FakeBatch(), (180, 64, 2), None, 1, "tanh", activation="tanh")
    with pytest.raises(TypeError):
        mlp.MlpPolicy(FakeBatch(), (180, 64, 2), None, 1, "tanh", "relu")
    with pytest.raises(ValueError, match="n_sets"):                                        # the other checks still come
        mlp.MlpPolicy(FakeBatch(), (180, 64, 2), n_sets=4, activation="tanh")
    for kw, name, code in ((dict(), "relu", 0), (dict(activation="relu"), "relu", 0), (dict(activation="tanh"), "tanh", 1)):
        pol = mlp.MlpPolicy(FakeBatch(), (180, 64, 2), n_sets=2, **kw)
        assert pol.activation == name and [net.activation for _, _, net in pol._parts] == [code]
    pol = mlp.MlpPolicy(FakeBatch(), (180, 64, 2), None, 3, "tanh")                        # the fifth argument
    assert pol.activation == "tanh" and pol.n_sets == 3 and pol._parts[0][2].activation == abi.FTL_MLP_ACT_TANH
