"""C-ABI checks of the MLP policy that need no GPU (include/ftl.h: ftl_sizeof_mlp, ftl_mlp_param_count, ftl_mlp_act, ftl_rollout_mlp):
exports, the ctypes mirror of ftl_mlp against the header compiled for the host (size and every offset), the staging constants against the
kernel's source, every argument check that comes before any device work, and the wrapper's refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

from continiousenvironment_follower_leader_amd import _lib, abi, make_config
from golden_util import config_for, load_episode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftl_sizeof_mlp", "ftl_mlp_param_count", "ftl_mlp_act", "ftl_rollout_mlp")
FAKE = 4096                   # a non-null, aligned "device pointer" that is never dereferenced: the checks under test come first
N = 6
W0 = 180                      # config B: policy_obs is [5][36]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def cfg_b():
    return config_for(load_episode("B_s1_chase")[1])


@pytest.fixture()
def handle(lib, cfg_b):
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg_b.c), N, 0, C.byref(h)) == 0, lib.ftl_last_error()
    yield h
    lib.ftl_destroy(h)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ftl.h")).read(), flags=re.S)


_KEEP = []


def _outputs(**over):
    o = abi.Outputs()
    for name, _ in abi.Outputs._fields_:
        setattr(o, name, FAKE)
    for k, v in over.items():
        setattr(o, k, v)
    _KEEP.append(o)
    return o


def _ro(**over):
    ro = abi.RolloutOutputs()
    ro.ret, ro.steps, ro.status = FAKE, FAKE, FAKE
    for k, v in over.items():
        setattr(ro, k, v)
    _KEEP.append(ro)
    return ro


def _net(widths=(W0, 64, 64, 2), **over):
    net = abi.Mlp()
    net.params, net.n_sets, net.n_layers, net.env_first, net.envs_per_set = FAKE, 1, len(widths) - 1, 0, N
    for l, w in enumerate(widths[:abi.FTL_MLP_MAX_LAYERS + 1]):
        net.width[l] = w
    net.set_stride = abi.mlp_param_count(widths[:abi.FTL_MLP_MAX_LAYERS + 1])
    for k, v in over.items():
        setattr(net, k, v)
    _KEEP.append(net)
    return net


def _act(lib, h, out="x", net="x", action=FAKE):
    out, net = _outputs() if out == "x" else out, _net() if net == "x" else net
    return lib.ftl_mlp_act(h, C.byref(out) if out is not None else None, C.byref(net) if net is not None else None, action, None)


def _rollout(lib, h, out="x", ro="x", net="x", T=3, actions=None, step_bytes=0, flags=0):
    out, ro, net = _outputs() if out == "x" else out, _ro() if ro == "x" else ro, _net() if net == "x" else net
    return lib.ftl_rollout_mlp(h, T, 0.9, C.byref(out) if out is not None else None, C.byref(ro) if ro is not None else None,
                               C.byref(net) if net is not None else None, actions, step_bytes, flags, None)


# ---------------------------------------------------------------- exports, the mirror, the constants
def test_symbols_declared_exported_and_listed(lib):
    hdr = _header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s
    assert any(s.endswith("ftl_mlp.hpp") for s in _lib.SOURCES)
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no existing struct changed
    for name in ("FTL_MLP_MAX_LAYERS", "FTL_MLP_MAX_WIDTH", "FTL_MLP_MAX_IN"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == getattr(abi, name), name
    assert (abi.FTL_MLP_MAX_LAYERS, abi.FTL_MLP_MAX_WIDTH, abi.FTL_MLP_MAX_IN) == (4, 256, 4096)


def test_mirror_matches_the_header(lib, tmp_path):
    """include/ftl.h's own ftl_mlp, compiled for the host: its size and the offset of every field, by name."""
    names = [f[0] for f in abi.Mlp._fields_]
    body = re.search(r"typedef\s+struct\s+ftl_mlp\s*\{(.*?)\}\s*ftl_mlp\s*;", _header(), re.S).group(1)
    declared = [re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert declared == names                                                # same fields, same order
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ftl.h"', "int main(void) {", '    printf("%zu\\n", sizeof(ftl_mlp));']
    src += ['    printf("%%zu\\n", offsetof(ftl_mlp, %s));' % n for n in names]
    src += ['    printf("%zu\\n", sizeof(((ftl_mlp*)0)->width));', "    return 0;", "}"]
    (tmp_path / "off.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "off.cpp"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(abi.Mlp) == lib.ftl_sizeof_mlp()
    assert got[1:-1] == [getattr(abi.Mlp, n).offset for n in names]
    assert got[-1] == 4 * (abi.FTL_MLP_MAX_LAYERS + 1) == C.sizeof(abi.Mlp().width)


def test_staging_constants_mirror_the_kernel():
    src = open(os.path.join(ROOT, "continiousenvironment_follower_leader_amd", "csrc", "ftl_mlp.hpp")).read()
    for name in ("FTL_MLP_ENV_TILE", "FTL_MLP_K_CHUNK", "FTL_MLP_W_STAGE", "FTL_MLP_ENVS_PER_WAVE", "FTL_MLP_NEURON_BLOCK", "FTL_MLP_THREADS"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1)) == getattr(abi, name), name
    assert abi.FTL_MLP_ENV_TILE % abi.FTL_MLP_ENVS_PER_WAVE == 0 and abi.FTL_MLP_MAX_WIDTH % abi.FTL_MLP_NEURON_BLOCK == 0
    assert abi.mlp_chunk_rows(256) == 16 and abi.mlp_chunk_rows(64) == 64 and abi.mlp_chunk_rows(1) == 64 and abi.mlp_chunk_rows(70) == 56


def test_param_count(lib):
    for widths in ((180, 64, 64, 2), (5, 3, 2), (4096, 256, 256, 256, 5), (7, 1)):
        arr = (C.c_int32 * len(widths))(*widths)
        want = sum((a + 1) * b for a, b in zip(widths[:-1], widths[1:]))
        assert lib.ftl_mlp_param_count(arr, len(widths) - 1) == want == abi.mlp_param_count(widths)
    assert lib.ftl_mlp_param_count((C.c_int32 * 4)(180, 64, 64, 2), 3) == 15874
    for widths in ((180, 257, 2), (4097, 2), (0, 2), (3, 0)):
        assert lib.ftl_mlp_param_count((C.c_int32 * len(widths))(*widths), len(widths) - 1) == -1
    assert lib.ftl_mlp_param_count((C.c_int32 * 6)(8, 8, 8, 8, 8, 2), 5) == -1
    assert lib.ftl_mlp_param_count((C.c_int32 * 1)(8), 0) == -1
    assert lib.ftl_mlp_param_count(None, 2) == -1


# ---------------------------------------------------------------- refusals before any device work
BAD_NETS = [(dict(params=None), abi.FTL_E_INVALID, b"null"),
            (dict(params=FAKE + 2), abi.FTL_E_INVALID, b"4-byte aligned"),
            (dict(set_stride=abi.mlp_param_count((W0, 64, 64, 2)) - 1), abi.FTL_E_INVALID, b"set_stride"),
            (dict(n_sets=0), abi.FTL_E_INVALID, b"n_sets"),
            (dict(envs_per_set=0), abi.FTL_E_INVALID, b"envs_per_set"),
            (dict(env_first=-1), abi.FTL_E_INVALID, b"env_first"),
            (dict(envs_per_set=N - 1), abi.FTL_E_INVALID, b"last weight set"),             # env N-1 would use set 1 of 1
            (dict(env_first=1), abi.FTL_E_INVALID, b"last weight set"),
            (dict(n_sets=2, envs_per_set=2), abi.FTL_E_INVALID, b"last weight set"),
            (dict(n_layers=0), abi.FTL_E_INVALID, b"n_layers")]
BAD_WIDTHS = [((W0 - 1, 64, 2), abi.FTL_E_INVALID, b"H * W"),
              ((W0 + 1, 2), abi.FTL_E_INVALID, b"H * W"),
              ((W0, 64, 3), abi.FTL_E_INVALID, b"head width"),
              ((W0, 64, 4), abi.FTL_E_INVALID, b"head width"),
              ((W0, 0, 2), abi.FTL_E_INVALID, b"at least 1"),
              ((W0, 257, 2), abi.FTL_E_UNSUPPORTED, b"FTL_MLP_MAX_WIDTH"),
              ((4097, 2), abi.FTL_E_UNSUPPORTED, b"FTL_MLP_MAX_IN"),
              ((W0, 8, 8, 8, 8, 2), abi.FTL_E_UNSUPPORTED, b"FTL_MLP_MAX_LAYERS")]


def _bad_nets():
    for over, code, msg in BAD_NETS:
        yield _net(**over), code, msg
    for widths, code, msg in BAD_WIDTHS:
        yield _net(widths), code, msg


def test_act_argument_checks(lib, handle):
    h = handle
    assert _act(lib, None) == abi.FTL_E_INVALID
    assert _act(lib, h, out=None) == abi.FTL_E_INVALID
    assert _act(lib, h, net=None) == abi.FTL_E_INVALID
    assert _act(lib, h, action=None) == abi.FTL_E_INVALID
    for net, code, msg in _bad_nets():
        assert _act(lib, h, net=net) == code, msg
        assert msg in lib.ftl_last_error(), (msg, lib.ftl_last_error())
    assert _act(lib, h, out=_outputs(policy_obs=None)) == abi.FTL_E_INVALID
    assert b"policy_obs" in lib.ftl_last_error()
    for widths in ((W0, 2), (W0, 1), (W0, 5), (W0, 1, 256, 2), (W0, 256, 256, 256, 5)):       # every argument fine: only the state is missing
        assert _act(lib, h, net=_net(widths)) == abi.FTL_E_STATE, widths
        assert b"ftl_bind_state" in lib.ftl_last_error()
    assert _act(lib, h, net=_net(n_sets=3, envs_per_set=2)) == abi.FTL_E_STATE
    assert _act(lib, h, net=_net(n_sets=9, envs_per_set=1, env_first=3)) == abi.FTL_E_STATE


def test_act_needs_a_config_with_policy_obs(lib):
    h = C.c_void_p()
    cfg = make_config(bear_number=1, follower_sensors={})
    assert lib.ftl_create(C.byref(cfg.c), N, 0, C.byref(h)) == 0, lib.ftl_last_error()
    try:
        assert _act(lib, h, net=_net((1, 2))) == abi.FTL_E_INVALID
        assert b"policy_obs" in lib.ftl_last_error()
    finally:
        lib.ftl_destroy(h)


def test_rollout_argument_checks(lib, handle):
    h = handle
    assert _rollout(lib, None) == abi.FTL_E_INVALID
    assert _rollout(lib, h, out=None) == abi.FTL_E_INVALID
    assert _rollout(lib, h, ro=None) == abi.FTL_E_INVALID
    assert _rollout(lib, h, net=None) == abi.FTL_E_INVALID
    for field in ("ret", "steps", "status"):
        assert _rollout(lib, h, ro=_ro(**{field: None})) == abi.FTL_E_INVALID
        assert field.encode() in lib.ftl_last_error()
    for T in (0, -2):
        assert _rollout(lib, h, T=T) == abi.FTL_E_INVALID
        assert b"T must be positive" in lib.ftl_last_error()
    assert _rollout(lib, h, flags=abi.FTL_STEP_NO_SENSORS) == abi.FTL_E_INVALID
    assert b"FTL_STEP_NO_SENSORS" in lib.ftl_last_error() and b"policy_obs" in lib.ftl_last_error()       # it says why
    for flags in (abi.FTL_STEP_AUTO_RESET, abi.FTL_STEP_NEXT_RESET, abi.FTL_STEP_QUEUE_RESET, abi.FTL_STEP_SAMPLE_RESET, 2,
                  abi.FTL_STEP_AUTO_RESET | abi.FTL_STEP_NO_SENSORS):
        assert _rollout(lib, h, flags=flags) == abi.FTL_E_INVALID, flags
    for net, code, msg in _bad_nets():
        assert _rollout(lib, h, net=net) == code, msg
        assert msg in lib.ftl_last_error(), (msg, lib.ftl_last_error())
    assert _rollout(lib, h, out=_outputs(policy_obs=None)) == abi.FTL_E_INVALID
    assert b"policy_obs" in lib.ftl_last_error()
    for widths, row in (((W0, 2), 16), ((W0, 1), 8), ((W0, 5), 4)):
        assert _rollout(lib, h, net=_net(widths), actions=FAKE, step_bytes=N * row - 1) == abi.FTL_E_INVALID
        assert b"step_bytes" in lib.ftl_last_error()
        for kw in (dict(), dict(actions=FAKE, step_bytes=N * row), dict(actions=FAKE, step_bytes=10 * N * row), dict(T=1)):
            assert _rollout(lib, h, net=_net(widths), **kw) == abi.FTL_E_STATE                 # only the state is missing
            assert b"ftl_bind_state" in lib.ftl_last_error()


# ---------------------------------------------------------------- the python surface
def test_python_surface_needs_no_device(cfg_b):
    import inspect
    from continiousenvironment_follower_leader_amd.mlp import MlpPolicy, check_widths, head_encoding
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    p = inspect.signature(MlpPolicy.__init__).parameters
    assert list(p)[1:] == ["batch", "widths", "params", "n_sets", "activation"] and p["params"].default is None and p["n_sets"].default == 1
    assert p["activation"].default == "relu" and all(q.kind is q.POSITIONAL_OR_KEYWORD for q in p.values())    # (a plain signature)
    p = inspect.signature(MlpPolicy.rollout).parameters
    assert list(p)[1:] == ["T", "gamma", "record"] and [p[k].default for k in list(p)[2:]] == [1.0, False]
    for cls in (VecGame, PipelinedVecGame):
        p = inspect.signature(cls.rollout_mlp).parameters
        assert list(p)[1:] == ["policy", "T", "gamma", "record"]
    for name in ("act", "__call__", "layer", "fitness"):
        assert callable(getattr(MlpPolicy, name))
    assert head_encoding(cfg_b) == (abi.FTL_ACTION_BOX2, 2)
    assert check_widths(cfg_b, [180, 64, 2]) == (180, 64, 2)

    class FakeBatch:
        n, device, policy_obs = 6, "cpu", None
    FakeBatch.cfg = cfg_b
    with pytest.raises(ValueError, match="policy_obs"):
        MlpPolicy(FakeBatch(), (180, 64, 2))                               # built without policy_obs=True
    for widths in ((180, 64, 3), (180, 5), (180, 1), (180,), (180, 0, 2)):
        with pytest.raises(ValueError):
            MlpPolicy(FakeBatch(), widths)
    for widths in ((180, 257, 2), (4097, 2), (180, 8, 8, 8, 8, 2)):
        with pytest.raises(NotImplementedError):
            MlpPolicy(FakeBatch(), widths)

    class FakeObs:
        shape = (6, 5, 36)
    FakeBatch.policy_obs = FakeObs()
    with pytest.raises(ValueError, match="H \\* W"):
        MlpPolicy(FakeBatch(), (181, 64, 2))
    for n_sets in (0, 4, 5, -1):
        with pytest.raises(ValueError, match="n_sets"):
            MlpPolicy(FakeBatch(), (180, 64, 2), n_sets=n_sets)
    meta = load_episode("B_s1_chase")[1]
    FakeBatch.cfg = config_for(meta, discrete_action_space=True)
    assert head_encoding(FakeBatch.cfg) == (abi.FTL_ACTION_DISCRETE, 5)
    with pytest.raises(ValueError, match="head"):
        MlpPolicy(FakeBatch(), (180, 64, 2))
    FakeBatch.cfg = config_for(load_episode("Bcfs_s2_chase")[1])
    assert head_encoding(FakeBatch.cfg) == (abi.FTL_ACTION_TURN, 1)
    with pytest.raises(ValueError, match="head"):
        MlpPolicy(FakeBatch(), (180, 64, 2))
    with pytest.raises(ValueError, match="MlpPolicy of this batch"):
        VecGame.rollout_mlp(FakeBatch(), object(), 3)
