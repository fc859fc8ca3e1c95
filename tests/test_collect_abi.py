"""C-ABI checks of the trajectory collection that need no GPU (include/ftl.h: ftl_mlp_sample, ftl_collect_mlp, ftl_gae): exports, the
ctypes mirror of ftl_collect_buffers against the header compiled for the host (size and every offset), the FTL_TR_* values, every
argument check that comes before any device work -- each refused flag with its message -- and the wrapper's refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

import test_mlp_abi as A
from continiousenvironment_follower_leader_amd import _lib, abi
from test_mlp_abi import cfg_b, handle, lib  # noqa: F401  (fixtures)

ROOT = A.ROOT
SYMBOLS = ("ftl_sizeof_collect_buffers", "ftl_mlp_sample", "ftl_collect_mlp", "ftl_gae")
FAKE, N, W0 = A.FAKE, A.N, A.W0
ROW = {2: 16, 1: 8, 5: 4}            # bytes of one env's encoded action by head width


def _buffers(widths=(W0, 64, 64, 2), **over):
    b = abi.CollectBuffers()
    wl = widths[-1]
    b.obs, b.head, b.action, b.reward, b.kind, b.noise, b.sigma = FAKE, FAKE, FAKE, FAKE, FAKE, None, None
    b.obs_step_bytes, b.head_step_bytes, b.action_step_bytes = N * widths[0] * 4, N * wl * 4, N * ROW[wl]
    b.reward_step_bytes, b.kind_step_bytes, b.noise_step_bytes = N * 8, N, N * wl * 4
    for k, v in over.items():
        setattr(b, k, v)
    A._KEEP.append(b)
    return b


def _sample(lib, h, out="x", net="x", noise=None, sigma=None, head=FAKE, obs=FAKE, action=FAKE):
    out, net = A._outputs() if out == "x" else out, A._net() if net == "x" else net
    return lib.ftl_mlp_sample(h, C.byref(out) if out is not None else None, C.byref(net) if net is not None else None, noise, sigma, head, obs,
                              action, None)


def _collect(lib, h, out="x", net="x", b="x", T=3, flags=abi.FTL_STEP_NEXT_RESET):
    out, net, b = A._outputs() if out == "x" else out, A._net() if net == "x" else net, _buffers() if b == "x" else b
    return lib.ftl_collect_mlp(h, T, C.byref(out) if out is not None else None, C.byref(net) if net is not None else None,
                               C.byref(b) if b is not None else None, flags, None)


def _gae(lib, h, T=3, n=N, reward=FAKE, rsb=None, kind=FAKE, ksb=None, values=FAKE, adv=FAKE, ret=FAKE):
    return lib.ftl_gae(h, T, n, reward, n * 8 if rsb is None else rsb, kind, n if ksb is None else ksb, values, 0.99, 0.95, adv, ret, None)


# ---------------------------------------------------------------- exports, the mirror, the constants
def test_symbols_declared_exported_and_listed(lib):
    hdr = A._header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s
    assert any(s.endswith("ftl_collect.hpp") for s in _lib.SOURCES)
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION      # no existing struct changed


def test_transition_kinds(lib):
    body = re.search(r"enum\s*\{\s*(FTL_TR_STEP[^}]*)\}", A._header()).group(1)
    got = {k.strip(): int(v) for k, v in (item.split("=") for item in body.split(","))}
    assert got == dict(FTL_TR_STEP=0, FTL_TR_TERMINATED=1, FTL_TR_TRUNCATED=2, FTL_TR_VOID=3)
    for k, v in got.items():
        assert getattr(abi, k) == v
    assert abi.MISSION.index("finished_by_time") == 3


def test_mirror_matches_the_header(lib, tmp_path):
    """include/ftl.h's own ftl_collect_buffers, compiled for the host: its size and the offset of every field, by name."""
    names = [f[0] for f in abi.CollectBuffers._fields_]
    body = re.search(r"typedef\s+struct\s+ftl_collect_buffers\s*\{(.*?)\}\s*ftl_collect_buffers\s*;", A._header(), re.S).group(1)
    declared = []
    for d in body.split(";"):
        if d.strip():
            declared += [re.search(r"(\w+)\s*$", part.strip()).group(1) for part in d.split(",")]
    assert declared == names                                                # same fields, same order
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ftl.h"', "int main(void) {", '    printf("%zu\\n", sizeof(ftl_collect_buffers));']
    src += ['    printf("%%zu\\n", offsetof(ftl_collect_buffers, %s));' % n for n in names]
    src += ["    return 0;", "}"]
    (tmp_path / "off.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "off.cpp"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(abi.CollectBuffers) == lib.ftl_sizeof_collect_buffers() == 104
    assert got[1:] == [getattr(abi.CollectBuffers, n).offset for n in names]


# ---------------------------------------------------------------- refusals before any device work
def test_sample_argument_checks(lib, handle):
    h = handle
    assert _sample(lib, None) == abi.FTL_E_INVALID
    assert _sample(lib, h, out=None) == abi.FTL_E_INVALID
    assert _sample(lib, h, net=None) == abi.FTL_E_INVALID
    assert _sample(lib, h, action=None) == abi.FTL_E_INVALID
    for net, code, msg in A._bad_nets():                                       # the checks of ftl_mlp_act
        assert _sample(lib, h, net=net) == code, msg
        assert msg in lib.ftl_last_error(), (msg, lib.ftl_last_error())
    assert _sample(lib, h, out=A._outputs(policy_obs=None)) == abi.FTL_E_INVALID
    assert b"policy_obs" in lib.ftl_last_error()
    for widths in ((W0, 2), (W0, 1)):                                          # a Box head with noise but no sigma
        assert _sample(lib, h, net=A._net(widths), noise=FAKE) == abi.FTL_E_INVALID
        assert b"sigma" in lib.ftl_last_error()
    for kw in (dict(noise=FAKE + 2, sigma=FAKE), dict(noise=FAKE, sigma=FAKE + 1), dict(head=FAKE + 2), dict(obs=FAKE + 3)):
        assert _sample(lib, h, **kw) == abi.FTL_E_INVALID, kw
        assert b"4-byte aligned" in lib.ftl_last_error()
    assert _sample(lib, h, action=FAKE + 4) == abi.FTL_E_INVALID and b"action" in lib.ftl_last_error()
    # every argument fine, every optional pointer there or not: only the state is missing
    for kw in (dict(), dict(noise=FAKE, sigma=FAKE), dict(head=None, obs=None), dict(sigma=FAKE), dict(net=A._net((W0, 5)), noise=FAKE),
               dict(net=A._net((W0, 1)), noise=FAKE, sigma=FAKE)):
        assert _sample(lib, h, **kw) == abi.FTL_E_STATE, kw
        assert b"ftl_bind_state" in lib.ftl_last_error()


REFUSED_FLAGS = [(abi.FTL_STEP_AUTO_RESET, (b"FTL_STEP_AUTO_RESET", b"terminal", b"obs[t+1]")),
                 (abi.FTL_STEP_QUEUE_RESET, (b"FTL_STEP_QUEUE_RESET", b"obs[t+1]")),
                 (abi.FTL_STEP_SAMPLE_RESET, (b"FTL_STEP_SAMPLE_RESET", b"obs[t+1]")),
                 (abi.FTL_STEP_NO_SENSORS, (b"FTL_STEP_NO_SENSORS", b"policy_obs")),
                 (abi.FTL_STEP_NEXT_RESET | abi.FTL_STEP_NO_SENSORS, (b"FTL_STEP_NO_SENSORS", b"policy_obs")),
                 (abi.FTL_STEP_NEXT_RESET | abi.FTL_STEP_AUTO_RESET, (b"FTL_STEP_AUTO_RESET",)),
                 (2, (b"no flag but FTL_STEP_NEXT_RESET",)),
                 (abi.FTL_STEP_NEXT_RESET | 64, (b"no flag but FTL_STEP_NEXT_RESET",))]


def test_collect_argument_checks(lib, handle):
    h = handle
    assert _collect(lib, None) == abi.FTL_E_INVALID
    assert _collect(lib, h, out=None) == abi.FTL_E_INVALID
    assert _collect(lib, h, net=None) == abi.FTL_E_INVALID
    assert _collect(lib, h, b=None) == abi.FTL_E_INVALID
    for flags, words in REFUSED_FLAGS:
        assert _collect(lib, h, flags=flags) == abi.FTL_E_INVALID, flags
        for w in words:
            assert w in lib.ftl_last_error(), (flags, w, lib.ftl_last_error())       # it says why
    for T in (0, -2):
        assert _collect(lib, h, T=T) == abi.FTL_E_INVALID
        assert b"T must be positive" in lib.ftl_last_error()
    for net, code, msg in A._bad_nets():
        assert _collect(lib, h, net=net) == code, msg
        assert msg in lib.ftl_last_error(), (msg, lib.ftl_last_error())
    assert _collect(lib, h, out=A._outputs(policy_obs=None)) == abi.FTL_E_INVALID
    assert b"policy_obs" in lib.ftl_last_error()
    for field in ("obs", "head", "action", "reward", "kind"):
        assert _collect(lib, h, b=_buffers(**{field: None})) == abi.FTL_E_INVALID
        assert field.encode() in lib.ftl_last_error() and b"missing" in lib.ftl_last_error()
    for widths in ((W0, 64, 64, 2), (W0, 1), (W0, 5)):
        net = A._net(widths)
        for field in ("obs", "head", "action", "reward", "kind"):
            low = getattr(_buffers(widths), field + "_step_bytes") - (1 if field == "kind" else 8 if field == "reward" else ROW[widths[-1]] if field == "action" else 4)
            assert _collect(lib, h, net=net, b=_buffers(widths, **{field + "_step_bytes": low})) == abi.FTL_E_INVALID, (widths, field)
            assert b"step_bytes below" in lib.ftl_last_error()
        assert _collect(lib, h, net=net, b=_buffers(widths, noise=FAKE, sigma=FAKE, noise_step_bytes=N * widths[-1] * 4 - 4)) == abi.FTL_E_INVALID
        assert b"step_bytes below" in lib.ftl_last_error()
        assert _collect(lib, h, net=net, b=_buffers(widths, noise_step_bytes=0)) == abi.FTL_E_STATE          # (unused without noise)
        for over in (dict(obs=FAKE + 2), dict(head=FAKE + 1), dict(action=FAKE + 2), dict(reward=FAKE + 4),
                     dict(obs_step_bytes=N * widths[0] * 4 + 2), dict(reward_step_bytes=N * 8 + 4), dict(action_step_bytes=N * ROW[widths[-1]] + 2),
                     dict(noise=FAKE, sigma=FAKE, noise_step_bytes=N * widths[-1] * 4 + 2)):
            assert _collect(lib, h, net=net, b=_buffers(widths, **over)) == abi.FTL_E_INVALID, (widths, over)
            assert b"aligned" in lib.ftl_last_error(), over
        for over in (dict(noise=FAKE + 2, sigma=FAKE), dict(noise=FAKE, sigma=FAKE + 2)):
            assert _collect(lib, h, net=net, b=_buffers(widths, **over)) == abi.FTL_E_INVALID
            assert b"4-byte aligned" in lib.ftl_last_error()
        rc = _collect(lib, h, net=net, b=_buffers(widths, noise=FAKE))                                          # noise without sigma
        assert rc == (abi.FTL_E_STATE if widths[-1] == 5 else abi.FTL_E_INVALID)
        assert (b"ftl_bind_state" if widths[-1] == 5 else b"sigma") in lib.ftl_last_error()
        for flags in (0, abi.FTL_STEP_NEXT_RESET):                                                              # only the state is missing
            for b in (_buffers(widths), _buffers(widths, noise=FAKE, sigma=FAKE), _buffers(widths, kind_step_bytes=N + 1, obs_step_bytes=10 * N * widths[0] * 4)):
                assert _collect(lib, h, net=net, b=b, flags=flags, T=1) == abi.FTL_E_STATE
                assert b"ftl_bind_state" in lib.ftl_last_error()


def test_gae_argument_checks(lib, handle):
    h = handle
    assert _gae(lib, None) == abi.FTL_E_INVALID
    for name in ("reward", "kind", "values", "adv", "ret"):
        assert _gae(lib, h, **{name: None}) == abi.FTL_E_INVALID, name
        assert b"null" in lib.ftl_last_error()
    for kw in (dict(T=0), dict(T=-1), dict(n=0), dict(n=-5, rsb=64, ksb=8)):
        assert _gae(lib, h, **kw) == abi.FTL_E_INVALID, kw
        assert b"must be positive" in lib.ftl_last_error()
    for kw in (dict(rsb=N * 8 - 8), dict(ksb=N - 1)):
        assert _gae(lib, h, **kw) == abi.FTL_E_INVALID, kw
        assert b"step_bytes below" in lib.ftl_last_error()
    for kw in (dict(reward=FAKE + 4), dict(rsb=N * 8 + 4)):
        assert _gae(lib, h, **kw) == abi.FTL_E_INVALID, kw
        assert b"8-byte aligned" in lib.ftl_last_error()
    for kw in (dict(values=FAKE + 2), dict(adv=FAKE + 1), dict(ret=FAKE + 2)):
        assert _gae(lib, h, **kw) == abi.FTL_E_INVALID, kw
        assert b"4-byte aligned" in lib.ftl_last_error()


# ---------------------------------------------------------------- the python surface
def test_python_surface_needs_no_device(cfg_b):
    import inspect
    import torch
    from continiousenvironment_follower_leader_amd import mlp
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    p = inspect.signature(mlp.MlpPolicy.sample).parameters
    assert list(p)[1:] == ["noise", "sigma"] and p["noise"].default is None and p["sigma"].default is None
    p = inspect.signature(mlp.MlpPolicy.collect).parameters
    assert list(p)[1:] == ["T", "noise", "sigma", "auto_reset", "out"] and p["auto_reset"].default == "next_step" and p["out"].default is None
    for cls in (VecGame, PipelinedVecGame):
        p = inspect.signature(cls.collect_mlp).parameters
        assert list(p)[1:] == ["policy", "T", "noise", "sigma", "auto_reset", "out"] and p["auto_reset"].default == "next_step"
    assert list(inspect.signature(mlp.gae).parameters) == ["traj", "values", "gamma", "lam", "out"]

    class FakeBatch:
        n, device = 6, "cpu"
    FakeBatch.cfg = cfg_b
    with pytest.raises(ValueError, match="MlpPolicy of this batch"):
        VecGame.collect_mlp(FakeBatch(), object(), 3)
    kind = torch.tensor([[0, 1], [2, 3], [0, 0]], dtype=torch.uint8)
    tr = mlp.Trajectory(obs=None, head=None, action=None, reward=None, kind=kind)
    assert tr.valid.dtype == torch.bool and tr.valid.tolist() == [[True, True], [True, False], [True, True]]
    assert tr.terminated.tolist() == [[False, True], [False, False], [False, False]]
    assert tr.truncated.tolist() == [[False, False], [True, False], [False, False]]
    assert tr.noise is None and tr.sigma is None
    with pytest.raises(ValueError, match="reward"):
        mlp.gae((torch.zeros(3, 2, dtype=torch.float64), kind), torch.zeros(4, 2), 0.99, 0.95)       # not on a device
