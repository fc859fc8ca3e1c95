"""C-ABI checks of the baseline follower that need no GPU (include/ftl.h: ftl_baseline_bytes, ftl_baseline_act, ftl_rollout_baseline):
exports, constants and the row size against the header, and the argument checks that come before any device work."""
import ctypes as C
import os
import re

import pytest

from continiousenvironment_follower_leader_amd import _lib, abi, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftl_baseline_bytes", "ftl_baseline_act", "ftl_rollout_baseline")
FAKE = 4096      # a non-null, aligned "device pointer" that is never dereferenced: the checks under test come first
N, CAP = 4, 8
ROW = 16 + 16 * CAP
RESETS = (abi.FTL_STEP_AUTO_RESET, abi.FTL_STEP_NEXT_RESET, abi.FTL_STEP_QUEUE_RESET, abi.FTL_STEP_SAMPLE_RESET)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture()
def handle(lib):
    cfg = make_config(bear_number=1)
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), N, 0, C.byref(h)) == 0, lib.ftl_last_error()
    yield h
    lib.ftl_destroy(h)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ftl.h")).read(), flags=re.S)


def _outputs():
    o = abi.Outputs()
    for name, _ in abi.Outputs._fields_:
        setattr(o, name, None if name == "policy_obs" else FAKE)
    return o


def _ro(**over):
    ro = abi.RolloutOutputs()
    ro.ret, ro.steps, ro.status = FAKE, FAKE, FAKE
    for k, v in over.items():
        setattr(ro, k, v)
    return ro


def _act(lib, h, out, bl=FAKE, bl_bytes=N * ROW, cap=CAP, action=FAKE):
    return lib.ftl_baseline_act(h, C.byref(out) if out is not None else None, bl, bl_bytes, cap, action, None)


def _rollout(lib, h, out, ro, T=3, bl=FAKE, bl_bytes=N * ROW, cap=CAP, actions=None, step_bytes=0, flags=0):
    return lib.ftl_rollout_baseline(h, T, 1.0, C.byref(out) if out is not None else None, C.byref(ro) if ro is not None else None, bl, bl_bytes,
                                    cap, actions, step_bytes, flags, None)


def test_symbols_declared_exported_and_listed(lib):
    hdr = _header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s


def test_constants_match_the_header():
    hdr = _header()
    assert int(re.search(r"#define\s+FTL_BL_EMPTY\s+(\d+)u", hdr).group(1)) == abi.FTL_BL_EMPTY == 1
    assert int(re.search(r"#define\s+FTL_BL_OVERFLOW\s+(\d+)u", hdr).group(1)) == abi.FTL_BL_OVERFLOW == 2
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no existing struct changed
    assert (abi.BL_HEAD, abi.BL_COUNT, abi.BL_PENDING, abi.BL_FLAGS) == (0, 1, 2, 3)


def test_row_size(lib, handle):
    for cap in (2, 8, 64, 1000):
        assert lib.ftl_baseline_bytes(handle, cap) == N * (16 + 16 * cap) == N * abi.baseline_row_bytes(cap)
    assert lib.ftl_baseline_bytes(handle, 1) == 0 and lib.ftl_baseline_bytes(None, 8) == 0


def test_act_argument_checks(lib, handle):
    out = _outputs()
    assert _act(lib, None, out) == abi.FTL_E_INVALID
    assert _act(lib, handle, None) == abi.FTL_E_INVALID
    assert _act(lib, handle, out, bl=None) == abi.FTL_E_INVALID
    assert _act(lib, handle, out, action=None) == abi.FTL_E_INVALID
    for cap in (1, 0, -3):
        assert _act(lib, handle, out, cap=cap) == abi.FTL_E_INVALID
        assert b"cap" in lib.ftl_last_error()
    assert _act(lib, handle, out, bl_bytes=N * ROW - 1) == abi.FTL_E_INVALID
    assert b"ftl_baseline_bytes" in lib.ftl_last_error()
    assert _act(lib, handle, out, bl=FAKE + 4) == abi.FTL_E_INVALID
    assert b"aligned" in lib.ftl_last_error()
    assert _act(lib, handle, out) == abi.FTL_E_STATE                                # every argument fine: only the state is missing
    assert b"ftl_bind_state" in lib.ftl_last_error()


def test_rollout_argument_checks(lib, handle):
    out = _outputs()
    assert _rollout(lib, None, out, _ro()) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, None, _ro()) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, out, None) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, out, _ro(), bl=None) == abi.FTL_E_INVALID
    for field in ("ret", "steps", "status"):
        assert _rollout(lib, handle, out, _ro(**{field: None})) == abi.FTL_E_INVALID
        assert field.encode() in lib.ftl_last_error()
    for T in (0, -2):
        assert _rollout(lib, handle, out, _ro(), T=T) == abi.FTL_E_INVALID
        assert b"T" in lib.ftl_last_error()
    for r in RESETS:
        for flags in (r, r | abi.FTL_STEP_NO_SENSORS):
            assert _rollout(lib, handle, out, _ro(), flags=flags) == abi.FTL_E_INVALID
            assert b"FTL_STEP_NO_SENSORS" in lib.ftl_last_error()
    for cap in (1, 0):
        assert _rollout(lib, handle, out, _ro(), cap=cap) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, out, _ro(), bl_bytes=N * ROW - 1) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, out, _ro(), bl=FAKE + 4) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, out, _ro(), actions=FAKE, step_bytes=N * 16 - 1) == abi.FTL_E_INVALID
    assert b"step_bytes" in lib.ftl_last_error()
    for kw in (dict(), dict(flags=abi.FTL_STEP_NO_SENSORS), dict(actions=FAKE, step_bytes=N * 16), dict(actions=FAKE, step_bytes=10 * N * 16)):
        assert _rollout(lib, handle, out, _ro(), **kw) == abi.FTL_E_STATE           # only the state is missing
        assert b"ftl_bind_state" in lib.ftl_last_error()


def test_python_surface_needs_no_device():
    import inspect
    from continiousenvironment_follower_leader_amd.baseline import BaselineFollower
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    assert inspect.signature(BaselineFollower.__init__).parameters["cap"].default == 64
    for cls in (VecGame, PipelinedVecGame):
        p = inspect.signature(cls.rollout_baseline).parameters
        assert list(p)[1:] == ["follower", "T", "gamma", "sensors", "record"]
        assert (p["gamma"].default, p["sensors"].default, p["record"].default) == (1.0, True, False)
    for name in ("act", "flags", "stack_len", "__call__"):
        assert callable(getattr(BaselineFollower, name))

    class FakeBatch:
        n, device = 4, "cpu"
    for kw in (dict(discrete_action_space=True, add_obstacles=False, path_finding_algorythm="astar"), dict(constant_follower_speed=True)):
        FakeBatch.cfg = make_config(**kw)
        with pytest.raises(ValueError, match="Box\\(2\\)"):
            BaselineFollower(FakeBatch())
