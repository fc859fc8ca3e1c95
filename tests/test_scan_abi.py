"""C-ABI checks of the on-demand sensor scans that need no GPU (include/ftl.h: FTL_STEP_NO_SENSORS, ftl_scan, ftl_rollout_outputs,
ftl_rollout): exports, the flag value and the struct mirror against the header, and the argument checks that come before any device
work."""
import ctypes as C
import os
import re

import pytest

from continiousenvironment_follower_leader_amd import _lib, abi, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftl_scan", "ftl_sizeof_rollout_outputs", "ftl_rollout")
FAKE = 4096      # a non-null "device pointer" that is never dereferenced: the checks under test come first
RESETS = (abi.FTL_STEP_AUTO_RESET, abi.FTL_STEP_NEXT_RESET, abi.FTL_STEP_QUEUE_RESET, abi.FTL_STEP_SAMPLE_RESET)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture()
def handle(lib):
    cfg = make_config(bear_number=1)
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), 4, 0, C.byref(h)) == 0, lib.ftl_last_error()
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


def _rollout(lib, h, out, ro, T=3, flags=0, actions=FAKE, enc=abi.FTL_ACTION_BOX2):
    return lib.ftl_rollout(h, actions, 64, enc, T, 1.0, C.byref(out) if out is not None else None, C.byref(ro) if ro is not None else None,
                           flags, None)


def test_symbols_declared_exported_and_listed(lib):
    hdr = _header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s


def test_flag_value_matches_the_header():
    assert int(re.search(r"#define\s+FTL_STEP_NO_SENSORS\s+(\d+)u", _header()).group(1)) == abi.FTL_STEP_NO_SENSORS == 32
    for r in RESETS:
        assert not abi.FTL_STEP_NO_SENSORS & r
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", _header()).group(1)) == abi.FTL_ABI_VERSION == 4


def test_rollout_outputs_mirror_matches_the_header(lib):
    body = re.search(r"typedef\s+struct\s+ftl_rollout_outputs\s*\{(.*?)\}\s*ftl_rollout_outputs\s*;", _header(), re.S).group(1)
    fields = [re.match(r"(\w+)\s*\*\s*(\w+)$", d.strip()).groups() for d in body.split(";") if d.strip()]
    assert fields == [("double", "ret"), ("int32_t", "steps"), ("uint8_t", "status")]
    assert [f[1] for f in fields] == [f[0] for f in abi.RolloutOutputs._fields_]
    assert all(f[1] is C.c_void_p for f in abi.RolloutOutputs._fields_)
    assert lib.ftl_sizeof_rollout_outputs() == C.sizeof(abi.RolloutOutputs) == 24


def test_scan_argument_checks(lib, handle):
    out = _outputs()
    assert lib.ftl_scan(None, C.byref(out), None) == abi.FTL_E_INVALID
    assert lib.ftl_scan(handle, None, None) == abi.FTL_E_INVALID
    assert lib.ftl_scan(handle, C.byref(out), None) == abi.FTL_E_STATE          # no state bound
    assert b"ftl_bind_state" in lib.ftl_last_error()


def test_rollout_argument_checks(lib, handle):
    out = _outputs()
    assert _rollout(lib, None, out, _ro()) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, None, _ro()) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, out, None) == abi.FTL_E_INVALID
    assert _rollout(lib, handle, out, _ro(), actions=None) == abi.FTL_E_INVALID
    for T in (0, -2):
        assert _rollout(lib, handle, out, _ro(), T=T) == abi.FTL_E_INVALID
        assert b"T" in lib.ftl_last_error()
    for r in RESETS:
        for flags in (r, r | abi.FTL_STEP_NO_SENSORS):
            assert _rollout(lib, handle, out, _ro(), flags=flags) == abi.FTL_E_INVALID
            assert b"FTL_STEP_NO_SENSORS" in lib.ftl_last_error()
    for field in ("ret", "steps", "status"):
        assert _rollout(lib, handle, out, _ro(**{field: None})) == abi.FTL_E_INVALID
        assert field.encode() in lib.ftl_last_error()
    assert _rollout(lib, handle, out, _ro(), enc=7) == abi.FTL_E_INVALID
    for flags in (0, abi.FTL_STEP_NO_SENSORS):                                      # every argument fine: only the state is missing
        assert _rollout(lib, handle, out, _ro(), flags=flags) == abi.FTL_E_STATE
        assert b"ftl_bind_state" in lib.ftl_last_error()


def test_reset_flags_still_exclude_each_other_with_the_sensor_flag(lib, handle):
    out, fin, act = _outputs(), abi.FinalOutputs(), C.c_void_p(FAKE)
    blind = abi.FTL_STEP_NO_SENSORS
    flags = abi.FTL_STEP_AUTO_RESET | abi.FTL_STEP_NEXT_RESET | blind
    assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), C.byref(fin), flags, None) == abi.FTL_E_INVALID
    assert lib.ftl_step_encoded(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), flags, None) == abi.FTL_E_INVALID
    assert lib.ftl_step(handle, act, C.byref(out), flags, None) == abi.FTL_E_INVALID
    for a, b in ((abi.FTL_STEP_QUEUE_RESET, abi.FTL_STEP_AUTO_RESET), (abi.FTL_STEP_SAMPLE_RESET, abi.FTL_STEP_NEXT_RESET),
                 (abi.FTL_STEP_QUEUE_RESET, abi.FTL_STEP_SAMPLE_RESET)):
        assert lib.ftl_step_encoded(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), a | b | blind, None) == abi.FTL_E_INVALID


def test_queue_and_sample_flags_combine_with_the_sensor_flag(lib, handle):
    """Without a queue / a sampler the combination gets as far as the attachment check (FTL_E_STATE), not FTL_E_INVALID."""
    out, act = _outputs(), C.c_void_p(FAKE)
    blind = abi.FTL_STEP_NO_SENSORS
    for step in (lambda f: lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), None, f, None),
                 lambda f: lib.ftl_step_encoded(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), f, None),
                 lambda f: lib.ftl_step(handle, act, C.byref(out), f, None)):
        assert step(abi.FTL_STEP_QUEUE_RESET | blind) == abi.FTL_E_STATE
        assert b"queue" in lib.ftl_last_error()
        assert step(abi.FTL_STEP_SAMPLE_RESET | blind) == abi.FTL_E_STATE
        assert b"sampler" in lib.ftl_last_error()
        for f in (blind, abi.FTL_STEP_AUTO_RESET | blind, abi.FTL_STEP_NEXT_RESET | blind):      # accepted: only the state is missing
            assert step(f) == abi.FTL_E_STATE
            assert b"ftl_bind_state" in lib.ftl_last_error()


def test_python_keywords_need_no_device():
    import inspect
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    for cls in (VecGame, PipelinedVecGame):
        assert inspect.signature(cls.step).parameters["sensors"].default is True
        assert inspect.signature(cls.rollout).parameters["sensors"].default is True
        assert inspect.signature(cls.rollout).parameters["gamma"].default == 1.0
        assert inspect.signature(cls.evaluate).parameters["sensors"].default is True
        assert callable(cls.scan)
    assert inspect.signature(PipelinedVecGame.step_part).parameters["sensors"].default is True
