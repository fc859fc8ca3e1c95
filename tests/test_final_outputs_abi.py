"""C-ABI of the terminal-observation modes without a GPU: the ctypes mirror of ftl_final_outputs, the step flags of include/ftl.h,
and the argument checks of ftl_step_final that run before any device work."""
import ctypes as C
import os
import re

import pytest

from continiousenvironment_follower_leader_amd import _lib, abi, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _header_define(name):
    src = open(os.path.join(ROOT, "include", "ftl.h")).read()
    m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, src)
    assert m, name
    return int(m.group(1))


def test_final_outputs_struct_size(lib):
    assert lib.ftl_sizeof_final_outputs() == C.sizeof(abi.FinalOutputs)
    assert [f[0] for f in abi.FinalOutputs._fields_] == ["obs_num", "lasers", "target", "policy_obs", "ended", "restarted"]


def test_step_flags_match_the_header():
    assert abi.FTL_STEP_AUTO_RESET == _header_define("FTL_STEP_AUTO_RESET") == 1
    assert abi.FTL_STEP_NEXT_RESET == _header_define("FTL_STEP_NEXT_RESET") == 4
    assert "ftl_step_final" in _lib.EXPORTS


def test_step_final_rejects_both_reset_modes_before_touching_the_device(lib):
    cfg = make_config(bear_number=1)
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), 4, 0, C.byref(h)) == 0
    try:
        out, fin = abi.Outputs(), abi.FinalOutputs()
        fake_action = C.c_void_p(256)        # never dereferenced: the flags are checked first
        both = abi.FTL_STEP_AUTO_RESET | abi.FTL_STEP_NEXT_RESET
        assert lib.ftl_step_final(h, fake_action, abi.FTL_ACTION_BOX2, C.byref(out), C.byref(fin), both, None) == abi.FTL_E_INVALID
        assert b"exclude" in lib.ftl_last_error()
        assert lib.ftl_step_encoded(h, fake_action, abi.FTL_ACTION_BOX2, C.byref(out), both, None) == abi.FTL_E_INVALID
        assert lib.ftl_step_final(None, fake_action, abi.FTL_ACTION_BOX2, C.byref(out), None, 0, None) == abi.FTL_E_INVALID
    finally:
        lib.ftl_destroy(h)


def test_step_mode_argument_is_checked():
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    g = VecGame.__new__(VecGame)          # _step_mode needs no device
    g._fin = None
    assert g._step_mode(False) == (0, None) and g._step_mode(True) == (abi.FTL_STEP_AUTO_RESET, None)
    assert g._step_mode("next_step") == (abi.FTL_STEP_NEXT_RESET, None)
    with pytest.raises(ValueError):
        g._step_mode("same_step")         # needs final_obs=True
    with pytest.raises(ValueError):
        g._step_mode("sometimes")
