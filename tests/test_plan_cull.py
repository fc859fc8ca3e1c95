"""The reach phase 1 of the ray kernel culls each segment class with, as ftl_create reports it under FTL_DEBUG_PRINT_LDS: one
continuation line per pass that has rays, `     ray cull: pass P static R dynamic R corridor R green R`, R = the longest laser_length + 2
among the pass's sensors that react to the class, or `none` ("The launch plan").  Pure host work.  The expected values are
written out here from the configs; nothing below asks the library what it should say."""
import ctypes as C
import re

import pytest

from golden_util import config_for, load_episode

TRACKER = "LeaderPositionsTracker_v2"
ALL, OBST = "LeaderCorridor_lasers_all", "LeaderCorridor_lasers_obstacles"      # config B: 12 rays / 100 px (all classes), 24 rays / 150 px (obstacles)
SWITCHES = ("FTL_RAYS_CLASS_CULL", "FTL_RAYS_ONE_PASS", "FTL_SPLIT", "FTL_DEBUG_CORR_LDS_CAP", "FTL_DEBUG_PAIR_WINDOW")
LINE = re.compile(r"^     ray cull: pass ([01]) static (\S+) dynamic (\S+) corridor (\S+) green (\S+)$", re.M)


@pytest.fixture(scope="module")
def lib():
    from continiousenvironment_follower_leader_amd import _lib
    _lib.build()
    return _lib.load()


@pytest.fixture
def env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("FTL_DEBUG_PRINT_LDS", "1")
    return monkeypatch


def _b_config(reacts=None, lengths=None, order=(TRACKER, ALL, OBST)):
    _, meta = load_episode("B_s1_chase")
    kw = dict(meta["kwargs"])
    src = {k: dict(v) for k, v in kw["follower_sensors"].items()}
    for k, (ro, rc, rg) in (reacts or {}).items():
        src[k].update(react_to_obstacles=ro, react_to_safe_corridor=rc, react_to_green_zone=rg)
    for k, length in (lengths or {}).items():
        src[k]["laser_length"] = length
    kw["follower_sensors"] = {k: src[k] for k in order}
    return config_for(dict(kwargs=kw, post=None), scen_route_len=256)


def _cull(lib, capfd, cfg):
    """{pass: (static, dynamic, corridor, green)} of the report's `ray cull:` lines, and the whole report."""
    capfd.readouterr()
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), 64, 0, C.byref(h)) == 0, lib.ftl_last_error().decode()
    err = capfd.readouterr().err
    lib.ftl_destroy(h)
    found = LINE.findall(err)
    assert err.count("ray cull:") == len(found), err
    assert err.count("ftl:") == 3, err                                         # continuation lines: no prefix of their own
    at = [m.start() for m in re.finditer(r"ray c", err)]
    if found:
        assert err.index("ray candidates:") == at[0] and len(at) == 1 + len(found), err     # they follow the `ray candidates:` line
    return {int(f[0]): f[1:] for f in found}, err


def test_config_B(lib, env, capfd):
    """Both sensors behind the tracker: pass 1 only.  Obstacles are seen by both sensors (150 + 2), corridor and green by the 100-px one."""
    rep, _ = _cull(lib, capfd, _b_config())
    assert rep == {1: ("152", "152", "102", "102")}


def test_roles_swapped(lib, env, capfd):
    rep, _ = _cull(lib, capfd, _b_config(reacts={ALL: (True, False, False), OBST: (False, True, True)}))
    assert rep == {1: ("102", "102", "152", "152")}


def test_obstacles_only_and_classes_apart(lib, env, capfd):
    rep, _ = _cull(lib, capfd, _b_config(reacts={ALL: (True, False, False), OBST: (True, False, False)}))
    assert rep == {1: ("152", "152", "none", "none")}
    # corridor without green, green without corridor, nobody sees the rects; lengths that are no integers keep their fraction
    rep, _ = _cull(lib, capfd, _b_config(reacts={ALL: (False, True, False), OBST: (False, False, True)}, lengths={ALL: 30.5, OBST: 45}))
    assert rep == {1: ("none", "none", "32.5", "47")}


def test_two_passes_have_a_table_each(lib, env, capfd):
    """Sensor "all" / tracker / sensor "obstacles": pass 0 sees every class at 102, pass 1 the rects at 152 and nothing else."""
    rep, _ = _cull(lib, capfd, _b_config(order=(ALL, TRACKER, OBST)))
    assert rep == {0: ("102", "102", "102", "102"), 1: ("152", "152", "none", "none")}


def test_switch_off_restores_one_box_per_pass(lib, env, capfd):
    """FTL_RAYS_CLASS_CULL=0: every class at the pass's longest laser + 2, a class nobody sees included (nothing is skipped); the lines
    of the report before `ray cull:` do not depend on the switch."""
    on = {}
    for name, cfg in (("B", _b_config()), ("obstacles", _b_config(reacts={ALL: (True, False, False), OBST: (True, False, False)})),
                      ("two", _b_config(order=(ALL, TRACKER, OBST)))):
        on[name] = _cull(lib, capfd, cfg)[1]
    env.setenv("FTL_RAYS_CLASS_CULL", "0")
    rep, err = _cull(lib, capfd, _b_config())
    assert rep == {1: ("152",) * 4} and err.split("     ray cull:")[0] == on["B"].split("     ray cull:")[0]
    rep, err = _cull(lib, capfd, _b_config(reacts={ALL: (True, False, False), OBST: (True, False, False)}))
    assert rep == {1: ("152",) * 4} and err.split("     ray cull:")[0] == on["obstacles"].split("     ray cull:")[0]
    rep, err = _cull(lib, capfd, _b_config(order=(ALL, TRACKER, OBST)))
    assert rep == {0: ("102",) * 4, 1: ("152",) * 4} and err.split("     ray cull:")[0] == on["two"].split("     ray cull:")[0]
    env.setenv("FTL_RAYS_CLASS_CULL", "1")
    assert _cull(lib, capfd, _b_config())[0] == {1: ("152", "152", "102", "102")}


def test_no_ray_sensor_no_line(lib, env, capfd):
    from continiousenvironment_follower_leader_amd import make_config
    rep, err = _cull(lib, capfd, make_config(bear_number=1))
    assert rep == {} and "ray c" not in err
