"""The cases of tests/ray_edge_cases.py on the ORACLE alone (CPU).  For every case: the oracle's readings equal the records the
unmodified reference's sensor classes gave on the same states (tests/golden/ray_edges.npz, written by tests/golden/gen/make_golden_rays.py),
the world has the shape the case is built for (`table_counts`, a numpy restatement of the kernel's counting, and the oracle's own
readings), and the margin condition holds: in float64 no rect corner and no corridor vertex lies within 1e-3 px of a ray of a sensor
that reacts to it, in any compared state -- so none of the readings tests/test_gpu_ray_edges.py compares is a knife edge, and that
file may insist on zero corner waivers.  `pytest -s` prints the counts."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_edge_cases as X
from golden_util import GOLDEN, close

_Z = {}


def _records():
    if not _Z:
        z = np.load(os.path.join(GOLDEN, "ray_edges.npz"))
        _Z.update({k: z[k] for k in z.files})
    return _Z


def _check_common(case):
    """Records, margin, error words; returns the smallest margin."""
    cfg, name = case["cfg"], case["name"]
    z = _records()
    assert name in z, "tests/golden/ray_edges.npz has no records of %s: run tests/golden/gen/make_golden_rays.py" % name
    assert list(z[name + "/envs"]) == case["golden"]
    ora = np.stack([np.stack([r["lasers"] for r in case["trace"][e]]) for e in case["golden"]])
    assert ora.shape == z[name].shape, (name, ora.shape, z[name].shape)
    assert close(ora, z[name]).all(), (name, "the oracle against the reference's records", float(np.abs(ora - z[name]).max()))
    worst = min(X.margin(cfg, recs, t, case["scen"][e]["static_rects"], case["per_class"]) for e, recs in enumerate(case["trace"]) for t in range(len(recs)))
    assert worst >= X.MARGIN, (name, "a corner or corridor vertex within %g px of a ray" % X.MARGIN, worst)
    assert all(r["err"] == 0 for recs in case["trace"] for r in recs), (name, "error word")
    print("ray_edges %-22s %6d readings against the reference, %d not bit-identical; smallest margin %.3g px; %d envs done at the end; "
          "%d worlds moved while settling" % (name, ora.size, int((ora != z[name]).sum()), worst, sum(r[-1]["done"] for r in case["trace"]), case["trials"]))
    return worst


def _names(group):
    return [n for n in X.case_names() if n.startswith(group + "-")]


@pytest.mark.parametrize("name", _names("A"))
def test_group_a_every_source_is_in_the_table(name):
    """n_static + H * (1 + bears) sources on either side of one wavefront; every static rect and the leader of every valid snapshot
    inside the static class box at the reset and after every step; snap_head wraps (H + 3 steps)."""
    case = X.get_case(name)
    _check_common(case)
    cfg = case["cfg"]
    n_static, bears, H = cfg.c.n_static, cfg.c.n_bears, cfg.lasers[0].history
    assert case["expect"]["sources"] == n_static + H * (1 + bears) and case["steps"] == H + 3 and case["n"] == 16
    assert H * (1 + bears) <= X.FTL_WAVE
    for e in range(case["n"]):
        for t in range(case["steps"] + 1):
            tc = X.table_counts(cfg, X.state_at(case, e, t))[1]
            assert tc["static_in"] == n_static, (name, e, t, tc)
            assert tc["leaders_in"] == min(t + 1, H), (name, e, t, tc)
            assert tc["dynamic_in"] == bears * min(t + 1, H), (name, e, t, "the bears of every valid snapshot inside the dynamic box", tc)
    assert not any(r["done"] for recs in case["trace"] for r in recs), (name, "an env ended")


@pytest.mark.parametrize("name", _names("B"))
def test_group_b_runs_end_on_the_chunk_edge(name):
    case = X.get_case(name)
    _check_common(case)
    kind, target = case["expect"]["kind"], case["expect"]["target"]
    for e in range(case["n"]):
        tc = X.table_counts(case["cfg"], X.state_at(case, e, 0))[1]
        if kind == "static":
            assert tc["static_edges"] == target == tc["n_items"], (name, e, tc)
        else:
            ends = {"run-static": tc["static_edges"], "run-dynamic": tc["static_edges"] + tc["dynamic_edges"],
                    "run-corridor": tc["static_edges"] + tc["dynamic_edges"] + tc["corridor"]}[kind]
            assert ends % X.FTL_WAVE == target % X.FTL_WAVE and ends >= target, (name, e, tc)
            assert tc["dynamic_edges"] > 0 and tc["corridor"] > 0 and tc["green"] == 2 and tc["n_items"] > ends, (name, e, tc)
    assert not any(r[-1]["done"] for r in case["trace"]), (name, "an env ended")


@pytest.mark.parametrize("name", _names("C"))
def test_group_c_rects_around_the_follower(name):
    case = X.get_case(name)
    _check_common(case)
    cfg, rays = case["cfg"], case["expect"]["rays"]
    assert sum(l.count for l in cfg.lasers if l.after_tracker) == rays
    for e in range(case["n"]):
        place = X.C_PLACES[e % 3]
        for t in range(case["steps"] + 1):
            st = X.state_at(case, e, t)
            near = st["static"][:3 if place == "nested" else 1]
            if place != "border" or t == 0:          # (a follower that creeps off the border sees one edge of that rect)
                assert (X.facing_edges(st["fpos"], near) == 4).all() and X.in_box(st["fpos"], near, 102.0).all(), (name, e, t, place)
            k = X.edges_within_2px(st["fpos"].astype(np.float64), near)
            if place == "nested":
                assert k >= 8, (name, e, t, k)
                if rays >= 36:
                    assert k * rays > X.FTL_PAIR_CAP, (name, e, t, k)
            if place == "border" and t == 0:
                assert k >= 1 and float(st["fpos"][0]) == float(near[0][0]), (name, e, k)
    assert not any(r[-1]["done"] for r in case["trace"]), (name, "an env ended")


@pytest.mark.parametrize("name", _names("D"))
def test_group_d_every_ray_meets_a_rect(name):
    case = X.get_case(name)
    _check_common(case)
    cfg = case["cfg"]
    assert case["n"] == 720 and [s["robot_dir"][1] for s in case["scen"]] == [0.5 * e for e in range(720)]
    for l in cfg.lasers:
        hit = np.zeros(l.count, bool)
        for e, recs in enumerate(case["trace"]):
            for r in recs:
                # a hit counts only where the reading is the distance to the nearest ring rect along that ray (float64 slab test):
                # the leader and the pool's bear are obstacles of these sensors too
                ring = _ring_distance(r["fpos"].astype(np.float64), X.ray_angles(l, r["fdir"]), case["scen"][e]["static_rects"])
                got = X.newest_row(cfg, l, r["lasers"]).astype(np.float64)
                hit |= (ring < l.length - 1e-3) & (np.abs(got - ring) < 1e-3)
        assert hit.all(), (name, l.name, "ray indices that never stop on a ring rect", np.nonzero(~hit)[0])


def _ring_distance(pos, angles_deg, rects):
    """[rays]: distance along each ray from `pos` to the nearest of the axis-aligned `rects` (inf where it meets none), float64."""
    a = np.radians(angles_deg)
    d = np.stack([np.cos(a), np.sin(a)], 1)[:, None, :]                               # [rays, 1, 2]
    q = np.asarray(rects, np.float64).reshape(-1, 4)
    lo, hi = (q[:, :2] - pos)[None], (q[:, :2] + q[:, 2:] - pos)[None]               # [1, rects, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = lo / d, hi / d
    tn, tf = np.minimum(t0, t1).max(2), np.maximum(t0, t1).min(2)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf).min(1)


@pytest.mark.parametrize("name", _names("E"))
def test_group_e_rects_at_the_cull_boxes(name):
    case = X.get_case(name)
    _check_common(case)
    cfg = case["cfg"]
    by = {l.name: l for l in cfg.lasers}
    seen = set()
    for e, (cls, d, gap, over) in enumerate(case["places"]):
        l = by[cls]
        got = X.newest_row(cfg, l, case["trace"][e][0]["lasers"])[X.E_RAY[d]]
        if over < 0:
            assert l.length - 1.0 < got < np.float32(l.length), (name, e, cls, d, over, got)
        else:
            assert got == np.float32(l.length), (name, e, cls, d, over, got)
        f = case["trace"][e][0]["fpos"]
        assert float(f[0]) % 1.0 == 0.5 and float(f[1]) % 1.0 == 0.5
        seen.add((cls, d, round(float(over), 2)))
    assert len(seen) == len(case["places"]) == 2 * (4 * 4 + 4 * 3)
    for cls in ("static", "dynamic"):
        axis = sorted(o for c, d, o in seen if c == cls and d == (1, 0))
        assert axis == [-0.5, 0.5, 1.5, 2.5], axis


@pytest.mark.parametrize("name", _names("G"))
def test_group_g_1023_rays(name):
    case = X.get_case(name)
    _check_common(case)
    cfg = case["cfg"]
    assert sum(l.count for l in cfg.lasers) == 1023
    assert sorted({int(bool(l.after_tracker)) for l in cfg.lasers}) == ([0, 1] if "2pass" in name else [1])
    for l in cfg.lasers:
        assert any((X.newest_row(cfg, l, r["lasers"]) < np.float32(l.length)).any() for recs in case["trace"] for r in recs), (name, l.name)


def test_group_g_limits_of_ftl_create():
    """1024 rays are refused with the message about 10 bits; the largest n_static ftl_create accepts for a 12-ray, one-row sensor is the
    one the dense case uses, one more is refused under a 64 KiB LDS rule, and most of the dense world lies inside the reach box."""
    from continiousenvironment_follower_leader_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(X.too_many_rays_config().c), 8, 0, C.byref(h)) != 0
    assert "10 bits" in lib.ftl_last_error().decode()
    n, message = X.largest_n_static()
    assert "64 KiB of LDS" in message, message
    name = "G-dense-%d" % n
    assert name in _records(), "the largest accepted n_static changed to %d: run tests/golden/gen/make_golden_rays.py" % n
    case = X.get_case(name)
    _check_common(case)
    for e in range(case["n"]):
        tc = X.table_counts(case["cfg"], X.state_at(case, e, 0))[1]
        assert tc["static_in"] > 6 * X.FTL_WAVE and tc["static_edges"] > 12 * X.FTL_WAVE, (e, tc)


def test_table_counts_on_hand_made_states():
    """The counting model itself, on states small enough to count by hand."""
    cfg = X.config([("ahead", X.prev(24, 130, 3, "dynamic"))], [("rays", X.prev(36, 150, 3, "static", True, True))], 1, 4)
    assert X.class_reach(cfg, 0) == [-1.0, 132.0, -1.0, -1.0] and X.class_reach(cfg, 1) == [152.0, -1.0, 152.0, 152.0]
    f = np.array([500.5, 400.5], np.float32)
    static = [[496, 300, 8, 8],         # straight above: one edge
              [600, 500, 8, 8],         # diagonal: two
              [480, 380, 40, 40],       # around the follower: four
              [653, 400, 8, 8]]         # left edge 152.5 px to the right: outside the box of 152 (652 would be inside)
    snaps = [np.array([[560, 400, 19, 26], [400, 396, 25, 25]]), np.array([[900, 400, 19, 26], [380, 396, 25, 25]])]
    t0, t1 = X.table_counts(cfg, dict(fpos=f, static=static, snaps=snaps, corr=None))
    assert (t0["static_in"], t0["dynamic_in"], t0["dynamic_edges"], t0["static_edges"]) == (0, 2, 2, 0)
    assert (t1["static_in"], t1["leaders_in"], t1["static_edges"], t1["dynamic_in"]) == (3, 1, 1 + 2 + 4 + 1, 0)
    static[3][0] = 652
    assert X.table_counts(cfg, dict(fpos=f, static=static, snaps=snaps, corr=None))[1]["static_in"] == 4
    corr = np.array([[500, 390, 500, 410], [520, 390, 520, 410], [700, 390, 700, 410], [720, 390, 720, 410]], np.float64)
    t1 = X.table_counts(cfg, dict(fpos=f, static=static, snaps=snaps[:1], corr=corr))[1]
    assert (t1["corridor"], t1["green"]) == (4, 1) and t1["n_items"] == t1["static_edges"] + 5
