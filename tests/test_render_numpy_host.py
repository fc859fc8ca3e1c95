"""Host-side checks of what the render edge tests rely on (no GPU):
  * the reference rasteriser (tests/render_numpy.py), which paints a primitive only inside a +-2 px window around its bounding box, against
    a brute-force evaluation of the coverage rules of include/ftl.h over the whole image;
  * ``scene_prims`` against ``render_scene`` and against the list lengths the header implies;
  * the preconditions of the crafted scenes (tests/render_scenes.py): empty band of the dyadic scenes, the pairs at the chunk edges;
  * a float32 emulation of the device's ``overlaps`` / ``covers`` (csrc/ftl_render.hpp; the library is built with -ffp-contract=off, so
    numpy float32 arithmetic rounds as the device does) against the float64 reference, which confirms the range include/ftl.h states for
    the 1e-3 rule: primitives whose output-pixel coordinates and sizes stay within 2048."""
import math

import numpy as np
import pytest

from continiousenvironment_follower_leader_amd import abi
import render_scenes as rs
from render_numpy import RED, TOL, Raster, prim_bbox, render_prims, render_scene, scene_prims

F = np.float32
RANGE = 2048.0          # include/ftl.h, coverage rules: the 1e-3 rule is guaranteed up to this magnitude of output-pixel coordinates


# ---- primitives in output pixels ------------------------------------------------------------------------------------------------------
def to_px(p, scale=1.0, origin=(0.0, 0.0)):
    """A ``scene_prims`` entry as (type, float64 parameters in output pixels) in the parameter order of the device's Prim."""
    s, ox, oy = float(F(scale)), float(F(origin[0])), float(F(origin[1]))
    X, Y, g, k = (lambda x: (x - ox) / s), (lambda y: (y - oy) / s), p["g"], p["kind"]
    if k == "disc": return "disc", (X(g[0]), Y(g[1]), g[2] / s, -1.0)
    if k == "ring": return "disc", (X(g[0]), Y(g[1]), g[2] / s, g[2] / s - max(g[3] / s, 1.0))
    if k == "seg": return "seg", (X(g[0]), Y(g[1]), X(g[2]), Y(g[3]), 0.5 * max(g[4] / s, 1.0))
    if k == "robot":
        t = math.radians(g[2])
        return "rrect", (X(g[0]), Y(g[1]), math.cos(t), math.sin(t), 0.5 * g[3] / s, 0.5 * g[4] / s)
    if k == "box": return "rrect", (X(g[0] + 0.5 * g[2]), Y(g[1] + 0.5 * g[3]), 1.0, 0.0, 0.5 * g[2] / s, 0.5 * g[3] / s)
    if k == "outline": return "outline", (X(g[0]), Y(g[1]), X(g[0] + g[2]), Y(g[1] + g[3]))
    raise ValueError(k)


def covers(t, g, px, py, dt):
    """The coverage rules of include/ftl.h for every pixel centre (px, py), evaluated in ``dt``: float64 = the rules themselves, float32 =
    the device's ``covers`` operation by operation on the float32 parameters it stores."""
    g = [dt(v) for v in g]
    px, py = px.astype(dt), py.astype(dt)
    if t == "disc":
        dx, dy = px - g[0], py - g[1]
        d2 = dx * dx + dy * dy
        return (d2 <= g[2] * g[2]) & ((g[3] < 0) | (d2 > g[3] * g[3]))
    if t == "seg":
        ex, ey = g[2] - g[0], g[3] - g[1]
        l2 = ex * ex + ey * ey
        u = ((px - g[0]) * ex + (py - g[1]) * ey) / l2 if l2 > 0 else np.zeros(np.broadcast(px, py).shape, dt)
        u = np.minimum(np.maximum(u, dt(0)), dt(1))
        qx, qy = (g[0] + u * ex) - px, (g[1] + u * ey) - py
        return qx * qx + qy * qy <= g[4] * g[4]
    if t == "rrect":
        dx, dy = px - g[0], py - g[1]
        a, b = dx * g[2] + dy * g[3], dy * g[2] - dx * g[3]
        return (np.abs(a) <= g[4]) & (np.abs(b) <= g[5])
    if t == "outline":
        one = dt(1)
        inside = (px >= g[0]) & (px < g[2]) & (py >= g[1]) & (py < g[3])
        return inside & ((px < g[0] + one) | (px >= g[2] - one) | (py < g[1] + one) | (py >= g[3] - one))
    raise ValueError(t)


def overlaps(t, g, x0, y0, x1, y1):
    """The device's bounding-box cull of a tile with pixel centres [x0, x1] x [y0, y1], in float32."""
    g = [F(v) for v in g]
    m = F(0.01)
    if t == "disc": a0, a1, b0, b1 = g[0] - g[2], g[0] + g[2], g[1] - g[2], g[1] + g[2]
    elif t == "seg": a0, a1, b0, b1 = min(g[0], g[2]) - g[4], max(g[0], g[2]) + g[4], min(g[1], g[3]) - g[4], max(g[1], g[3]) + g[4]
    elif t == "rrect":
        ex, ey = abs(g[2]) * g[4] + abs(g[3]) * g[5], abs(g[3]) * g[4] + abs(g[2]) * g[5]
        a0, a1, b0, b1 = g[0] - ex, g[0] + ex, g[1] - ey, g[1] + ey
    else: a0, a1, b0, b1 = g[0], g[2], g[1], g[3]
    return bool(a1 + m >= F(x0) and a0 - m <= F(x1) and b1 + m >= F(y0) and b0 - m <= F(y1))


def grid(w, h):
    return np.arange(w, dtype=np.float64)[None, :] + 0.5, np.arange(h, dtype=np.float64)[:, None] + 0.5


def device_cover(t, g, w, h):
    """What the tile kernel decides for one primitive: culled per 32 x 32 tile by ``overlaps``, then ``covers`` in float32."""
    px, py = grid(w, h)
    out = np.broadcast_to(covers(t, g, px, py, F), (h, w)).copy()
    for ty in range(0, h, 32):
        for tx in range(0, w, 32):
            if not overlaps(t, g, tx + 0.5, ty + 0.5, min(tx + 32, w) - 0.5, min(ty + 32, h) - 0.5):
                out[ty:ty + 32, tx:tx + 32] = False
    return out


def paint_px(ras, t, g, rgb=RED):
    if t == "disc": ras.disc_px(g[0], g[1], g[2], g[3], rgb)
    elif t == "seg": ras.seg_px(*g, rgb)
    elif t == "rrect": ras.rrect_px(*g, rgb)
    else: ras.outline_px(*g, rgb)


# ---- the reference against brute force ---------------------------------------------------------------------------------------------------
def _random_prims(rng, n, w, h, dyadic):
    q = (lambda v: np.round(np.asarray(v) * 4) / 4) if dyadic else (lambda v: np.asarray(v))
    out = []
    for _ in range(n):
        c = q(rng.uniform(-10, [w + 10, h + 10]))
        kind = rng.integers(6)
        if kind == 0: out.append(("disc", (c[0], c[1], float(q(rng.uniform(0.25, 30))), -1.0)))
        elif kind == 1:
            r = float(q(rng.uniform(0.25, 30)))
            out.append(("disc", (c[0], c[1], r, r - float(q(rng.choice([1.0, 2.0, 0.25 + r])) if dyadic else rng.choice([1.0, 2.0, 0.3 + r])))))
        elif kind == 2:
            d = q(rng.uniform(-40, 40, 2)) * (rng.integers(4) > 0)            # every fourth has zero length
            if dyadic:
                d[rng.integers(2)] = 0.0                                        # axis-aligned
            out.append(("seg", (c[0], c[1], c[0] + d[0], c[1] + d[1], float(rng.choice([0.5, 1.5, 0.75])))))
        elif kind == 3:
            t = rng.choice([0.0, 0.5 * math.pi]) if dyadic else rng.uniform(0, 2 * math.pi)
            out.append(("rrect", (c[0], c[1], round(math.cos(t), 15) if dyadic else math.cos(t), round(math.sin(t), 15) if dyadic else math.sin(t),
                                  float(q(rng.uniform(0.25, 25))), float(q(rng.uniform(0.25, 25))))))
        elif kind == 4:
            x0, y0 = np.floor(c)
            out.append(("outline", (x0, y0, x0 + rng.integers(1, 30), y0 + rng.integers(1, 30))))
        else:
            x0, y0 = np.floor(c)
            out.append(("outline", (x0, y0, x0 + 1.0, y0 + 1.0)))             # a 1 x 1 outline
    return out


@pytest.mark.parametrize("dyadic", [False, True])
def test_windowed_reference_equals_brute_force(dyadic):
    rng = np.random.default_rng(3 + dyadic)
    kinds = set()
    for w, h in ((70, 45), (33, 31), (5, 3), (1, 1)):
        prims = _random_prims(rng, 160, w, h, dyadic)
        ras = Raster(w, h)
        owner = np.full((h, w), -1)
        px, py = grid(w, h)
        for i, (t, g) in enumerate(prims):
            paint_px(ras, t, g, 1000 * (i + 1))                                 # its own colour: the last one that covers a pixel owns it
            owner[np.broadcast_to(covers(t, g, px, py, np.float64), (h, w))] = i
            kinds.add((t, g[3] < 0) if t == "disc" else t)
        rgb = np.where(owner >= 0, 1000 * (owner + 1), 0xFFFFFF)
        assert np.array_equal(ras.img, np.stack([rgb >> 16, (rgb >> 8) & 255, rgb & 255], -1).astype(np.uint8)), (w, h, dyadic)
        if dyadic:
            assert ras.band.sum() == 0
    assert kinds == {("disc", True), ("disc", False), "seg", "rrect", "outline"}


def test_degenerate_primitives():
    px, py = grid(8, 8)
    # a zero-length segment is a disc of its half width; a ring whose inner radius is negative is a filled disc; a 1 x 1 outline is its pixel
    for (t, g), want in ((("seg", (3.5, 3.5, 3.5, 3.5, 1.5)), covers("disc", (3.5, 3.5, 1.5, -1.0), px, py, np.float64)),
                         (("disc", (3.25, 4.0, 0.625, -0.375)), covers("disc", (3.25, 4.0, 0.625, -1.0), px, py, np.float64)),
                         (("outline", (2.0, 5.0, 3.0, 6.0)), (px == 2.5) & (py == 5.5))):
        ras = Raster(8, 8)
        paint_px(ras, t, g)
        assert np.array_equal((ras.img != 255).any(-1), np.broadcast_to(want, (8, 8))) and want.any(), (t, g)
        assert np.array_equal(device_cover(t, g, 8, 8), np.broadcast_to(want, (8, 8)))


# ---- scene_prims ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rs.EPISODES))
def test_scene_prims_lengths_on_the_golden_scenes(name):
    cfg, scen, z = rs.golden_config(name)
    c = cfg.c
    sp = rs.Spec(cfg, scen)                                                     # the world of the episode, robots at their start
    sp.lasers[:] = 50.0
    sc = sp.scene()
    props = rs.sensor_properties(cfg)
    rlen = len(z["scen:route"])
    want = {abi.RENDER_PATH: (rlen - 1 if rlen > 2 else 0) + (c.n_static >= 2) + (rlen >= 1), abi.RENDER_BOX: 1,
            abi.RENDER_OBJECTS: cfg.n_robots + c.n_static, abi.RENDER_OBJECTS | abi.RENDER_RECTS: 2 * (cfg.n_robots + c.n_static),
            abi.RENDER_RECTS: 0, abi.RENDER_TARGET: 1,
            abi.RENDER_SENSORS: sum(p["count"] * (1 + (0 if p["kind"] == "compas" else 1 if p["kind"] in ("explicit", "lenient") else p["history"]))
                                    for p in props)}
    for layers, n in want.items():
        assert len(scene_prims(cfg, sc, layers)) == n, (name, layers)
    every = scene_prims(cfg, sc, abi.RENDER_ALL)
    assert len(every) == sum(n for l, n in want.items() if l not in (abi.RENDER_OBJECTS, abi.RENDER_RECTS)) <= rs.list_cap(cfg)
    assert len(scene_prims(cfg, sc, abi.RENDER_SENSORS, lasers=False)) == sum(p["count"] for p in props)
    fx, fy = (float(v) for v in sc["rb_pos"][1])
    view = (192, 128, 2.0, (fx - 192.0, fy - 128.0))
    img, band = render_scene(cfg, sc, *view)
    img2, band2 = render_prims(every, *view)
    assert np.array_equal(img, img2) and np.array_equal(band, band2) and (img != 255).any()
    for p in every[:200]:
        b = prim_bbox(p, 2.0, view[3])
        t, g = to_px(p, 2.0, view[3])
        px, py = grid(192, 128)
        cov = np.broadcast_to(covers(t, g, px, py, np.float64), (128, 192))
        if cov.any():                                                           # the box holds every covered pixel centre
            jj, ii = np.nonzero(cov)
            assert b[0] <= ii.min() + 0.5 and ii.max() + 0.5 <= b[2] and b[1] <= jj.min() + 0.5 and jj.max() + 0.5 <= b[3], (p, b)


def test_scenario_outside_the_pool():
    cfg, scen, _ = rs.tracker_only_config()
    sp = rs.chunk_spec(cfg, scen, 12, 30, 20)
    inside = scene_prims(cfg, sp.scene(0, 8), abi.RENDER_ALL)
    for s in (-1, 8):
        sp.scen = s
        sc = sp.scene(0, 8)
        assert sc["pool"] is None
        out = scene_prims(cfg, sc, abi.RENDER_ALL)
        secs = {p["section"] for p in out}
        assert not secs & {"route", "bridge", "finish"} and not any(k.startswith("static") for k in secs)
        assert out[-1]["section"] == "target" and out[-1]["g"][:2] == (44.5, 50.5)              # at the leader's current position
        assert len(inside) - len(out) == 12 + 2 + 2 * cfg.c.n_static


# ---- preconditions of the crafted scenes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(rs.CHUNK_CASES))
def test_chunk_scenes_hold_their_precondition(n):
    cfg, scen, _ = rs.tracker_only_config()
    layers, A, gc, cnt = rs.CHUNK_CASES[n]
    prims = scene_prims(cfg, rs.chunk_spec(cfg, scen, A, gc, cnt).scene(), layers)
    assert len(prims) == n
    assert rs.chunk_pair_problems(prims, rs.CHUNK_W, rs.CHUNK_H, rs.CHUNK_TILE, render_prims, prim_bbox) == []
    for p in rs.chunk_edges(n):                                                 # the pairs the issue names
        assert p in (n - 512, n - 256) and prims[p - 1]["rgb"] != prims[p]["rgb"]
    assert sorted(rs.CHUNK_CASES) == [1, 2, 255, 256, 257, 511, 512, 513, 768, 1023, 1024, 1025, 1537]


def test_dyadic_scenes_are_exact_in_float32():
    cfg, scen, _ = rs.tracker_only_config()
    ties = 0
    for shift in ((0, 0), (-3, 2), (5, -1)):
        prims = scene_prims(cfg, rs.dyadic_spec(cfg, scen, shift).scene(), abi.RENDER_ALL)
        assert {p["kind"] for p in prims} == {"disc", "ring", "seg", "robot", "box", "outline"}
        for scale in rs.DYADIC_SCALES:
            for origin in ((0.0, 0.0), (-3.25, 1.5)):
                img, band, tie = render_prims(prims, 36, 40, scale, origin, ties=True)
                assert band.sum() == 0
                ties += int(tie.sum())
                dev = np.full((40, 36), -1)
                for i, p in enumerate(prims):                                   # the float32 emulation of the device draws the same image
                    t, g = to_px(p, scale, origin)
                    assert all(float(F(v)) == v for v in g)                     # stored without rounding
                    dev[device_cover(t, g, 36, 40)] = i
                ref = np.full((40, 36), -1)
                px, py = grid(36, 40)
                for i, p in enumerate(prims):
                    t, g = to_px(p, scale, origin)
                    ref[np.broadcast_to(covers(t, g, px, py, np.float64), (40, 36))] = i
                assert np.array_equal(dev, ref), (shift, scale, origin)
    assert ties > 1000


# ---- float32 emulation of the device's coverage over the claimed range ---------------------------------------------------------------------
def _crossing_prims(rng, n, M, win=192):
    """Primitives with coordinates and sizes up to M output pixels whose boundary passes through the window [0, win]^2."""
    out = []
    for i in range(n):
        b = rng.uniform(0, win, 2)                                              # a boundary point inside the window
        th = rng.uniform(0, 2 * math.pi)
        d = np.array([math.cos(th), math.sin(th)])
        size = M * rng.uniform(0.05, 1.0)
        kind = i % 5
        if kind == 0:
            c = b + size * d
            out.append(("disc", (c[0], c[1], size, -1.0)))
        elif kind == 1:
            c = b + size * d
            out.append(("disc", (c[0], c[1], size, size - rng.choice([1.0, 2.0, 3.7]))))
        elif kind == 2:
            hw = float(rng.choice([0.5, 1.5, 4.0]))
            a = b + hw * np.array([-d[1], d[0]]) - d * size * rng.uniform(0, 1)
            e = a + d * size
            out.append(("seg", (a[0], a[1], e[0], e[1], hw)))
        elif kind == 3:
            hw, hh = size * 0.5, size * rng.uniform(0.05, 0.5)
            c = b - d * hw + np.array([-d[1], d[0]]) * rng.uniform(-hh, hh)
            out.append(("rrect", (c[0], c[1], d[0], d[1], hw, hh)))
        else:
            x0, y0 = np.floor(b) + rng.choice([0.0, 0.3, 0.5], 2)
            out.append(("outline", (x0, y0, x0 + math.floor(size) + 1.0, y0 + math.floor(size * rng.uniform(0.1, 1)) + 1.0)))
    return out


def emulation_table(mags=(256.0, 1024.0, 2048.0, 8192.0, 32768.0, 131072.0), n=200, seed=17):
    """Per magnitude M: (M, primitives, compared pixels, differing pixels inside the band, outside the band)."""
    rows = []
    for M in mags:
        rng = np.random.default_rng(seed)
        inside = outside = pixels = 0
        for t, g in _crossing_prims(rng, n, M):
            ras = Raster(192, 192)
            paint_px(ras, t, g)
            ref = (ras.img != 255).any(-1)
            diff = device_cover(t, g, 192, 192) != ref
            inside += int((diff & ras.band).sum())
            outside += int((diff & ~ras.band).sum())
            pixels += diff.size
        rows.append((M, n, pixels, inside, outside))
    return rows


def test_float32_coverage_meets_the_band_within_the_claimed_range():
    rows = emulation_table()
    for M, n, pixels, inside, outside in rows:
        print("EMULATION magnitude %8.0f primitives %d pixels %d differing in the band %d outside %d" % (M, n, pixels, inside, outside))
    # u = 2^-24; the longest chain of roundings in covers() (the segment's closest point) puts at most 8 u M on a distance: 8 u M <= 1e-3
    assert 8 * 2.0 ** -24 * RANGE <= TOL
    assert {M for M, *_ in rows if M <= RANGE} == {256.0, 1024.0, 2048.0}
    for M, n, pixels, inside, outside in rows:
        if M <= RANGE:
            assert outside == 0, (M, outside)


def test_sensors_that_draw_one_row_keep_one_row():
    """The list kernel reads output row ``history - rows + r`` of a sensor that draws ``rows`` of its ``history`` rows.  The two differ only
    for the sensors that draw the newest row alone (explicit angles / lenient), and the config layer gives those a history of 1 -- so
    replacing that row index by ``r`` changes no reachable picture, and no GPU test can tell the two apart.  Should such a sensor ever
    get a longer history, this test fails: tests/test_gpu_render_edges.py group E then needs a config of that kind."""
    cfgs = [rs.golden_config(n)[0] for n in sorted(rs.EPISODES)] + [rs.fuzz_config(s)[0] for s in range(0, 96)]
    kinds = set()
    for cfg in cfgs:
        for p in rs.sensor_properties(cfg):
            kinds.add(p["kind"])
            if p["kind"] in ("explicit", "lenient"):
                assert p["history"] == 1, p
    assert kinds == {"prev", "explicit", "lenient", "compas"}
