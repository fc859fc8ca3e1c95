"""ftl_render without a GPU: the ctypes mirror of ftl_render_params, the layer bits of include/ftl.h, the argument checks that run
before any device work, and the numpy rasteriser of the spec (tests/render_numpy.py) on hand-built scenes with known answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from continiousenvironment_follower_leader_amd import _lib, abi, make_config
from render_numpy import RED, Raster, rgb_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "ftl.h")).read()


def test_render_params_struct(lib):
    assert lib.ftl_sizeof_render_params() == C.sizeof(abi.RenderParams) == 28
    names = [f[0] for f in abi.RenderParams._fields_]
    assert names == ["width", "height", "scale", "origin_x", "origin_y", "layers", "_pad"]
    assert [getattr(abi.RenderParams, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24]
    for n in ("ftl_sizeof_render_params", "ftl_render_workspace", "ftl_render"):
        assert n in _lib.EXPORTS and hasattr(lib, n)


def test_layer_bits_match_the_header():
    m = re.search(r"enum\s*\{\s*(FTL_RENDER_PATH[^}]*)\}", _header())
    assert m
    bits = {k: int(v) for k, v in re.findall(r"(FTL_RENDER_\w+)\s*=\s*(\d+)", m.group(1))}
    assert bits == dict(FTL_RENDER_PATH=abi.RENDER_PATH, FTL_RENDER_BOX=abi.RENDER_BOX, FTL_RENDER_OBJECTS=abi.RENDER_OBJECTS,
                        FTL_RENDER_RECTS=abi.RENDER_RECTS, FTL_RENDER_SENSORS=abi.RENDER_SENSORS, FTL_RENDER_TARGET=abi.RENDER_TARGET)
    assert abi.RENDER_ALL == sum(bits.values()) == int(re.search(r"#define\s+FTL_RENDER_ALL\s+(\d+)u", _header()).group(1))


def test_render_rejects_bad_arguments_before_device_work(lib):
    cfg = make_config(bear_number=1)
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), 4, 0, C.byref(h)) == 0
    try:
        k = 3
        need = C.c_size_t()
        assert lib.ftl_render_workspace(h, k, C.byref(need)) == 0 and need.value > 0
        assert lib.ftl_render_workspace(h, 0, C.byref(need)) == abi.FTL_E_INVALID
        assert lib.ftl_render_workspace(None, k, C.byref(need)) == abi.FTL_E_INVALID
        lib.ftl_render_workspace(h, k, C.byref(need))
        fake = C.c_void_p(256)             # never dereferenced: every check below fails before any device work

        def call(ids=fake, kk=k, ws=fake, nb=need.value, rgb=fake, **over):
            rp = abi.RenderParams()
            rp.width, rp.height, rp.scale, rp.layers = 64, 48, 1.0, abi.RENDER_ALL
            for a, v in over.items():
                setattr(rp, a, v)
            return lib.ftl_render(h, ids, kk, C.byref(rp), ws, nb, rgb, None)

        bad = [dict(kk=0), dict(kk=-1), dict(width=0), dict(height=-2), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(layers=64), dict(layers=abi.RENDER_ALL | 128), dict(ids=None), dict(ws=None),
               dict(rgb=None), dict(nb=need.value - 1)]
        for b in bad:
            assert call(**b) == abi.FTL_E_INVALID, b
        assert lib.ftl_render(h, fake, k, None, fake, need.value, fake, None) == abi.FTL_E_INVALID
        assert lib.ftl_render(None, fake, k, None, fake, need.value, fake, None) == abi.FTL_E_INVALID
        # the same call with valid arguments gets past every argument check and stops at the unbound state
        assert call() == abi.FTL_E_STATE
        assert call(layers=0) == abi.FTL_E_STATE
    finally:
        lib.ftl_destroy(h)


def test_render_params_of_the_show_flags():
    from continiousenvironment_follower_leader_amd.vec_game import _render_layers, _render_params
    assert _render_layers(make_config()) == abi.RENDER_ALL
    cfg = make_config(show_box_flag=False, show_sensors_flag=False, show_rectangles_flag=False)
    assert _render_layers(cfg) == abi.RENDER_PATH | abi.RENDER_OBJECTS | abi.RENDER_TARGET
    assert _render_layers(make_config(show_leader_path_flag=False, show_objects_flag=False)) == \
        abi.RENDER_ALL & ~(abi.RENDER_PATH | abi.RENDER_OBJECTS)
    rp, (w, h) = _render_params(make_config(), 4.0, None, (0, 0), None)
    assert (w, h) == (375, 250) and rp.width == 375 and rp.height == 250 and rp.layers == abi.RENDER_ALL
    with pytest.raises(ValueError):
        _render_params(make_config(), 0.0, None, (0, 0), None)


def _covered(ras, rgb=RED):
    return np.all(ras.img == rgb_of(rgb), axis=-1)


def test_numpy_disc_pixel_count():
    ras = Raster(40, 40)
    ras.disc(20.0, 20.0, 5.0, RED)          # pixel centres (i + 0.5, j + 0.5) with (i - 19.5)^2 + (j - 19.5)^2 <= 25
    want = sum(1 for i in range(40) for j in range(40) if (i + 0.5 - 20) ** 2 + (j + 0.5 - 20) ** 2 <= 25)
    assert _covered(ras).sum() == want == 80
    ras = Raster(40, 40)
    ras.disc(20.5, 20.5, 5.0, RED)          # centred on a pixel centre: ties d = 5 at (3, 4) offsets are covered (d <= r)
    assert _covered(ras).sum() == 81
    assert _covered(ras)[20, 25] and _covered(ras)[24, 23] and not _covered(ras)[20, 26]


def test_numpy_ring_pixel_counts():
    for w, want in ((1, 32), (2, 60)):
        ras = Raster(40, 40)
        ras.ring(20.0, 20.0, 6.0, w, RED)    # 6 - w < d <= 6
        cnt = sum(1 for i in range(40) for j in range(40) if 6 - w < np.hypot(i + 0.5 - 20, j + 0.5 - 20) <= 6)
        assert _covered(ras).sum() == cnt == want, (w, cnt)
    ras = Raster(40, 40, scale=4.0)          # a width-2 ring at scale 4 is max(2 / 4, 1) = 1 output pixel wide
    ras.ring(80.0, 80.0, 24.0, 2.0, RED)
    assert _covered(ras).sum() == 32


def test_numpy_rect_outline_is_pygames_border():
    ras = Raster(30, 20)
    ras.outline((3, 4, 10, 6))               # pygame.draw.rect(width=1): columns 3 and 12, rows 4 and 9 of the rect
    want = np.zeros((20, 30), bool)
    want[4, 3:13] = want[9, 3:13] = True
    want[4:10, 3] = want[4:10, 12] = True
    assert np.array_equal(_covered(ras), want) and want.sum() == 2 * 10 + 2 * 4
    ras = Raster(30, 20)
    ras.outline((5, 5, 1, 1))                # a 1x1 rect is its own border
    assert _covered(ras).sum() == 1 and _covered(ras)[5, 5]


def test_numpy_segment_ties_and_painter_order():
    ras = Raster(20, 20)
    ras.seg(10.0, 2.0, 10.0, 17.0, 1.0, RED)  # a 1-px line on an integer x: pixel centres 9.5 and 10.5 lie exactly 0.5 away -> both covered
    cols = np.nonzero(_covered(ras).any(axis=0))[0]
    assert list(cols) == [9, 10]
    ras.disc(10.0, 10.0, 3.0, 0x00FF00)       # the later primitive wins where both cover
    assert not _covered(ras)[9, 9] and np.all(ras.img[9, 9] == rgb_of(0x00FF00))
    ras = Raster(20, 20)
    ras.robot(10.0, 10.0, 90.0, 8.0, 4.0, RED)   # direction 90: the 8-px side along +y
    cov = _covered(ras)
    assert cov[:, 10].sum() == 8 and cov[10, :].sum() == 4


def test_numpy_green_zone_is_the_window_of_green_len():
    """green_zone_trajectory_points are built (ENV:968-969) before the frame's trajectory append (ENV:1074-1075): the window is taken on
    the EI_GREEN_LEN points the trajectory had then -- points green_len - 2 .. green_len - 1 - green_count -- not on the current length."""
    from render_numpy import GREEN, render_scene
    cfg = make_config(bear_number=1)
    c, R = cfg.c, cfg.n_robots
    gap = 3.0 * c.max_dev
    traj = np.zeros((c.traj_cap, 2), np.float32)
    traj[:10] = [(c.max_dev + gap * q, 100.0) for q in range(10)]
    ei = np.zeros(abi.EI_COUNT, np.int32)
    ei[abi.EI_TRAJ_LEN], ei[abi.EI_GREEN_LEN], ei[abi.EI_GREEN_COUNT] = 10, 9, 6
    pos = np.full((R, 2), -5000.0, np.float32)                 # the leader's min-distance ring off the image
    sc = dict(env_int=ei, rb_pos=pos, rb_dbl=np.zeros((R, abi.RD_COUNT)), rb_int=np.zeros((R, abi.RI_COUNT), np.int32), traj=traj,
              pool=dict(route_len=np.int32(0), route=np.zeros((c.route_cap, 2)), static_rects=np.zeros((c.n_static, 4), np.int32),
                        robot_pos=pos))
    img, _ = render_scene(cfg, sc, int(gap * 10 + 2 * c.max_dev), 200, layers=abi.RENDER_BOX)
    green = np.all(img == rgb_of(GREEN), axis=-1)
    drawn = [bool(green[100, int(traj[q, 0])]) for q in range(10)]
    assert drawn == [q in range(2, 8) for q in range(10)], drawn
    ei[abi.EI_GREEN_COUNT] = 5                                 # five points or fewer: no discs (ENV:1245)
    img, _ = render_scene(cfg, sc, int(gap * 10 + 2 * c.max_dev), 200, layers=abi.RENDER_BOX)
    assert not np.all(img == rgb_of(GREEN), axis=-1).any()
