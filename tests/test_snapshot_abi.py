"""C-ABI checks of the env snapshot entry points that need no GPU (include/ftl.h: ftl_env_bytes, ftl_env_layout_id, ftl_pack_envs,
ftl_unpack_envs): exports, the stream word and flags against the header, the packed row size from the state field table, the layout id,
and the argument checks that come before any device work."""
import ctypes as C
import os
import re

import pytest

from continiousenvironment_follower_leader_amd import _lib, abi
from golden_util import config_for, load_episode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPISODES = {"B": "B_s1_chase", "D": "D_s2_chase", "E": "E_s3_chase", "F": "F_s1_chase", "L": "L_s2_chase", "T": "T_s3_chase"}
FIELDS = ("rb_pos", "rb_dbl", "rb_int", "env_int", "env_dbl", "traj", "hist", "corr", "snap_rects", "snap_win", "traj_bb", "ep_stats",
          "hist1", "fol_cs", "corr32")
SYMBOLS = ("ftl_env_bytes", "ftl_env_layout_id", "ftl_pack_envs", "ftl_unpack_envs")


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _cfg(name, **over):
    z, meta = load_episode(EPISODES[name])
    return config_for(meta, scen_route_len=len(z["scen:route"]), **over)


def _handle(lib, cfg, n=4):
    """A handle created host-only (ftl_create is layout + config freeze, as in tests/test_abi.py)."""
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), n, 0, C.byref(h)) == 0, lib.ftl_last_error()
    return h


def _fields(lib, h):
    out = {}
    for name in FIELDS:
        off, per, dt, st = C.c_size_t(), C.c_size_t(), C.c_int32(), C.c_size_t()
        assert lib.ftl_state_field(h, name.encode(), C.byref(off), C.byref(per), C.byref(dt), C.byref(st)) == 0
        out[name] = (off.value, per.value, (4, 4, 8)[dt.value], st.value)
    return out


def _up(v, a):
    return (v + a - 1) // a * a


def test_symbols_declared_exported_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "ftl.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s


def test_stream_word_and_flags_match_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ftl.h")).read(), flags=re.S)
    body = re.search(r"enum\s*\{\s*(FTL_EI_SCEN\b.*?)\};", hdr, re.S).group(1)
    names = [t.split("=")[0].strip() for t in body.split(",") if t.strip()]
    assert names.index("FTL_EI_STREAM") == abi.EI_STREAM
    assert names.index("FTL_EI_COUNT") == abi.EI_COUNT == abi.EI_STREAM + 1
    assert abi.EI_STREAM == abi.EI_ERROR_STICKY + 1
    for name, val in (("FTL_ENV_SLOT_STATS", abi.FTL_ENV_SLOT_STATS), ("FTL_ENV_OWN_STREAM", abi.FTL_ENV_OWN_STREAM)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, hdr).group(1)) == val


@pytest.mark.parametrize("name", ["B", "D", "F", "L", "T"])
def test_env_bytes_is_the_aligned_sum_of_the_fields(lib, name):
    h = _handle(lib, _cfg(name))
    try:
        f = _fields(lib, h)
        want = _up(sum(_up(per * esz, 16) for _, per, esz, _ in f.values()), 256)
        assert lib.ftl_env_bytes(h) == want
        assert want % 256 == 0
    finally:
        lib.ftl_destroy(h)


@pytest.mark.parametrize("name", ["B", "D", "E", "F"])
def test_record_stride_does_not_grow_with_the_stream_word(lib, name):
    h = _handle(lib, _cfg(name))
    try:
        f = _fields(lib, h)
        rec = [v for k, v in f.items() if v[0] < v[3] and v[3] % 128 == 0 and v[3] != v[1] * v[2]]
        stride = rec[0][3]
        used_before = 0
        for off, per, esz, _ in sorted(rec):
            per = per - 1 if off == f["env_int"][0] else per        # env_int as it was without FTL_EI_STREAM
            used_before = _up(used_before, 16) + per * esz
        assert _up(used_before, 128) == stride
        if name == "B":
            assert stride == 896
    finally:
        lib.ftl_destroy(h)


def test_layout_id(lib):
    def lid(cfg, n=4):
        h = _handle(lib, cfg, n)
        try:
            return lib.ftl_env_layout_id(h)
        finally:
            lib.ftl_destroy(h)
    b = _cfg("B")
    base = lid(b)
    shifted = _cfg("B")
    shifted.c.env_id_base = 2048
    assert lid(shifted) == base
    assert lid(_cfg("B"), n=97) == base
    assert lid(_cfg("B", traj_cap=b.c.traj_cap + 64)) != base            # a capacity
    assert lid(_cfg("B", corr_cap=2 * b.c.corr_cap)) != base
    assert lid(_cfg("D")) != base                                          # another sensor set


def test_argument_rejections_come_before_device_work(lib):
    """Every rejection returns before the library touches the device: the handle here never had one, and its bound "state" is an address
    nothing may dereference."""
    h = _handle(lib, _cfg("B"))
    try:
        ids = (C.c_int32 * 2)(0, 1)
        rows = C.c_void_p(1 << 20)
        assert lib.ftl_pack_envs(h, ids, 2, rows, None) == abi.FTL_E_STATE                    # unbound state
        assert lib.ftl_unpack_envs(h, rows, ids, 2, 0, None) == abi.FTL_E_STATE
        assert lib.ftl_pack_envs(h, ids, -1, rows, None) == abi.FTL_E_INVALID                 # argument checks come first
        assert lib.ftl_pack_envs(None, ids, 1, rows, None) == abi.FTL_E_INVALID
        assert lib.ftl_env_bytes(None) == 0 and lib.ftl_env_layout_id(None) == 0
        nbytes = lib.ftl_state_bytes(h)
        assert lib.ftl_bind_state(h, C.c_void_p(1 << 30), nbytes) == 0                       # host bookkeeping only
        for rc in (lib.ftl_pack_envs(h, ids, -1, rows, None), lib.ftl_unpack_envs(h, rows, ids, -1, 0, None),
                   lib.ftl_pack_envs(h, None, 2, rows, None), lib.ftl_pack_envs(h, ids, 2, None, None),
                   lib.ftl_unpack_envs(h, None, ids, 2, 0, None), lib.ftl_unpack_envs(h, rows, None, 2, 0, None),
                   lib.ftl_pack_envs(h, ids, 2, C.c_void_p((1 << 20) + 8), None),
                   lib.ftl_unpack_envs(h, C.c_void_p((1 << 20) + 4), ids, 2, 0, None),
                   lib.ftl_unpack_envs(h, rows, ids, 2, 4, None), lib.ftl_unpack_envs(h, rows, ids, 2, 0x80000000, None)):
            assert rc == abi.FTL_E_INVALID
        assert lib.ftl_pack_envs(h, None, 0, None, None) == 0                                 # k == 0: nothing to do
        assert lib.ftl_unpack_envs(h, None, None, 0, abi.FTL_ENV_SLOT_STATS | abi.FTL_ENV_OWN_STREAM, None) == 0
    finally:
        lib.ftl_destroy(h)
