"""C-ABI checks of the action search that need no GPU (include/ftl.h: ftl_unpack_envs_from, ftl_search, ftl_search_begin / _sample / _select,
ftl_search_uniform): exports, the ctypes mirrors and the draw against the header, every argument check that comes before any device work,
and the numpy twin's selection rule."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import search_numpy
from continiousenvironment_follower_leader_amd import _lib, abi, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftl_unpack_envs_from", "ftl_sizeof_search_params", "ftl_sizeof_search_buffers", "ftl_search_begin", "ftl_search_sample",
           "ftl_search_select", "ftl_search")
FAKE = 4096      # a non-null, aligned "device pointer" that is never dereferenced: the checks under test come first
N, K, T = 4, 3, 5
CTYPE = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double, "uint64_t": C.c_uint64}


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _create(lib, n, **kw):
    cfg = make_config(**dict(dict(bear_number=1), **kw))
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), n, 0, C.byref(h)) == 0, lib.ftl_last_error()
    return h


@pytest.fixture()
def handles(lib):
    hs = dict(real=_create(lib, N), search=_create(lib, N * K), short=_create(lib, N * K + 1), other=_create(lib, N * K, bear_number=2))
    yield hs
    for h in hs.values():
        lib.ftl_destroy(h)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ftl.h")).read(), flags=re.S)


def _params(**over):
    p = abi.SearchParams()
    p.K, p.T, p.hold, p.iters, p.gamma, p.spread, p.decay, p.seed, p.flags = K, T, 2, 2, 0.97, 1.0, 0.5, 7, 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


_KEEP = []


def _buffers(**over):
    out, ro = abi.Outputs(), abi.RolloutOutputs()
    for name, _ in abi.Outputs._fields_:
        setattr(out, name, None if name == "policy_obs" else FAKE)
    ro.ret, ro.steps, ro.status = FAKE, FAKE, FAKE
    for k in [k for k in over if k.startswith("out_")]:
        setattr(out, k[4:], over.pop(k))
    for k in [k for k in over if k.startswith("ro_")]:
        setattr(ro, k[3:], over.pop(k))
    b = abi.SearchBuffers()
    for name in ("rows", "row_ids", "env_ids", "nominal", "cand", "action", "best_k", "best_ret"):
        setattr(b, name, FAKE)
    b.out, b.ro = C.pointer(out), C.pointer(ro)
    for k, v in over.items():
        setattr(b, k, v)
    _KEEP.append((out, ro))
    return b


def _search(lib, real, search, p=None, b=None, call=1, warm=1, null_p=False, null_b=False):
    p, b = p or _params(), b or _buffers()
    return lib.ftl_search(real, search, None if null_p else C.byref(p), call, warm, None if null_b else C.byref(b), None)


# ---------------------------------------------------------------- exports and mirrors
def test_symbols_declared_exported_and_listed(lib):
    hdr = _header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s
    assert re.search(r"static\s+inline\s+double\s+ftl_search_uniform\s*\(", hdr)
    assert any(s.endswith("ftl_search.hpp") for s in _lib.SOURCES)


def _struct_fields(name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _header(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl.strip())
        if m:
            fields += [("ptr" if m.group(3) else m.group(2), nm.strip()) for nm in m.group(4).split(",")]
    return fields


def test_mirrors_match_the_header(lib):
    fields = _struct_fields("ftl_search_params")
    assert [f[1] for f in fields] == [f[0] for f in abi.SearchParams._fields_]
    for (ctype, name), cf in zip(fields, abi.SearchParams._fields_):
        assert cf[1] is CTYPE[ctype], name
    assert lib.ftl_sizeof_search_params() == C.sizeof(abi.SearchParams) == 56
    fields = _struct_fields("ftl_search_buffers")
    assert [f[1] for f in fields] == [f[0] for f in abi.SearchBuffers._fields_]
    assert all(ctype == "ptr" for ctype, _ in fields)
    assert lib.ftl_sizeof_search_buffers() == C.sizeof(abi.SearchBuffers) == 80
    hdr = _header()
    assert int(re.search(r"#define\s+FTL_SEARCH_OWN_STREAM\s+(\d+)u", hdr).group(1)) == abi.FTL_SEARCH_OWN_STREAM == 1
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no existing struct changed


# ---------------------------------------------------------------- the draw
CASES = [(seed, sid, call, it, k, block, j) for seed in (0, 7, 2 ** 64 - 1) for sid in (0, 63, 2 ** 31 - 1) for call in (0, 1, 2 ** 40)
         for it, k, block in ((0, 1, 0), (1, 1, 0), (0, 2, 0), (0, 1, 1), (127, 2 ** 19 - 1, 65535), (3, 69, 2)) for j in (0, 1)]


def test_header_draw_equals_the_twin(tmp_path):
    """include/ftl.h's own ftl_search_uniform, compiled for the host, printed as hexadecimal floats."""
    src = ['#include <stdio.h>', '#include "ftl.h"', "int main(void) {"]
    for c in CASES:
        src.append('    printf("%%a\\n", ftl_search_uniform(%dULL, %dULL, %dULL, %du, %du, %du, %du));' % c)
    src += ["    return 0;", "}"]
    (tmp_path / "draw.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "draw")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "draw.cpp"), "-o", exe])
    got = [float.fromhex(x) for x in subprocess.check_output([exe]).decode().split()]
    want = [abi.search_uniform(*c) for c in CASES]
    assert got == want
    assert len(set(want)) == len(want)                   # every field of the key reaches the draw
    assert all(0.0 <= u < 1.0 for u in want)


def test_draw_is_the_uniform_stream_in_a_key_range_of_its_own():
    for seed, sid, call, it, k, block, j in CASES:
        key = (1 << 43) | block | (j << 16) | (it << 17) | (k << 24)
        assert abi.search_uniform(seed, sid, call, it, k, block, j) == abi.uniform01(seed, sid, call, key)
        assert key >> 43 == 1      # bit 43 and nothing above: the frames / range / scenario draws (bits 40, 41 | 44.., 42) never set it
    u = np.array([abi.search_uniform(1, 5, 2, 0, k, b, j) for k in range(1, 65) for b in range(8) for j in range(2)])
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / len(u))


# ---------------------------------------------------------------- argument checks before any device work
def test_search_null_arguments(lib, handles):
    r, s = handles["real"], handles["search"]
    assert _search(lib, None, s) == abi.FTL_E_INVALID
    assert _search(lib, r, None) == abi.FTL_E_INVALID
    assert _search(lib, r, s, null_p=True) == abi.FTL_E_INVALID
    assert _search(lib, r, s, null_b=True) == abi.FTL_E_INVALID
    for name, _ in abi.SearchBuffers._fields_:
        assert _search(lib, r, s, b=_buffers(**{name: None})) == abi.FTL_E_INVALID, name
    for name in ("ret", "steps", "status"):
        assert _search(lib, r, s, b=_buffers(**{"ro_" + name: None})) == abi.FTL_E_INVALID, name
    for name in ("obs_num", "target", "reward", "done", "status"):      # (this config has no ray sensor: lasers may be NULL)
        assert _search(lib, r, s, b=_buffers(**{"out_" + name: None})) == abi.FTL_E_INVALID, name
    for name in ("rows", "nominal", "cand"):
        assert _search(lib, r, s, b=_buffers(**{name: FAKE + 8})) == abi.FTL_E_INVALID, name
        assert b"aligned" in lib.ftl_last_error()


@pytest.mark.parametrize("over", [dict(K=0), dict(T=0), dict(hold=0), dict(iters=0), dict(K=-1), dict(K=1 << 19), dict(iters=128),
                                  dict(T=65536, hold=1), dict(spread=0.0), dict(spread=1.5), dict(spread=float("nan")), dict(decay=0.0),
                                  dict(decay=1.0001), dict(gamma=float("inf")), dict(gamma=float("nan")), dict(flags=2)])
def test_search_parameter_ranges(lib, handles, over):
    assert _search(lib, handles["real"], handles["search"], p=_params(**over)) == abi.FTL_E_INVALID
    assert lib.ftl_search_sample(handles["real"], FAKE, N, C.byref(_params(**over)), 1, 0, 1.0, FAKE, FAKE, None) == abi.FTL_E_INVALID


def test_search_handles_must_fit(lib, handles):
    r, s = handles["real"], handles["search"]
    assert _search(lib, r, handles["short"]) == abi.FTL_E_INVALID
    assert b"n * K" in lib.ftl_last_error()
    assert _search(lib, r, s, p=_params(K=K + 1)) == abi.FTL_E_INVALID
    assert _search(lib, r, handles["other"]) == abi.FTL_E_INVALID
    assert b"layout" in lib.ftl_last_error()
    assert _search(lib, r, r, p=_params(K=1)) == abi.FTL_E_INVALID
    # every argument fine: only the state is missing (nothing was bound, no pool loaded)
    for kw in (dict(), dict(call=0), dict(warm=0), dict(p=_params(flags=abi.FTL_SEARCH_OWN_STREAM)), dict(p=_params(hold=T + 3))):
        assert _search(lib, r, s, **kw) == abi.FTL_E_STATE
        assert b"ftl_bind_state" in lib.ftl_last_error()


def test_piece_argument_checks(lib, handles):
    h = handles["real"]
    p = C.byref(_params())
    assert lib.ftl_search_begin(None, FAKE, N, T, 1, 1, FAKE, None) == abi.FTL_E_INVALID
    assert lib.ftl_search_begin(h, None, N, T, 1, 1, FAKE, None) == abi.FTL_E_INVALID
    assert lib.ftl_search_begin(h, FAKE, N, T, 1, 1, None, None) == abi.FTL_E_INVALID
    assert lib.ftl_search_begin(h, FAKE, 0, T, 1, 1, FAKE, None) == abi.FTL_E_INVALID
    assert lib.ftl_search_begin(h, FAKE, N, 0, 1, 1, FAKE, None) == abi.FTL_E_INVALID
    for args in ((None, FAKE, N, p, 1, 0, 1.0, FAKE, FAKE), (h, None, N, p, 1, 0, 1.0, FAKE, FAKE), (h, FAKE, N, None, 1, 0, 1.0, FAKE, FAKE),
                 (h, FAKE, N, p, 1, 0, 1.0, None, FAKE), (h, FAKE, N, p, 1, 0, 1.0, FAKE, None), (h, FAKE, 0, p, 1, 0, 1.0, FAKE, FAKE),
                 (h, FAKE, N, p, 1, -1, 1.0, FAKE, FAKE), (h, FAKE, N, p, 1, 128, 1.0, FAKE, FAKE), (h, FAKE, N, p, 1, 0, 1.5, FAKE, FAKE),
                 (h, FAKE, N, p, 1, 0, -0.5, FAKE, FAKE), (h, FAKE, N, p, 1, 0, float("nan"), FAKE, FAKE), (h, FAKE, N, p, 1, 0, 1.0, FAKE + 8, FAKE)):
        assert lib.ftl_search_sample(*args, None) == abi.FTL_E_INVALID, args
    for args in ((None, FAKE, N, K, T, FAKE, FAKE, FAKE, FAKE), (h, None, N, K, T, FAKE, FAKE, FAKE, FAKE), (h, FAKE, N, K, T, None, FAKE, FAKE, FAKE),
                 (h, FAKE, N, K, T, FAKE, None, FAKE, FAKE), (h, FAKE, N, K, T, FAKE, FAKE, None, FAKE), (h, FAKE, N, K, T, FAKE, FAKE, FAKE, None),
                 (h, FAKE, 0, K, T, FAKE, FAKE, FAKE, FAKE), (h, FAKE, N, 0, T, FAKE, FAKE, FAKE, FAKE), (h, FAKE, N, K, 0, FAKE, FAKE, FAKE, FAKE),
                 (h, FAKE, N, K, T, FAKE + 8, FAKE, FAKE, FAKE), (h, FAKE, 1 << 20, 1 << 18, T, FAKE, FAKE, FAKE, FAKE)):
        assert lib.ftl_search_select(*args, None) == abi.FTL_E_INVALID, args


def test_unpack_envs_from_checks_as_unpack_envs(lib, handles):
    h = handles["real"]
    assert lib.ftl_unpack_envs_from(None, FAKE, FAKE, FAKE, 2, 0, None) == abi.FTL_E_INVALID
    assert lib.ftl_unpack_envs_from(h, None, FAKE, FAKE, 2, 0, None) == abi.FTL_E_INVALID
    assert lib.ftl_unpack_envs_from(h, FAKE, FAKE, None, 2, 0, None) == abi.FTL_E_INVALID
    assert lib.ftl_unpack_envs_from(h, FAKE, FAKE, FAKE, -1, 0, None) == abi.FTL_E_INVALID
    assert lib.ftl_unpack_envs_from(h, FAKE + 4, FAKE, FAKE, 2, 0, None) == abi.FTL_E_INVALID
    assert lib.ftl_unpack_envs_from(h, FAKE, FAKE, FAKE, 2, 4, None) == abi.FTL_E_INVALID
    for row_ids in (FAKE, None):                                                # NULL row ids: ftl_unpack_envs itself
        assert lib.ftl_unpack_envs_from(h, FAKE, row_ids, FAKE, 2, abi.FTL_ENV_OWN_STREAM, None) == abi.FTL_E_STATE
        assert lib.ftl_unpack_envs_from(h, FAKE, row_ids, FAKE, 0, 0, None) == abi.FTL_E_STATE       # (state is checked before k == 0)


# ---------------------------------------------------------------- the python surface
def test_python_surface_needs_no_device():
    import inspect
    from continiousenvironment_follower_leader_amd.search import ActionSearch
    p = inspect.signature(ActionSearch.__init__).parameters
    assert list(p)[1:] == ["batch", "K", "T", "hold", "iters", "gamma", "spread", "decay", "seed", "warm", "own_stream"]
    assert [p[k].default for k in list(p)[4:]] == [1, 1, 1.0, 1.0, 0.5, 0, True, False]
    for name in ("act", "__call__", "radius", "close"):
        assert callable(getattr(ActionSearch, name))

    class FakeBatch:
        n, device = 4, "cpu"
    for kw in (dict(discrete_action_space=True, add_obstacles=False, path_finding_algorythm="astar"), dict(constant_follower_speed=True)):
        FakeBatch.cfg = make_config(**kw)
        with pytest.raises(ValueError, match="Box\\(2\\)"):
            ActionSearch(FakeBatch(), 4, 3)
    FakeBatch.cfg = make_config()
    FakeBatch.games = [object(), object()]
    with pytest.raises(ValueError, match="pipelined"):
        ActionSearch(FakeBatch(), 4, 3)
    FakeBatch.games = None
    for kw in (dict(K=0), dict(T=0), dict(hold=0), dict(iters=0), dict(iters=128), dict(K=1 << 19), dict(spread=0.0), dict(decay=2.0),
               dict(gamma=float("inf"))):
        with pytest.raises(ValueError):
            ActionSearch(FakeBatch(), **dict(dict(K=4, T=3), **kw))


# ---------------------------------------------------------------- the twin
def test_twin_select_takes_the_first_maximum():
    Kt, Tt = 5, 2
    ret = np.array([1.0, 3.0, 3.0, 2.0, 3.0,          # ties at several k: the lowest
                    4.0, 1.0, 4.0, 0.0, 0.0,          # the maximum at k = 0 and again later
                    0.0, 0.0, 0.0, 0.0, 9.0,          # at K - 1
                    -0.0, 0.0, -0.0, 0.0, -1.0,       # -0.0 equals 0.0: k = 0, and best_ret keeps its sign bit
                    0.0, -0.0, -5.0, -0.0, 0.0,
                    -2.0, -2.0, -2.0, -2.0, -2.0])    # all equal
    n = len(ret) // Kt
    cand = np.arange(Tt * n * Kt * 2, dtype=np.float64).reshape(Tt, n * Kt, 2)
    nominal = -np.ones((Tt, n, 2))
    bk, br, nom = search_numpy.select(ret, Kt, cand, nominal)
    assert bk.tolist() == [1, 0, 4, 0, 0, 0] and bk.dtype == np.int32
    assert br.tolist() == [3.0, 4.0, 9.0, 0.0, 0.0, -2.0]
    assert np.signbit(br).tolist() == [False, False, False, True, False, True]
    for e in range(n):
        assert np.array_equal(nom[:, e], cand[:, e * Kt + bk[e]])
    assert (nominal == -1).all()                      # the input is left alone


def test_twin_sample_and_begin():
    cfg = make_config(bear_number=1)
    lo, hi = search_numpy.box(cfg)
    assert lo[0] == cfg.c.follower.min_speed and hi[0] == cfg.c.follower.max_speed and lo[1] == -hi[1] < 0
    rng = np.random.default_rng(0)
    nominal = lo + rng.random((3, 2, 2)) * (hi - lo)
    cand = search_numpy.sample(nominal, [5, 2 ** 31 - 1], 9, 1, 0, 4, 2, 1.0, lo, hi)
    assert np.array_equal(cand[:, ::4], nominal)                               # k = 0 is the nominal
    assert (cand >= lo).all() and (cand <= hi).all()
    same = search_numpy.sample(np.broadcast_to(nominal[:1], nominal.shape), [5, 6], 9, 1, 0, 4, 2, 0.25, lo, hi)
    assert np.array_equal(same[0], same[1]) and not np.array_equal(same[0], same[2])      # steps 0 and 1 share a hold block, step 2 starts another
    u = abi.search_uniform(9, 5, 1, 0, 1, 0, 1)
    x = nominal[0, 0, 1] + (1.0 * (u - 0.5)) * (hi[1] - lo[1])
    assert cand[0, 1, 1] == min(max(x, lo[1]), hi[1])
    tiny = search_numpy.sample(nominal, [5, 6], 9, 1, 1, 4, 2, 2.0 ** -30, lo, hi)
    assert np.abs(tiny - nominal.repeat(4, 1)).max() < 1e-6
    shifted = search_numpy.begin([0, 7], nominal, 3, True, hi[0])
    assert np.array_equal(shifted[:, 0], np.array([[hi[0], 0.0]] * 3))
    assert np.array_equal(shifted[:2, 1], nominal[1:, 1]) and np.array_equal(shifted[2, 1], nominal[2, 1])
    for call, warm in ((0, True), (3, False)):
        assert np.array_equal(search_numpy.begin([0, 7], nominal, call, warm, hi[0]), np.broadcast_to([hi[0], 0.0], (3, 2, 2)))
