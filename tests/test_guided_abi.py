"""C-ABI checks of the guided search that need no GPU (include/ftl.h: ftl_baseline_act_guided, ftl_rollout_guided, ftl_guided_fanout,
ftl_search_guided): exports, the ctypes mirror of ftl_guided_buffers against the header compiled for the host (size and every offset), every
argument check that comes before any device work, the numpy twin's clip-add-clip on edge inputs, and the wrapper's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guided_numpy
from continiousenvironment_follower_leader_amd import _lib, abi, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftl_sizeof_guided_buffers", "ftl_baseline_act_guided", "ftl_rollout_guided", "ftl_guided_fanout", "ftl_search_guided")
FAKE, FAKE2 = 4096, 8192      # non-null, aligned "device pointers" that are never dereferenced: the checks under test come first
N, K, T, CAP = 4, 3, 5, 8
ROW = 16 + 16 * CAP
RESETS = (abi.FTL_STEP_AUTO_RESET, abi.FTL_STEP_NEXT_RESET, abi.FTL_STEP_QUEUE_RESET, abi.FTL_STEP_SAMPLE_RESET)


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


_KEEP = []


def _outputs(ptr=FAKE, **over):
    o = abi.Outputs()
    for name, _ in abi.Outputs._fields_:
        setattr(o, name, None if name == "policy_obs" else ptr)
    for k, v in over.items():
        setattr(o, k, v)
    _KEEP.append(o)
    return o


def _ro(**over):
    ro = abi.RolloutOutputs()
    ro.ret, ro.steps, ro.status = FAKE, FAKE, FAKE
    for k, v in over.items():
        setattr(ro, k, v)
    _KEEP.append(ro)
    return ro


def _params(**over):
    p = abi.SearchParams()
    p.K, p.T, p.hold, p.iters, p.gamma, p.spread, p.decay, p.seed, p.flags = K, T, 2, 2, 0.97, 1.0, 0.5, 7, 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _buffers(**over):
    out = _outputs(FAKE, **{k[4:]: over.pop(k) for k in [k for k in over if k.startswith("out_")]})
    real_out = _outputs(FAKE2, **{k[5:]: over.pop(k) for k in [k for k in over if k.startswith("real_") and hasattr(abi.Outputs, k[5:])]})
    ro = _ro(**{k[3:]: over.pop(k) for k in [k for k in over if k.startswith("ro_")]})
    b = abi.GuidedBuffers()
    for name in ("rows", "row_ids", "env_ids", "nominal", "cand", "action", "best_k", "best_ret", "real_bl"):
        setattr(b, name, FAKE)
    b.search_bl = FAKE2
    b.out, b.ro, b.real_out = C.pointer(out), C.pointer(ro), C.pointer(real_out)
    b.real_bl_bytes, b.search_bl_bytes, b.cap = N * ROW, N * K * ROW, CAP
    for k, v in over.items():
        setattr(b, k, v)
    return b


def _guided(lib, real, search, p=None, b=None, call=1, warm=1, tail=2, null_p=False, null_b=False):
    p, b = p or _params(), b or _buffers()
    return lib.ftl_search_guided(real, search, None if null_p else C.byref(p), call, warm, tail, None if null_b else C.byref(b), None)


# ---------------------------------------------------------------- exports and the mirror
def test_symbols_declared_exported_and_listed(lib):
    hdr = _header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s
    assert any(s.endswith("ftl_guided.hpp") for s in _lib.SOURCES)
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # no existing struct changed


def test_mirror_matches_the_header(lib, tmp_path):
    """include/ftl.h's own ftl_guided_buffers, compiled for the host: its size and the offset of every field, by name."""
    names = [f[0] for f in abi.GuidedBuffers._fields_]
    body = re.search(r"typedef\s+struct\s+ftl_guided_buffers\s*\{(.*?)\}\s*ftl_guided_buffers\s*;", _header(), re.S).group(1)
    declared = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert declared == names                                                # same fields, same order
    assert names[:10] == [f[0] for f in abi.SearchBuffers._fields_]         # "the fields of ftl_search_buffers plus ..."
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ftl.h"', "int main(void) {",
           '    printf("%zu\\n", sizeof(ftl_guided_buffers));']
    src += ['    printf("%%zu\\n", offsetof(ftl_guided_buffers, %s));' % n for n in names]
    src += ['    printf("%zu\\n", sizeof(ftl_search_buffers));', "    return 0;", "}"]
    (tmp_path / "off.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "off")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "off.cpp"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(abi.GuidedBuffers) == lib.ftl_sizeof_guided_buffers() == 128
    assert got[1:-1] == [getattr(abi.GuidedBuffers, n).offset for n in names]
    assert got[-1] == C.sizeof(abi.SearchBuffers) == lib.ftl_sizeof_search_buffers() == 80                # the existing struct is as it was
    for n in names[:10]:
        assert getattr(abi.GuidedBuffers, n).offset == getattr(abi.SearchBuffers, n).offset


# ---------------------------------------------------------------- ftl_baseline_act_guided
def _act(lib, h, out, bl=FAKE, bl_bytes=N * ROW, cap=CAP, resid=FAKE, action=FAKE):
    return lib.ftl_baseline_act_guided(h, C.byref(out) if out is not None else None, bl, bl_bytes, cap, resid, action, None)


def test_act_guided_argument_checks(lib, handles):
    h, out = handles["real"], _outputs()
    assert _act(lib, None, out) == abi.FTL_E_INVALID
    assert _act(lib, h, None) == abi.FTL_E_INVALID
    assert _act(lib, h, out, bl=None) == abi.FTL_E_INVALID
    assert _act(lib, h, out, resid=None) == abi.FTL_E_INVALID
    assert _act(lib, h, out, action=None) == abi.FTL_E_INVALID
    for cap in (1, 0, -3):
        assert _act(lib, h, out, cap=cap) == abi.FTL_E_INVALID
        assert b"cap" in lib.ftl_last_error()
    assert _act(lib, h, out, bl_bytes=N * ROW - 1) == abi.FTL_E_INVALID
    assert b"ftl_baseline_bytes" in lib.ftl_last_error()
    assert _act(lib, h, out, bl=FAKE + 4) == abi.FTL_E_INVALID
    assert b"aligned" in lib.ftl_last_error()
    assert _act(lib, h, out, resid=FAKE + 4) == abi.FTL_E_INVALID
    assert b"aligned" in lib.ftl_last_error()
    for name in ("obs_num", "target"):
        assert _act(lib, h, _outputs(**{name: None})) in (abi.FTL_E_INVALID, abi.FTL_E_STATE)      # (the state is checked first, as in ftl_baseline_act)
    assert _act(lib, h, out) == abi.FTL_E_STATE                                # every argument fine: only the state is missing
    assert b"ftl_bind_state" in lib.ftl_last_error()


# ---------------------------------------------------------------- ftl_rollout_guided
def _rollout(lib, h, out, ro, T=3, tail=2, bl=FAKE, bl_bytes=N * ROW, cap=CAP, resid=FAKE, resid_step=N * 16, actions=None, step_bytes=0, flags=0):
    return lib.ftl_rollout_guided(h, T, tail, 1.0, C.byref(out) if out is not None else None, C.byref(ro) if ro is not None else None, bl, bl_bytes,
                                  cap, resid, resid_step, actions, step_bytes, flags, None)


def test_rollout_guided_argument_checks(lib, handles):
    h, out = handles["real"], _outputs()
    assert _rollout(lib, None, out, _ro()) == abi.FTL_E_INVALID
    assert _rollout(lib, h, None, _ro()) == abi.FTL_E_INVALID
    assert _rollout(lib, h, out, None) == abi.FTL_E_INVALID
    assert _rollout(lib, h, out, _ro(), bl=None) == abi.FTL_E_INVALID
    for field in ("ret", "steps", "status"):
        assert _rollout(lib, h, out, _ro(**{field: None})) == abi.FTL_E_INVALID
        assert field.encode() in lib.ftl_last_error()
    for T_ in (0, -2):
        assert _rollout(lib, h, out, _ro(), T=T_) == abi.FTL_E_INVALID
        assert b"T must be positive" in lib.ftl_last_error()
    for tail in (-1, -100, 2 ** 31 - 3):
        assert _rollout(lib, h, out, _ro(), tail=tail) == abi.FTL_E_INVALID
        assert b"tail" in lib.ftl_last_error()
    for r in RESETS:
        for flags in (r, r | abi.FTL_STEP_NO_SENSORS):
            assert _rollout(lib, h, out, _ro(), flags=flags) == abi.FTL_E_INVALID
            assert b"FTL_STEP_NO_SENSORS" in lib.ftl_last_error()
    for cap in (1, 0):
        assert _rollout(lib, h, out, _ro(), cap=cap) == abi.FTL_E_INVALID
    assert _rollout(lib, h, out, _ro(), bl_bytes=N * ROW - 1) == abi.FTL_E_INVALID
    assert _rollout(lib, h, out, _ro(), bl=FAKE + 4) == abi.FTL_E_INVALID
    assert _rollout(lib, h, out, _ro(), actions=FAKE, step_bytes=N * 16 - 1) == abi.FTL_E_INVALID
    assert b"step_bytes" in lib.ftl_last_error()
    assert _rollout(lib, h, out, _ro(), resid_step=N * 16 - 8) == abi.FTL_E_INVALID
    assert b"resid_step_bytes" in lib.ftl_last_error()
    assert _rollout(lib, h, out, _ro(), resid=FAKE + 4) == abi.FTL_E_INVALID
    assert _rollout(lib, h, out, _ro(), resid_step=N * 16 + 4) == abi.FTL_E_INVALID
    assert b"aligned" in lib.ftl_last_error()
    for kw in (dict(), dict(tail=0), dict(flags=abi.FTL_STEP_NO_SENSORS), dict(actions=FAKE, step_bytes=N * 16), dict(resid=None, resid_step=0),
               dict(resid_step=10 * N * 16), dict(T=1, tail=0)):
        assert _rollout(lib, h, out, _ro(), **kw) == abi.FTL_E_STATE                               # only the state is missing
        assert b"ftl_bind_state" in lib.ftl_last_error()


# ---------------------------------------------------------------- ftl_guided_fanout
def _fanout(lib, real, search, k=K, real_out="x", search_out="x", real_bl=FAKE, real_bytes=N * ROW, search_bl=FAKE2, search_bytes=N * K * ROW, cap=CAP):
    ro = _outputs(FAKE) if real_out == "x" else real_out
    so = _outputs(FAKE2) if search_out == "x" else search_out
    return lib.ftl_guided_fanout(real, search, k, C.byref(ro) if ro is not None else None, C.byref(so) if so is not None else None,
                                 real_bl, real_bytes, search_bl, search_bytes, cap, None)


def test_fanout_argument_checks(lib, handles):
    r, s = handles["real"], handles["search"]
    assert _fanout(lib, None, s) == abi.FTL_E_INVALID
    assert _fanout(lib, r, None) == abi.FTL_E_INVALID
    assert _fanout(lib, r, s, real_out=None) == abi.FTL_E_INVALID
    assert _fanout(lib, r, s, search_out=None) == abi.FTL_E_INVALID
    assert _fanout(lib, r, s, real_bl=None) == abi.FTL_E_INVALID
    assert _fanout(lib, r, s, search_bl=None) == abi.FTL_E_INVALID
    for name in ("obs_num", "target"):
        assert _fanout(lib, r, s, real_out=_outputs(FAKE, **{name: None})) == abi.FTL_E_INVALID
        assert _fanout(lib, r, s, search_out=_outputs(FAKE2, **{name: None})) == abi.FTL_E_INVALID
    for cap in (1, 0, -2):
        assert _fanout(lib, r, s, cap=cap) == abi.FTL_E_INVALID
        assert b"cap" in lib.ftl_last_error()
    for k in (0, -1, K + 1, K - 1):
        assert _fanout(lib, r, s, k=k) == abi.FTL_E_INVALID
    assert _fanout(lib, r, handles["short"]) == abi.FTL_E_INVALID
    assert b"n * K" in lib.ftl_last_error()
    assert _fanout(lib, r, s, real_bytes=N * ROW - 1) == abi.FTL_E_INVALID
    assert b"ftl_baseline_bytes" in lib.ftl_last_error()
    assert _fanout(lib, r, s, search_bytes=N * K * ROW - 1) == abi.FTL_E_INVALID
    assert b"ftl_baseline_bytes" in lib.ftl_last_error()
    for kw in (dict(real_bl=FAKE + 8), dict(search_bl=FAKE2 + 8), dict(search_bl=FAKE2 + 4)):
        assert _fanout(lib, r, s, **kw) == abi.FTL_E_INVALID
        assert b"16-byte aligned" in lib.ftl_last_error()
    assert _fanout(lib, r, s, search_bl=FAKE) == abi.FTL_E_INVALID                                 # onto its own source
    assert _fanout(lib, r, s, search_out=_outputs(FAKE)) == abi.FTL_E_INVALID
    assert b"distinct" in lib.ftl_last_error()


# ---------------------------------------------------------------- ftl_search_guided
def test_search_guided_null_arguments(lib, handles):
    r, s = handles["real"], handles["search"]
    assert _guided(lib, None, s) == abi.FTL_E_INVALID
    assert _guided(lib, r, None) == abi.FTL_E_INVALID
    assert _guided(lib, r, s, null_p=True) == abi.FTL_E_INVALID
    assert _guided(lib, r, s, null_b=True) == abi.FTL_E_INVALID
    for name, ctype in abi.GuidedBuffers._fields_:
        if name in ("real_bl_bytes", "search_bl_bytes", "cap", "_pad"):
            continue
        assert _guided(lib, r, s, b=_buffers(**{name: None})) == abi.FTL_E_INVALID, name
    for name in ("ret", "steps", "status"):
        assert _guided(lib, r, s, b=_buffers(**{"ro_" + name: None})) == abi.FTL_E_INVALID, name
    for name in ("obs_num", "target", "reward", "done", "status"):      # (this config has no ray sensor: lasers may be NULL)
        assert _guided(lib, r, s, b=_buffers(**{"out_" + name: None})) == abi.FTL_E_INVALID, name
        assert _guided(lib, r, s, b=_buffers(**{"real_" + name: None})) == abi.FTL_E_INVALID, name
    for name in ("rows", "nominal", "cand", "real_bl", "search_bl"):
        assert _guided(lib, r, s, b=_buffers(**{name: FAKE + 8})) == abi.FTL_E_INVALID, name
        assert b"aligned" in lib.ftl_last_error()


@pytest.mark.parametrize("over", [dict(K=0), dict(T=0), dict(hold=0), dict(iters=0), dict(K=-1), dict(K=1 << 19), dict(iters=128),
                                  dict(T=65536, hold=1), dict(spread=0.0), dict(spread=1.5), dict(spread=float("nan")), dict(decay=0.0),
                                  dict(decay=1.0001), dict(gamma=float("inf")), dict(gamma=float("nan")), dict(flags=2)])
def test_search_guided_parameter_ranges(lib, handles, over):
    assert _guided(lib, handles["real"], handles["search"], p=_params(**over)) == abi.FTL_E_INVALID


def test_search_guided_tail_cap_and_follower_buffers(lib, handles):
    r, s = handles["real"], handles["search"]
    for tail in (-1, -7, 2 ** 31 - 1 - T + 1):
        assert _guided(lib, r, s, tail=tail) == abi.FTL_E_INVALID
        assert b"tail" in lib.ftl_last_error()
    for cap in (1, 0, -4):
        assert _guided(lib, r, s, b=_buffers(cap=cap)) == abi.FTL_E_INVALID
        assert b"cap" in lib.ftl_last_error()
    assert _guided(lib, r, s, b=_buffers(real_bl_bytes=N * ROW - 1)) == abi.FTL_E_INVALID
    assert b"ftl_baseline_bytes" in lib.ftl_last_error()
    assert _guided(lib, r, s, b=_buffers(search_bl_bytes=N * K * ROW - 1)) == abi.FTL_E_INVALID
    assert b"ftl_baseline_bytes" in lib.ftl_last_error()
    assert _guided(lib, r, s, b=_buffers(cap=CAP + 1)) == abi.FTL_E_INVALID                        # the same bytes are short for a longer row


def test_search_guided_handles_must_fit(lib, handles):
    r, s = handles["real"], handles["search"]
    assert _guided(lib, r, handles["short"]) == abi.FTL_E_INVALID
    assert b"n * K" in lib.ftl_last_error()
    assert _guided(lib, r, s, p=_params(K=K + 1)) == abi.FTL_E_INVALID
    assert _guided(lib, r, handles["other"]) == abi.FTL_E_INVALID
    assert b"layout" in lib.ftl_last_error()
    assert _guided(lib, r, r, p=_params(K=1)) == abi.FTL_E_INVALID
    # every argument fine: only the state is missing (nothing was bound, no pool loaded)
    for kw in (dict(), dict(call=0), dict(warm=0), dict(tail=0), dict(tail=1000), dict(p=_params(flags=abi.FTL_SEARCH_OWN_STREAM)),
               dict(p=_params(hold=T + 3)), dict(b=_buffers(real_bl_bytes=10 * N * ROW, search_bl_bytes=10 * N * K * ROW))):
        assert _guided(lib, r, s, **kw) == abi.FTL_E_STATE
        assert b"ftl_bind_state" in lib.ftl_last_error()


# ---------------------------------------------------------------- the twin
def test_twin_guided_action_on_edge_inputs():
    cfg = make_config(bear_number=1)
    lo, hi = guided_numpy.box(cfg)
    rlo, rhi = guided_numpy.residual_box(cfg)
    assert np.array_equal(rhi - rlo, hi - lo) and np.array_equal(rlo, -rhi)            # the residual box has the action Box's width, exactly
    g = lambda base, r: guided_numpy.guided_action(np.array(base, dtype=np.float64), np.array(r, dtype=np.float64), lo, hi)
    mid = (lo + hi) / 2.0
    # the base above the Box (the usual case: v in px, the turn in tenths of degrees) and below it: clipped first, so the residual acts
    assert np.array_equal(g([250.0, 17.5], [0.0, 0.0]), hi)
    assert np.array_equal(g([-3.0, -17.5], [0.0, 0.0]), lo)
    assert np.array_equal(g([250.0, 17.5], rlo), hi + rlo) and (hi + rlo < hi).all()   # a residual added before the clip would have done nothing
    assert np.array_equal(g([-3.0, -17.5], rhi), lo + rhi) and (lo + rhi > lo).all()
    assert np.array_equal(g([250.0, 17.5], rhi), hi) and np.array_equal(g([-3.0, -17.5], rlo), lo)          # and the second clip holds the Box
    # residual 0 and -0.0: the clipped baseline action, bit for bit -- -0.0 included, since x + (-0.0) == x and x + 0.0 == x for x != 0
    for z in (0.0, -0.0):
        for base in ([250.0, 17.5], [-3.0, -17.5], list(mid), [lo[0], hi[1]], [0.3, -0.0], [0.3, 0.0]):
            want = np.fmin(np.fmax(np.array(base), lo), hi)
            got = g(base, [z, z])
            assert np.array_equal(got, want), (z, base)
            nz = want != 0
            assert np.array_equal(np.signbit(got)[nz], np.signbit(want)[nz])
    assert not np.signbit(g([0.3, -0.0], [0.0, 0.0]))[1] and np.signbit(g([0.3, -0.0], [0.0, -0.0]))[1]    # (-0.0) + 0.0 = 0.0; (-0.0) + (-0.0) = -0.0
    # the residual at either end of its box from the middle of the Box reaches the Box's ends exactly
    assert np.array_equal(g(mid, rhi), np.fmin(mid + rhi, hi)) and np.array_equal(g(mid, rlo), np.fmax(mid + rlo, lo))
    assert (g(mid, rhi) <= hi).all() and (g(mid, rlo) >= lo).all()
    # one rounding per operation, in this order
    base, r = np.array([0.1, 0.7]), np.array([1e-17, -1e-17])
    c = np.minimum(np.maximum(base, lo), hi)
    assert np.array_equal(g(base, r), np.minimum(np.maximum(c + r, lo), hi))
    # the follower twin takes the residual after its own bookkeeping
    import baseline_numpy
    f1, f2 = baseline_numpy.Follower(4), baseline_numpy.Follower(4)
    num = np.zeros(10, dtype=np.float32); num[5], num[6], num[8] = 100.0, 50.0, 30.0
    a = guided_numpy.act(f1, num, (160.0, 90.0), 0, np.array([-0.1, 0.2]), lo, hi)
    v, w = f2.act(num, (160.0, 90.0), 0)
    assert np.array_equal(a, g([v, w], [-0.1, 0.2])) and f1.fifo == f2.fifo and f1.pending == f2.pending


def test_twin_begin_and_sample_are_the_action_search_twins_on_the_residual_box():
    import search_numpy
    cfg = make_config(bear_number=1)
    rlo, rhi = guided_numpy.residual_box(cfg)
    nominal = rlo + np.random.default_rng(0).random((3, 2, 2)) * (rhi - rlo)
    start = guided_numpy.begin([0, 7], nominal, 3, True)
    assert np.array_equal(start[:, 0], np.zeros((3, 2))) and np.array_equal(start[:2, 1], nominal[1:, 1])
    assert np.array_equal(guided_numpy.begin([5, 7], nominal, 0, True), np.zeros((3, 2, 2)))
    cand = guided_numpy.sample(nominal, [5, 9], 9, 1, 0, 4, 2, 1.0, cfg)
    assert np.array_equal(cand[:, ::4], nominal) and (cand >= rlo).all() and (cand <= rhi).all()
    lo, hi = search_numpy.box(cfg)
    shifted = search_numpy.sample(nominal + (lo + hi) / 2.0, [5, 9], 9, 1, 0, 4, 2, 1.0, lo, hi)   # the same draws as on the action Box
    assert np.abs(shifted - (lo + hi) / 2.0 - cand).max() < 1e-12


# ---------------------------------------------------------------- the python surface
def test_python_surface_needs_no_device():
    import inspect
    from continiousenvironment_follower_leader_amd.search import ActionSearch, GuidedSearch
    from continiousenvironment_follower_leader_amd.vec_game import VecGame
    p = inspect.signature(GuidedSearch.__init__).parameters
    assert list(p)[1:] == ["batch", "K", "T", "tail", "hold", "iters", "gamma", "spread", "decay", "seed", "warm", "own_stream", "cap"]
    assert [p[k].default for k in list(p)[5:]] == [1, 1, 1.0, 1.0, 0.5, 0, True, False, 64]
    for name in ("act", "__call__", "radius", "close", "flags", "front", "_follow_pool"):
        assert callable(getattr(GuidedSearch, name))
    assert GuidedSearch._follow_pool is ActionSearch._follow_pool                       # shared, not copied
    p = inspect.signature(VecGame.rollout_guided).parameters
    assert list(p)[1:] == ["follower", "resid", "tail", "gamma", "sensors", "record"]
    assert [p[k].default for k in list(p)[3:]] == [0, 1.0, True, False]

    class FakeBatch:
        n, device = 4, "cpu"
    for kw in (dict(discrete_action_space=True, add_obstacles=False, path_finding_algorythm="astar"), dict(constant_follower_speed=True)):
        FakeBatch.cfg = make_config(**kw)
        with pytest.raises(ValueError, match="Box\\(2\\)"):
            GuidedSearch(FakeBatch(), 4, 3, 2)
    FakeBatch.cfg = make_config()
    FakeBatch.games = [object(), object()]
    with pytest.raises(ValueError, match="pipelined"):
        GuidedSearch(FakeBatch(), 4, 3, 2)
    FakeBatch.games = None
    for kw in (dict(K=0), dict(T=0), dict(hold=0), dict(iters=0), dict(iters=128), dict(K=1 << 19), dict(spread=0.0), dict(decay=2.0),
               dict(gamma=float("inf"))):
        with pytest.raises(ValueError):
            GuidedSearch(FakeBatch(), **dict(dict(K=4, T=3, tail=2), **kw))
    with pytest.raises(ValueError, match="tail"):
        GuidedSearch(FakeBatch(), 4, 3, -1)
    with pytest.raises(ValueError, match="cap"):
        GuidedSearch(FakeBatch(), 4, 3, 2, cap=1)
