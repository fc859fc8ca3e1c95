"""C-ABI checks of the episode queue that need no GPU (include/ftl.h: ftl_episode_record, ftl_episode_queue, ftl_set_episode_queue,
ftl_queue_start, FTL_STEP_QUEUE_RESET): exports, the ctypes / numpy mirrors of the record against the header, the flag values, and the
argument checks that come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from continiousenvironment_follower_leader_amd import _lib, abi, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftl_sizeof_episode_record", "ftl_sizeof_episode_queue", "ftl_set_episode_queue", "ftl_queue_start")
CTYPE = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double, "int64_t": C.c_int64}
FAKE = 4096      # a non-null "device pointer" that is never dereferenced: the checks under test come first


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture()
def handle(lib):
    cfg = make_config(bear_number=1)
    cfg.c.env_id_base = 5
    h = C.c_void_p()
    assert lib.ftl_create(C.byref(cfg.c), 4, 0, C.byref(h)) == 0, lib.ftl_last_error()
    yield h
    lib.ftl_destroy(h)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ftl.h")).read(), flags=re.S)


def _struct_fields(name):
    """[(C type, field name, array length or 0)] of `typedef struct name { ... } name;` in the header."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _header(), re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        ctype, ptr = m.group(2), m.group(3)
        for nm in m.group(4).split(","):
            nm = nm.strip()
            a = re.match(r"(\w+)\[(\d+)\]$", nm)
            out.append(("ptr" if ptr else ctype, a.group(1) if a else nm, int(a.group(2)) if a else 0))
    return out


def _queue(**over):
    q = abi.EpisodeQueueC()
    q.scenario, q.stream, q.stream_base, q.n = FAKE, None, 0, 8
    q.head, q.records, q.ticket = FAKE, FAKE, FAKE
    for k, v in over.items():
        setattr(q, k, v)
    return q


def test_symbols_declared_exported_and_listed(lib):
    hdr = _header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s


def test_record_mirrors_match_the_header(lib):
    fields = _struct_fields("ftl_episode_record")
    assert [f[1] for f in fields] == [f[0] for f in abi.EpisodeRecord._fields_] == [d[0] for d in abi.RECORD_DTYPE]
    for (ctype, name, arr), cf in zip(fields, abi.EpisodeRecord._fields_):
        want = CTYPE[ctype] * arr if arr else CTYPE[ctype]
        assert C.sizeof(cf[1]) == C.sizeof(want) and (cf[1] is want or arr), name
    dt = np.dtype(abi.RECORD_DTYPE)
    assert lib.ftl_sizeof_episode_record() == C.sizeof(abi.EpisodeRecord) == dt.itemsize == 56
    for name, _ in [(f[0], f[1]) for f in abi.EpisodeRecord._fields_]:
        assert dt.fields[name][1] == getattr(abi.EpisodeRecord, name).offset, name
    assert dt["ret"] == np.float64 and dt["stream"] == np.int64 and dt["errors"] == np.uint32 and dt["status"].shape == (3,)


def test_queue_mirror_matches_the_header(lib):
    fields = _struct_fields("ftl_episode_queue")
    assert [f[1] for f in fields] == [f[0] for f in abi.EpisodeQueueC._fields_]
    for (ctype, name, _), cf in zip(fields, abi.EpisodeQueueC._fields_):
        assert cf[1] is (C.c_void_p if ctype == "ptr" else CTYPE[ctype]), name
    assert lib.ftl_sizeof_episode_queue() == C.sizeof(abi.EpisodeQueueC)


def test_flag_values_match_the_header():
    hdr = _header()
    for name, val in (("FTL_STEP_QUEUE_RESET", abi.FTL_STEP_QUEUE_RESET), ("FTL_EPISODE_DONE_AT_RESET", abi.FTL_EPISODE_DONE_AT_RESET),
                      ("FTL_ERR_BAD_STREAM", abi.FTL_ERR_BAD_STREAM)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, hdr).group(1)) == val
    assert abi.FTL_STEP_QUEUE_RESET == 8
    assert not abi.FTL_STEP_QUEUE_RESET & (abi.FTL_STEP_AUTO_RESET | abi.FTL_STEP_NEXT_RESET)


@pytest.mark.parametrize("other", [abi.FTL_STEP_AUTO_RESET, abi.FTL_STEP_NEXT_RESET])
def test_queue_flag_excludes_the_other_reset_flags(lib, handle, other):
    q = _queue()
    assert lib.ftl_set_episode_queue(handle, C.byref(q)) == 0, lib.ftl_last_error()
    out, fin, act = abi.Outputs(), abi.FinalOutputs(), C.c_void_p(FAKE)
    flags = abi.FTL_STEP_QUEUE_RESET | other
    assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), C.byref(fin), flags, None) == abi.FTL_E_INVALID
    assert b"FTL_STEP_QUEUE_RESET" in lib.ftl_last_error()
    assert lib.ftl_step_encoded(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), flags, None) == abi.FTL_E_INVALID
    assert lib.ftl_step(handle, act, C.byref(out), flags, None) == abi.FTL_E_INVALID


@pytest.mark.parametrize("field", ["scenario", "head", "records", "ticket"])
def test_null_pointer_inside_the_queue_is_rejected(lib, handle, field):
    q = _queue(**{field: None})
    assert lib.ftl_set_episode_queue(handle, C.byref(q)) == abi.FTL_E_INVALID
    assert field.encode() in lib.ftl_last_error()


@pytest.mark.parametrize("n", [0, -3])
def test_empty_queue_is_rejected(lib, handle, n):
    q = _queue(n=n)
    assert lib.ftl_set_episode_queue(handle, C.byref(q)) == abi.FTL_E_INVALID


@pytest.mark.parametrize("base, n, ok", [(0, 8, True), (2 ** 31 - 8, 8, True), (2 ** 31 - 7, 8, False), (-1, 8, False), (2 ** 40, 1, False)])
def test_stream_ids_outside_int32_are_rejected_at_attach(lib, handle, base, n, ok):
    q = _queue(stream_base=base, n=n)
    rc = lib.ftl_set_episode_queue(handle, C.byref(q))
    assert rc == (0 if ok else abi.FTL_E_INVALID), lib.ftl_last_error()
    # a stream array is the caller's: its ids are checked on the device (FTL_ERR_BAD_STREAM), so any base passes with one
    q = _queue(stream_base=base, n=n, stream=FAKE)
    assert lib.ftl_set_episode_queue(handle, C.byref(q)) == 0


def test_step_and_start_without_a_queue_are_rejected(lib, handle):
    out, act = abi.Outputs(), C.c_void_p(FAKE)
    assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), None, abi.FTL_STEP_QUEUE_RESET, None) == abi.FTL_E_STATE
    assert b"queue" in lib.ftl_last_error()
    assert lib.ftl_queue_start(handle, C.byref(out), None) == abi.FTL_E_STATE
    q = _queue()
    assert lib.ftl_set_episode_queue(handle, C.byref(q)) == 0
    assert lib.ftl_set_episode_queue(handle, None) == 0          # detached again
    assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), None, abi.FTL_STEP_QUEUE_RESET, None) == abi.FTL_E_STATE
    assert b"queue" in lib.ftl_last_error()
    assert lib.ftl_queue_start(handle, C.byref(out), None) == abi.FTL_E_STATE
    assert lib.ftl_set_episode_queue(None, C.byref(q)) == abi.FTL_E_INVALID


def test_python_mode_and_refusals_need_no_device():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    g = VecGame.__new__(VecGame)
    g._fin, g.queue = None, None
    with pytest.raises(_lib.FtlError):
        g._step_mode("queue")                 # no queue attached
    g.queue = object()
    assert g._step_mode("queue") == (abi.FTL_STEP_QUEUE_RESET, None)
    for cls in (VecGame, PipelinedVecGame):   # a batch with a queue attached is not saved
        b = cls.__new__(cls)
        b.queue = object()
        for method in (b.snapshot, b.state_dict):
            with pytest.raises(_lib.FtlError, match="episode queue"):
                method()
