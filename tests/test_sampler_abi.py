"""C-ABI checks of the scenario sampler that need no GPU (include/ftl.h: ftl_scenario_sampler, ftl_set_scenario_sampler,
ftl_sampler_refresh, ftl_sampler_start, FTL_STEP_SAMPLE_RESET, ftl_sample_scenario): exports, the ctypes mirror and the constants against
the header, the argument checks that come before any device work, the draw's Python twin against a restatement of the header's text (and
against the header's own C function), its frequencies, and the weight quantisation of ``ScenarioSampler``."""
import bisect
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from continiousenvironment_follower_leader_amd import _lib, abi, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftl_sizeof_scenario_sampler", "ftl_set_scenario_sampler", "ftl_sampler_refresh", "ftl_sampler_start")
CTYPE = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
FAKE = 4096      # a non-null, 8-byte aligned "device pointer" that is never dereferenced: the checks under test come first
M64 = (1 << 64) - 1
U32 = 2 ** 32 - 1
WEIGHTS = (list(range(1, 98)), [0, 5, 0, 0, 1, 0, 3] + [0] * 50 + [7], [U32] * 5 + [1, 0, U32], [0, 0, 9, 0])


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


def _sampler(**over):
    s = abi.ScenarioSamplerC()
    s.weight, s.cdf, s.base, s.count, s.table = FAKE, FAKE, 0, 8, FAKE
    for k, v in over.items():
        setattr(s, k, v)
    return s


# ---------------------------------------------------------------- exports and mirrors
def test_symbols_declared_exported_and_listed(lib):
    hdr = _header()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s
    assert re.search(r"static\s+inline\s+int32_t\s+ftl_sample_scenario\s*\(", hdr)


def test_sampler_mirror_matches_the_header(lib):
    body = re.search(r"typedef\s+struct\s+ftl_scenario_sampler\s*\{(.*?)\}\s*ftl_scenario_sampler\s*;", _header(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl.strip())
        if m:
            fields += [("ptr" if m.group(3) else m.group(2), nm.strip()) for nm in m.group(4).split(",")]
    assert [f[1] for f in fields] == [f[0] for f in abi.ScenarioSamplerC._fields_] == ["weight", "cdf", "base", "count", "table"]
    for (ctype, name), cf in zip(fields, abi.ScenarioSamplerC._fields_):
        assert cf[1] is (C.c_void_p if ctype == "ptr" else CTYPE[ctype]), name
    assert lib.ftl_sizeof_scenario_sampler() == C.sizeof(abi.ScenarioSamplerC) == 32


def test_flag_and_columns_match_the_header():
    hdr = _header()
    assert int(re.search(r"#define\s+FTL_STEP_SAMPLE_RESET\s+(\d+)u", hdr).group(1)) == abi.FTL_STEP_SAMPLE_RESET == 16
    assert not abi.FTL_STEP_SAMPLE_RESET & (abi.FTL_STEP_AUTO_RESET | abi.FTL_STEP_NEXT_RESET | abi.FTL_STEP_QUEUE_RESET)
    assert int(re.search(r"#define\s+FTL_N_SCEN_STATS\s+(\d+)", hdr).group(1)) == abi.FTL_N_SCEN_STATS == len(abi.SS_NAMES)
    cols = re.search(r"enum\s*\{\s*(FTL_SS_EPISODES.*?)\}", hdr, re.S).group(1)
    names = [c.split("=")[0].strip() for c in cols.split(",")]
    assert names == ["FTL_SS_" + n.upper() for n in abi.SS_NAMES]
    for k, n in enumerate(abi.SS_NAMES):
        assert getattr(abi, "SS_" + n.upper()) == k


# ---------------------------------------------------------------- argument checks before any device work
@pytest.mark.parametrize("field", ["weight", "cdf", "table"])
def test_null_pointer_inside_the_sampler_is_rejected(lib, handle, field):
    assert lib.ftl_set_scenario_sampler(handle, C.byref(_sampler(**{field: None}))) == abi.FTL_E_INVALID
    assert field.encode() in lib.ftl_last_error()


@pytest.mark.parametrize("over", [dict(count=0), dict(count=-3), dict(base=-1), dict(cdf=FAKE + 4), dict(table=FAKE + 2)])
def test_bad_window_or_alignment_is_rejected(lib, handle, over):
    assert lib.ftl_set_scenario_sampler(handle, C.byref(_sampler(**over))) == abi.FTL_E_INVALID
    assert lib.ftl_set_scenario_sampler(None, C.byref(_sampler())) == abi.FTL_E_INVALID
    # nothing was attached
    out, act = abi.Outputs(), C.c_void_p(FAKE)
    assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), None, abi.FTL_STEP_SAMPLE_RESET, None) == abi.FTL_E_STATE


def test_a_weight_array_needs_no_alignment_beyond_its_type(lib, handle):
    assert lib.ftl_set_scenario_sampler(handle, C.byref(_sampler(weight=FAKE + 4))) == 0, lib.ftl_last_error()


@pytest.mark.parametrize("other", [abi.FTL_STEP_AUTO_RESET, abi.FTL_STEP_NEXT_RESET, abi.FTL_STEP_QUEUE_RESET])
def test_sample_flag_excludes_the_other_reset_flags(lib, handle, other):
    assert lib.ftl_set_scenario_sampler(handle, C.byref(_sampler())) == 0, lib.ftl_last_error()
    out, fin, act = abi.Outputs(), abi.FinalOutputs(), C.c_void_p(FAKE)
    flags = abi.FTL_STEP_SAMPLE_RESET | other
    assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), C.byref(fin), flags, None) == abi.FTL_E_INVALID
    assert b"excludes the other reset flags" in lib.ftl_last_error()
    assert lib.ftl_step_encoded(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), flags, None) == abi.FTL_E_INVALID
    assert lib.ftl_step(handle, act, C.byref(out), flags, None) == abi.FTL_E_INVALID
    assert lib.ftl_step(handle, act, C.byref(out), flags | abi.FTL_STEP_AUTO_RESET | abi.FTL_STEP_NEXT_RESET, None) == abi.FTL_E_INVALID


def test_step_start_and_refresh_without_a_sampler_are_rejected(lib, handle):
    out, act = abi.Outputs(), C.c_void_p(FAKE)

    def all_refused():
        assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), None, abi.FTL_STEP_SAMPLE_RESET, None) == abi.FTL_E_STATE
        assert b"sampler" in lib.ftl_last_error()
        assert lib.ftl_step(handle, act, C.byref(out), abi.FTL_STEP_SAMPLE_RESET, None) == abi.FTL_E_STATE
        assert lib.ftl_sampler_start(handle, C.byref(out), None) == abi.FTL_E_STATE
        assert lib.ftl_sampler_refresh(handle, None) == abi.FTL_E_STATE
    all_refused()
    assert lib.ftl_set_scenario_sampler(handle, C.byref(_sampler())) == 0
    assert lib.ftl_set_scenario_sampler(handle, None) == 0          # detached again
    all_refused()
    assert lib.ftl_set_scenario_sampler(handle, None) == 0          # (detaching twice is fine)
    assert lib.ftl_sampler_start(None, C.byref(out), None) == abi.FTL_E_INVALID
    assert lib.ftl_sampler_refresh(None, None) == abi.FTL_E_INVALID


def test_call_order_with_a_sampler_attached(lib, handle):
    """Attached, but no state bound / no scenarios loaded: the usual FTL_E_STATE, before the window check and any device work."""
    out, act = abi.Outputs(), C.c_void_p(FAKE)
    assert lib.ftl_set_scenario_sampler(handle, C.byref(_sampler())) == 0
    assert lib.ftl_step(handle, act, C.byref(out), abi.FTL_STEP_SAMPLE_RESET, None) == abi.FTL_E_STATE
    assert b"ftl_bind_state" in lib.ftl_last_error()
    assert lib.ftl_sampler_start(handle, C.byref(out), None) == abi.FTL_E_STATE
    assert b"ftl_bind_state" in lib.ftl_last_error()


def _attach_both(lib, handle):
    from test_queue_abi import _queue
    assert lib.ftl_set_episode_queue(handle, C.byref(_queue())) == 0, lib.ftl_last_error()
    assert lib.ftl_set_scenario_sampler(handle, C.byref(_sampler())) == 0, lib.ftl_last_error()


def test_queue_and_sampler_on_one_handle_are_detached_one_by_one(lib, handle):
    """Both attached to one handle; detaching either leaves the other attached: its step and start calls pass the attachment check and
    fail on ftl_bind_state (as test_call_order_with_a_sampler_attached), those of the detached one fail with their own message."""
    out, act = abi.Outputs(), C.c_void_p(FAKE)
    queue = (lib.ftl_set_episode_queue, abi.FTL_STEP_QUEUE_RESET, lib.ftl_queue_start,
             b"FTL_STEP_QUEUE_RESET without an episode queue (ftl_set_episode_queue)", b"ftl_set_episode_queue has not been called")
    sampler = (lib.ftl_set_scenario_sampler, abi.FTL_STEP_SAMPLE_RESET, lib.ftl_sampler_start,
               b"FTL_STEP_SAMPLE_RESET without a scenario sampler (ftl_set_scenario_sampler)", b"ftl_set_scenario_sampler has not been called")
    for gone, kept in ((queue, sampler), (sampler, queue)):
        _attach_both(lib, handle)
        assert gone[0](handle, None) == 0
        assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), None, gone[1], None) == abi.FTL_E_STATE
        assert lib.ftl_last_error() == gone[3]
        assert gone[2](handle, C.byref(out), None) == abi.FTL_E_STATE
        assert lib.ftl_last_error() == gone[4]
        assert lib.ftl_step_final(handle, act, abi.FTL_ACTION_BOX2, C.byref(out), None, kept[1], None) == abi.FTL_E_STATE
        assert b"ftl_bind_state" in lib.ftl_last_error()
        assert kept[2](handle, C.byref(out), None) == abi.FTL_E_STATE
        assert b"ftl_bind_state" in lib.ftl_last_error()


_DEVICE_STUB = """
static int calls;
int hipSetDevice(int device) { (void)device; calls++; return 100; }
int hipFree(void* p) { (void)p; calls++; return 100; }
int device_calls(void) { return calls; }
"""

_DESTROY_SCRIPT = """
import ctypes as C, sys
stub = C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL)      # loaded first, so the library's hipSetDevice / hipFree resolve to the counting ones
from continiousenvironment_follower_leader_amd import _lib, abi, make_config
lib = C.CDLL(_lib.SO_PATH)
cfg, h = make_config(bear_number=1), C.c_void_p()
assert lib.ftl_create(C.byref(cfg.c), 4, 0, C.byref(h)) == 0
q, s = abi.EpisodeQueueC(), abi.ScenarioSamplerC()
q.scenario = q.head = q.records = q.ticket = s.weight = s.cdf = s.table = 4096
q.n = s.count = 8
assert lib.ftl_set_episode_queue(h, C.byref(q)) == 0 and lib.ftl_set_scenario_sampler(h, C.byref(s)) == 0
before = stub.device_calls()
assert lib.ftl_sampler_refresh(h, None) == abi.FTL_E_DEVICE and stub.device_calls() == before + 1      # the stub is what the library calls
lib.ftl_destroy(h)
assert stub.device_calls() == before + 1, "ftl_destroy touched the device"
"""


def test_destroy_with_both_attached_and_nothing_launched_leaves_the_device_alone(lib, tmp_path):
    """A process of its own, in which a counting hipSetDevice / hipFree stands in front of the runtime's."""
    (tmp_path / "stub.c").write_text(_DEVICE_STUB)
    so = str(tmp_path / "libstub.so")
    subprocess.check_call([_lib.HIPCC, "-x", "c", "-shared", "-fPIC", str(tmp_path / "stub.c"), "-o", so])
    subprocess.check_call([sys.executable, "-c", _DESTROY_SCRIPT, so], cwd=ROOT)


def test_python_mode_needs_no_device():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame, VecGame
    g = VecGame.__new__(VecGame)
    g._fin, g.queue, g.sampler = None, None, None
    with pytest.raises(_lib.FtlError, match="set_scenario_sampler"):
        g._step_mode("sample")
    g.sampler = object()
    assert g._step_mode("sample") == (abi.FTL_STEP_SAMPLE_RESET, None)
    with pytest.raises(ValueError, match='"sample"'):
        g._step_mode("no such mode")
    for cls in (VecGame, PipelinedVecGame):
        b = cls.__new__(cls)
        b.sampler = None
        for method in (b.reset_from_sampler, b.refresh_sampler):
            with pytest.raises(_lib.FtlError, match="set_scenario_sampler"):
                method()


# ---------------------------------------------------------------- the draw: a restatement of the header's text
def _mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _restated(rng_seed, stream_id, resets, weights):
    """idx by the header's text: x = the raw 64 bits of the mix at frame key bit 42, r = (x * total) >> 64, idx = number of cdf entries
    <= r (``bisect_right`` on the cumulative sum of Python integers); total == 0: (x * count) >> 64."""
    cdf = list(np.cumsum(np.array(weights, dtype=object)))
    key = _mix64(rng_seed + 0x9E3779B97F4A7C15 * (stream_id + 1)) ^ _mix64(0xD1B54A32D192ED03 * (resets + 1))
    x = _mix64(key + 0x9E3779B97F4A7C15 * ((1 << 42) + 1))
    total = cdf[-1]
    if total == 0:
        return (x * len(cdf)) >> 64
    return bisect.bisect_right(cdf, (x * total) >> 64)


def _cdf(weights):
    out, acc = [], 0
    for w in weights:
        acc += w
        out.append(acc)
    return out


_DRAWS = {}


def _draws(k):
    """The 100,320 draws of weight vector k: seeds 0 and 7 x stream ids 0 .. 1044 x resets 0 .. 47 (the twin, computed once)."""
    if k not in _DRAWS:
        cdf = _cdf(WEIGHTS[k])
        _DRAWS[k] = np.array([abi.sample_scenario(seed, sid, rs, cdf) for seed in (0, 7) for sid in range(1045) for rs in range(48)])
    return _DRAWS[k]


@pytest.mark.parametrize("k", range(len(WEIGHTS)))
def test_twin_equals_the_restatement(k):
    w, cdf = WEIGHTS[k], _cdf(WEIGHTS[k])
    d = _draws(k).reshape(2, 1045, 48)
    for seed_i, seed in enumerate((0, 7)):
        for sid in range(0, 1045, 7):
            for rs in range(0, 48, 5):
                assert d[seed_i, sid, rs] == _restated(seed, sid, rs, w), (seed, sid, rs)
    # large ids and seeds, and the base offset
    for seed, sid, rs in ((2 ** 64 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (0x123456789ABCDEF0, 123456789, 4000), (1, 0, 0)):
        assert abi.sample_scenario(seed, sid, rs, cdf, base=11) == 11 + _restated(seed, sid, rs, w)


@pytest.mark.parametrize("k", range(len(WEIGHTS)))
def test_zero_weights_are_never_drawn_and_frequencies_follow_the_weights(k):
    w = np.array(WEIGHTS[k], dtype=object)
    d = _draws(k)
    n = len(d)
    assert n == 100320 and d.min() >= 0 and d.max() < len(w)
    counts = np.bincount(d, minlength=len(w))
    total = int(w.sum())
    worst = 0.0
    for i, wi in enumerate(w):
        if wi == 0:
            assert counts[i] == 0, i
            continue
        p = int(wi) / total
        dev, sd = abs(counts[i] - n * p), math.sqrt(n * p * (1 - p))
        assert dev <= 5 * sd, (i, counts[i], n * p, sd)          # (p = 1: the entry takes every draw)
        worst = max(worst, dev / sd if sd > 0 else 0.0)
    print("weights %d: worst entry at %.2f binomial standard deviations" % (k, worst))


def test_all_zero_weights_give_the_uniform_form():
    count = 13
    cdf = [0] * count
    got = [abi.sample_scenario(3, sid, rs, cdf) for sid in range(200) for rs in range(20)]
    for (sid, rs), g in zip(((s, r) for s in range(200) for r in range(20)), got):
        assert g == _restated(3, sid, rs, [0] * count)
    counts = np.bincount(got, minlength=count)
    n, p = len(got), 1.0 / count
    assert len(counts) == count and (abs(counts - n * p) <= 5 * math.sqrt(n * p * (1 - p))).all()


def test_header_function_equals_the_twin(tmp_path):
    """include/ftl.h's own ftl_sample_scenario, compiled for the host, on the four weight vectors and the all-zero one."""
    vectors = list(WEIGHTS) + [[0] * 13]
    cases = [(seed, sid, rs) for seed in (0, 7, 2 ** 64 - 1) for sid in (0, 1, 63, 1044, 2 ** 31 - 1) for rs in (0, 1, 47, 2 ** 31 - 1)]
    src = ['#include <stdio.h>', '#include "ftl.h"', "int main(void) {"]
    for v, w in enumerate(vectors):
        src.append("    static const uint64_t cdf%d[] = {%s};" % (v, ", ".join("%dULL" % c for c in _cdf(w))))
        for seed, sid, rs in cases:
            src.append('    printf("%%d\\n", ftl_sample_scenario(%dULL, %dULL, %dULL, cdf%d, %d));' % (seed, sid, rs, v, len(w)))
    src += ["    return 0;", "}"]
    (tmp_path / "draw.cpp").write_text("\n".join(src))
    exe = str(tmp_path / "draw")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "draw.cpp"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [abi.sample_scenario(seed, sid, rs, _cdf(w)) for w in vectors for seed, sid, rs in cases]
    assert got == want


# ---------------------------------------------------------------- ScenarioSampler.set_weights (the class holds weights on a CPU device too)
def test_set_weights_quantisation_and_rejections():
    import torch
    from continiousenvironment_follower_leader_amd import ScenarioSampler
    s = ScenarioSampler(6, base=2, device="cpu")
    s.set_weights(torch.tensor([0.0, 1e-30, 3.0, 1.5, 0.75, 3.0 * (2.5 / 2 ** 24)]))
    # rint(w / max * 2**24): 0 stays 0, a positive weight is at least 1, the tie 2.5 goes to the even 2
    assert s.raw_weights().tolist() == [0, 1, 2 ** 24, 2 ** 23, 2 ** 22, 2]
    s.set_weights(torch.tensor([0.0, 0.0, 3.5 / 2 ** 24, 1.0, 0.0, 0.0], dtype=torch.float32))
    assert s.raw_weights().tolist() == [0, 0, 4, 2 ** 24, 0, 0]                 # the tie 3.5 goes to the even 4
    s.set_weights(torch.zeros(6))                                               # all zero is allowed: uniform
    assert s.raw_weights().tolist() == [0] * 6
    s.set_weights(np.array([5, 0, 0, 0, 0, 10]))                                # (integers are taken as floats)
    assert s.raw_weights().tolist() == [2 ** 23, 0, 0, 0, 0, 2 ** 24]
    for bad in ([1.0, -1e-9, 0, 0, 0, 0], [1.0, float("nan"), 0, 0, 0, 0], [1.0, float("inf"), 0, 0, 0, 0], [1.0, 2.0], [1.0] * 7):
        with pytest.raises(ValueError):
            s.set_weights(torch.tensor(bad))
    assert s.raw_weights().tolist() == [2 ** 23, 0, 0, 0, 0, 2 ** 24]           # a rejected call changes nothing
    s.set_raw_weights(torch.tensor([0, U32, 2 ** 31, 2 ** 31 - 1, 1, 7]))
    assert s.raw_weights().tolist() == [0, U32, 2 ** 31, 2 ** 31 - 1, 1, 7]
    for bad in (torch.tensor([0, U32 + 1, 0, 0, 0, 0]), torch.tensor([0, -1, 0, 0, 0, 0]), torch.tensor([1.0] * 6), torch.tensor([1, 2])):
        with pytest.raises(ValueError):
            s.set_raw_weights(bad)
    sd = s.state_dict()
    t = ScenarioSampler(6, base=2, device="cpu")
    t.load_state_dict(sd)
    assert t.raw_weights().tolist() == s.raw_weights().tolist()
    with pytest.raises(ValueError):
        ScenarioSampler(5, base=2, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError):
        ScenarioSampler(0, device="cpu")
    tab = s.table()
    assert set(abi.SS_NAMES) | {"mean_return", "success_rate"} == set(tab) and all(v.shape == (6,) for v in tab.values())
