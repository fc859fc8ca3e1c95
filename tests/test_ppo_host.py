"""CPU tests of the PPO loss head's arithmetic (include/ftl.h, the ftl_ppo_head block): csrc/ftl_ppo_math.hpp compiled for the host against
the twin (tests/ppo_numpy.py) bit for bit on random and crafted rows, the twin's reductions against their definition, and the twin --
in its float32 form and in its exact float64 form -- against torch float64 autograd on the loss of INTEGRATION.md's example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ppo_numpy as P
from continiousenvironment_follower_leader_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# The worst deviations of the twin from torch float64 autograd on the inputs of _example() (120 rows, a fifth VOID; 3 sets of 40 for the
# population form), measured on the CPU and recorded in DESIGN.md 8.24; the tests assert 8 x these, the margin of tests/test_rnn_backward_abi.py.
MEASURED = {
    "float32": dict(ratio=1.93e-6, dhead=2.74e-7, dvalue=7.71e-10, dlog_std=2.25e-7, loss=5.60e-8),
    "exact": dict(ratio=2.23e-15, dhead=5.56e-16, dvalue=2.0 ** -53, dlog_std=4.45e-16, loss=5.56e-17),     # (dvalue measured 0: one float64 ulp of 0.5 instead)
}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/ftl_ppo_math.hpp compiled for the host with -ffp-contract=off into a small library."""
    d = tmp_path_factory.mktemp("ppo_math")
    src = d / "ppo_math.cpp"
    src.write_text('#include "ftl_ppo_math.hpp"\n'
                   "using namespace ftlppomath;\n"
                   'extern "C" void ppo_rows(int A, const Set* s, const float* hn, const float* ho, const float* nz, const float* adv, const float* ret,\n'
                   "                         const float* v, float* f, int* clipped, long n) {\n"
                   "    for (long i = 0; i < n; i++) {\n"
                   "        Row r;\n"
                   "        if (A == 2) row<2>(*s, hn + 2 * i, ho + 2 * i, nz + 2 * i, adv[i], ret[i], v[i], r);\n"
                   "        else row<1>(*s, hn + i, ho + i, nz + i, adv[i], ret[i], v[i], r);\n"
                   "        float* o = f + 9 * i;\n"
                   "        o[0] = r.dhead[0]; o[1] = r.dhead[1]; o[2] = r.dvalue; o[3] = r.ratio; o[4] = r.pl; o[5] = r.vl; o[6] = r.nd; o[7] = r.k[0]; o[8] = r.k[1];\n"
                   "        clipped[i] = r.clipped;\n"
                   "    }\n}\n"
                   'extern "C" void ppo_moments(double cnt, double S1, double S2, double* d, float* f) {\n'
                   "    const Moments m = moments(cnt, S1, S2);\n"
                   "    d[0] = m.mean; d[1] = m.std; f[0] = m.mean32; f[1] = m.inv32; f[2] = m.invc;\n}\n"
                   'extern "C" unsigned long ppo_sizeof_set(void) { return sizeof(Set); }\n')
    so = str(d / "libppo_math.so")
    subprocess.check_call([_lib.HIPCC, "-x", "c++", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I", os.path.join(ROOT, "continiousenvironment_follower_leader_amd", "csrc"), str(src), "-o", so])
    lib = C.CDLL(so)
    lib.ppo_rows.argtypes = [C.c_int] + [C.c_void_p] * 9 + [C.c_long]
    lib.ppo_rows.restype = None
    lib.ppo_moments.argtypes = [C.c_double] * 3 + [C.c_void_p] * 2
    lib.ppo_moments.restype = None
    lib.ppo_sizeof_set.restype = C.c_ulong
    return lib


class _Set(C.Structure):
    _fields_ = [("sigma_new", C.c_float * 2), ("sigma_old", C.c_float * 2), ("shift", C.c_float * 2), ("mean32", C.c_float), ("inv32", C.c_float),
                ("invc", C.c_float), ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("vf_coef", C.c_float), ("normalize", C.c_int),
                ("has_value", C.c_int)]


def _host_rows(host, A, rows, sig_old, sig_new, shift, mean32, inv32, invc, lo, hi, vf, normalize, has_value):
    assert host.ppo_sizeof_set() == C.sizeof(_Set)
    s = _Set()
    for j in range(A):
        s.sigma_new[j], s.sigma_old[j], s.shift[j] = sig_new[j], sig_old[j], shift[j]
    s.mean32, s.inv32, s.invc, s.clip_lo, s.clip_hi, s.vf_coef, s.normalize, s.has_value = mean32, inv32, invc, lo, hi, vf, normalize, has_value
    arr = {k: np.ascontiguousarray(rows[k], F) for k in ("head_new", "head_old", "noise", "adv", "ret", "value")}
    n = arr["adv"].size
    f, cl = np.empty((n, 9), F), np.empty(n, np.int32)
    host.ppo_rows(A, C.addressof(s), *(arr[k].ctypes.data for k in ("head_new", "head_old", "noise", "adv", "ret", "value")), f.ctypes.data,
                  cl.ctypes.data, n)
    return f, cl


def _twin_rows(A, rows, sig_old, sig_new, shift, mean32, inv32, invc, lo, hi, vf, normalize, has_value):
    n = rows["adv"].size
    rep = lambda v: np.broadcast_to(np.asarray(v, F)[None, :A], (n, A))
    full = lambda v: np.full(n, v, F)
    o = P.rows(rows["head_new"], rows["head_old"], rows["noise"], rep(sig_old), rep(sig_new), rep(shift), rows["adv"], rows["ret"],
               rows["value"] if has_value else None, full(mean32), full(inv32), full(invc), F(lo), F(hi), F(vf), normalize)
    f = np.zeros((n, 9), F)
    f[:, :A], f[:, 7:7 + A] = o["dhead"], o["k"]
    f[:, 2] = o["dvalue"] if has_value else 0
    f[:, 3], f[:, 4], f[:, 5], f[:, 6] = o["ratio"], o["pl"], o["vl"], o["nd"]
    return f, o["clipped"].astype(np.int32)


def _same(name, got, want):
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))       # bit for bit, NaNs in the same places
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


@pytest.mark.parametrize("A", [1, 2])
def test_header_equals_the_twin_bit_for_bit_on_random_rows(host, A):
    rng = np.random.default_rng(17 + A)
    n = 40_000
    rows = dict(head_old=rng.standard_normal((n, A)).astype(F), noise=rng.standard_normal((n, A)).astype(F),
                adv=rng.standard_normal(n).astype(F), ret=rng.standard_normal(n).astype(F), value=rng.standard_normal(n).astype(F))
    rows["head_new"] = (rows["head_old"] + (rng.standard_normal((n, A)) * rng.choice([0.0, 1e-3, 0.05, 0.5, 5.0], (n, 1))).astype(F)).astype(F)
    rows["noise"][::97] *= F(6.0)                                             # large draws: |d| beyond 86 on some rows
    rows["adv"][::89] = F(0.0)
    for k in ("head_new", "noise", "adv", "value"):                          # NaN and infinity in every input
        rows[k].reshape(-1)[rng.integers(0, rows[k].size, 20)] = rng.choice([np.nan, np.inf, -np.inf], 20).astype(F)
    for sig_old, sig_new, shift, normalize, has_value in (((0.4, 0.3), (0.4, 0.3), (0.0, 0.0), 0, 1), ((0.37, 0.52), (0.35, 0.55), (-0.0556, 0.0561), 1, 1),
                                                          ((0.2, 0.9), (0.25, 0.8), (0.2231, -0.1178), 1, 0)):
        args = (A, rows, sig_old, sig_new, shift, F(0.123), F(0.87), F(1.0 / 777.0), F(0.8), F(1.2), F(0.5), normalize, has_value)
        (f, c), (tf, tc) = _host_rows(host, *args), _twin_rows(*args)
        _same("rows", f, tf)
        assert (c == tc).all()
        assert np.isnan(tf[:, 3]).any() and (tc == 1).any() and (tc == 0).any() and (tf[:, 0] == 0).any() and (tf[:, 0] != 0).any()


@pytest.mark.parametrize("A", [1, 2])
def test_header_equals_the_twin_on_crafted_rows(host, A):
    cr = P.crafted(A)
    sg = tuple(cr["sigma"][0]) + (0.0,) * (2 - A)
    base = (A, cr, sg, sg, (0.0, 0.0), F(0.0), F(1.0), F(1.0 / 12.0))
    t0, _ = _twin_rows(*base, F(0.8), F(1.2), F(0.5), 0, 1)
    lo, hi = t0[0, 3], t0[1, 3]
    assert 0.7 < lo < 0.9 and 1.2 < hi < 1.5
    args = base + (lo, hi, F(0.5), 0, 1)
    (f, c), (tf, tc) = _host_rows(host, *args), _twin_rows(*args)
    _same("crafted", f, tf)
    assert (c == tc).all()
    r, g0 = tf[:, 3], tf[:, 0]
    assert r[0] == lo and r[1] == hi and tc[0] == 0 and tc[1] == 0 and g0[0] != 0 and g0[1] != 0      # at the bounds: not clipped, the gradient flows
    assert r[2] > hi and r[3] < lo and tc[2:6].tolist() == [1, 1, 1, 1]
    assert g0[2] == 0 and g0[3] != 0 and g0[4] != 0 and g0[5] == 0            # a > 0 above, a > 0 below, a < 0 above, a < 0 below
    assert g0[6] == 0 and tf[6, 4] == 0                                      # a = 0
    assert r[7] > 1 and np.isfinite(r[8]) and r[8] > 1e37 and 0 < r[9] < 1e-37
    assert abs(float(r[10]) - 1) <= 2 ** -22 and abs(float(r[11]) - 1) <= 2 ** -22 and np.abs(tf[10:, 6]).max() <= 2.4e-7


def test_moments_equal_the_twin(host):
    rng = np.random.default_rng(3)
    cases = [(0.0, 0.0, 0.0), (1.0, 0.7, 0.49), (2.0, 0.0, 0.0), (2.0, 3.0, 4.5), (5.0, 1.0, 0.1), (3.0, float("nan"), 1.0), (4.0, 2.0, float("inf"))]
    cases += [(float(c), float(s), float(abs(q)) + s * s / c) for c, s, q in zip(rng.integers(2, 5000, 200), rng.standard_normal(200) * 30, rng.standard_normal(200) * 50)]
    for cnt, S1, S2 in cases:
        d, f = np.empty(2), np.empty(3, F)
        host.ppo_moments(cnt, S1, S2, d.ctypes.data, f.ctypes.data)
        mean, std, mean32, inv32, invc = P.moments(np.array([cnt]), np.array([S1]), np.array([S2]))
        want_d, want_f = np.array([mean[0], std[0]]), np.array([mean32[0], inv32[0], invc[0]], F)
        assert (d.view(np.uint64) == want_d.view(np.uint64)).all() or (np.isnan(d) == np.isnan(want_d)).all() and np.isnan(d).any(), (cnt, S1, S2, d, want_d)
        assert (f.view(np.uint32) == want_f.view(np.uint32)).all() or (np.isnan(f) == np.isnan(want_f)).all() and np.isnan(f).any(), (cnt, S1, S2, f, want_f)
    assert P.moments(np.array([0.0]), np.array([0.0]), np.array([0.0]))[4][0] == 0 and P.moments(np.array([1.0]), np.array([2.0]), np.array([4.0]))[1][0] == 0


def test_segment_sum_is_the_lane_order_of_the_contract():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 200, 1023, 1024):
        x, valid = rng.standard_normal(n) * 1e3, rng.random(n) > 0.2
        lanes = [0.0] * 64
        for i in range(n):
            if valid[i]:
                lanes[i % 64] = lanes[i % 64] + x[i]
        for stride in (32, 16, 8, 4, 2, 1):
            for k in range(stride):
                lanes[k] = lanes[k] + lanes[k + stride]
        assert P.segment_sum(x, valid) == lanes[0]
    x = rng.standard_normal((2, 2 * 1025 + 0))
    valid = np.ones_like(x, bool)
    got = P.set_totals(x, valid, 2)                                           # 2 sets of 1,025 rows: segments of 1,024 and 1, block-major
    for s in range(2):
        want = 0.0
        for b in range(2):
            for lo, hi in ((0, 1024), (1024, 1025)):
                want = want + P.segment_sum(x[b, s * 1025 + lo:s * 1025 + hi], valid[b, lo:hi])
        assert got[s] == want
    assert P.segments(65536, 1024) == (64, 1) and P.segments(65536, 1) == (65536, 64) and P.workspace_bytes(32, 65536, 1024) == 32768 * 72 + 16384


def _example(n_sets, seed=1):
    """120 rows in 2 blocks, a fifth VOID: what a PPO epoch after a few optimizer steps looks like."""
    rng = np.random.default_rng(seed)
    B, n, A = 2, 60, 2
    log_std_old = (rng.standard_normal((n_sets, A)) * 0.2 - 1.0).astype(F)
    log_std = (log_std_old + (rng.standard_normal((n_sets, A)) * 0.05).astype(F)).astype(F)
    head_old = rng.standard_normal((B, n, A)).astype(F)
    head_new = (head_old + (rng.standard_normal((B, n, A)) * 0.1).astype(F)).astype(F)
    noise = rng.standard_normal((B, n, A)).astype(F)
    adv, ret = rng.standard_normal((B, n)).astype(F), rng.standard_normal((B, n)).astype(F)
    value = (ret + rng.standard_normal((B, n)).astype(F) * F(0.3)).astype(F)
    kind = rng.integers(0, 3, (B, n)).astype(np.uint8)
    kind[rng.random((B, n)) < 0.2] = abi.FTL_TR_VOID
    return dict(log_std_old=log_std_old, log_std=log_std, head_old=head_old, head_new=head_new, noise=noise, adv=adv, ret=ret, value=value, kind=kind)


def _torch_loss(e, n_sets, lo, hi, vf):
    """The loss head of INTEGRATION.md's example in float64 under autograd (per member with n_sets > 1), and the float64 check that no
    compared row sits on a tie that torch's min splits."""
    t = {k: torch.from_numpy(v.astype(np.float64)) for k, v in e.items() if k != "kind"}
    head, value, log_std = t["head_new"].requires_grad_(), t["value"].requires_grad_(), t["log_std"].requires_grad_()
    B, n, A = head.shape
    m = torch.from_numpy(e["kind"] != abi.FTL_TR_VOID).view(B, n_sets, -1)
    per = lambda x: x.view(n_sets, 1, A)
    sigma, sigma_old = per(log_std.exp()), per(t["log_std_old"].exp())
    noise, hv = t["noise"].view(B, n_sets, -1, A), head.view(B, n_sets, -1, A)
    z = t["head_old"].view(B, n_sets, -1, A) + sigma_old * noise
    logp = (-0.5 * ((z - hv) / sigma) ** 2 - per(log_std)).sum(-1)
    logp_old = (-0.5 * noise ** 2 - per(t["log_std_old"])).sum(-1)
    ratio = (logp - logp_old).exp()
    adv = t["adv"].view(B, n_sets, -1)
    loss, a_all = 0.0, torch.zeros_like(adv)
    for s in range(n_sets):
        ms = m[:, s]
        a = (adv[:, s] - adv[:, s][ms].mean()) / (adv[:, s][ms].std() + 1e-8)
        a_all[:, s] = a
        rows = -torch.min(ratio[:, s] * a, ratio[:, s].clamp(lo, hi) * a) + vf * 0.5 * (value.view(B, n_sets, -1)[:, s] - t["ret"].view(B, n_sets, -1)[:, s]) ** 2
        loss = loss + rows[ms].mean()
    loss.backward()
    r, a = ratio.detach(), a_all
    tie = (r * a == r.clamp(lo, hi) * a) & ((r < lo) | (r > hi)) & (a != 0) & m
    assert not tie.any()
    return dict(ratio=r.reshape(B, n).numpy(), dhead=head.grad.numpy(), dvalue=value.grad.numpy(), dlog_std=log_std.grad.numpy(), loss=float(loss.detach()))


def _deviations(n_sets, exact):
    e = _example(n_sets)
    lo, hi, vf = F(1 - 0.2), F(1 + 0.2), F(0.5)
    want = _torch_loss(e, n_sets, float(lo), float(hi), float(vf))
    if exact:
        up = lambda v: v.astype(np.float64)
        got = P.head(up(e["head_new"]), up(e["head_old"]), up(e["noise"]), np.exp(up(e["log_std_old"])), np.exp(up(e["log_std"])), up(e["adv"]),
                     up(e["ret"]), e["kind"], up(e["value"]), up(e["log_std"]) - up(e["log_std_old"]), float(lo), float(hi), float(vf), True, exact=True)
    else:
        sig_old = np.exp(e["log_std_old"].astype(np.float64)).astype(F)        # (what torch's float32 exp gives to within an ulp)
        sig_new = np.exp(e["log_std"].astype(np.float64)).astype(F)
        got = P.head(e["head_new"], e["head_old"], e["noise"], sig_old, sig_new, e["adv"], e["ret"], e["kind"], e["value"],
                     (e["log_std"] - e["log_std_old"]).astype(F), lo, hi, vf, True)
    valid = got["valid"]
    dev = {k: float(np.abs(got[k].astype(np.float64) - want[k])[valid if k != "dlog_std" else ...].max()) for k in ("ratio", "dhead", "dvalue", "dlog_std")}
    dev["loss"] = abs(float(got["stats"][:, 7].sum()) - want["loss"])
    assert not got["dhead"][~valid].any() and not got["dvalue"][~valid].any() and np.abs(want["dhead"]).max() > 0.01
    return dev


@pytest.mark.parametrize("mode", ["float32", "exact"])
def test_twin_against_torch_float64_autograd(mode):
    worst = {}
    for n_sets in (1, 3):
        for k, v in _deviations(n_sets, mode == "exact").items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(mode, " ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    for k, v in worst.items():
        assert v <= 8 * MEASURED[mode][k], (k, v, MEASURED[mode][k])
