"""CPU checks of the PPO loss head (include/ftl.h: ``ftl_ppo_head``, ``ftl_sizeof_ppo_head_workspace``, ``ftl_sizeof_ppo_head_args``;
``mlp.ppo_head``, ``mlp.ppo_loss``): the exports and the struct, the workspace query against a segment count by hand, every refusal that
comes before any device work -- on a handle that never got a state, and never with a call that would pass them all, so nothing here can
launch --, and the Python argument checks on CPU tensors with the library patched out."""
import ctypes as C
import inspect
import re

import pytest
import torch

import ppo_numpy as P
import test_mlp_abi as A
from continiousenvironment_follower_leader_amd import _lib, abi, mlp
from test_mlp_abi import cfg_b, handle, lib  # noqa: F401  (fixtures)

FAKE = A.FAKE
LAST = b"workspace must be 8-byte aligned"  # the last check of ftl_ppo_head: a call refused with it has passed every other one
BIG = 1 << 40
B, N, S = 2, 12, 3

POINTERS = ("head_new", "head_old", "noise", "sigma_old", "sigma_new", "log_sigma_shift", "adv", "ret", "value_new", "kind", "dhead", "dvalue",
            "dlog_std", "stats", "workspace")
REQUIRED = tuple(p for p in POINTERS if p not in ("log_sigma_shift", "value_new", "dvalue"))
STRIDES = dict(head_new=8, head_old=8, noise=8, adv=4, ret=4, value_new=4, kind=1, dhead=8, dvalue=4)     # bytes of a row at width 2


def _args(**over):
    a = abi.PpoHeadArgs()
    a.n_blocks, a.n, a.n_sets, a.width = B, N, S, 2
    for i, p in enumerate(POINTERS):
        setattr(a, p, FAKE * (i + 1))
    n, w = over.get("n", N), over.get("width", 2)
    for p, row in STRIDES.items():
        setattr(a, p + "_block_bytes", n * (row if row != 8 else 4 * max(w, 1)))
    a.clip_lo, a.clip_hi, a.vf_coef, a.normalize, a.workspace_bytes = 0.8, 1.2, 0.5, 1, BIG
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _call(lib, h, **over):
    return lib.ftl_ppo_head(h, C.byref(_args(**over)), None)


def _passes_all_but_the_last(lib, h, **over):
    """The call with a misaligned workspace: FTL_E_INVALID with the message of the last check, so every check before it let the call pass."""
    rc = _call(lib, h, **dict(over, workspace=15 * FAKE + 4))
    return rc == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()


def test_symbols_declared_exported_and_listed(lib):
    hdr = A._header()
    for s in ("ftl_ppo_head", "ftl_sizeof_ppo_head_workspace", "ftl_sizeof_ppo_head_args"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s) and s in _lib.EXPORTS, s
    assert lib.ftl_ppo_head.restype is C.c_int and len(lib.ftl_ppo_head.argtypes) == 3
    assert lib.ftl_sizeof_ppo_head_workspace.restype is C.c_int64
    assert C.sizeof(abi.PpoHeadArgs) == lib.ftl_sizeof_ppo_head_args() == 232
    assert int(re.search(r"#define\s+FTL_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.FTL_ABI_VERSION == 4      # new names only
    assert int(re.search(r"#define\s+FTL_PPO_SEG\s+(\d+)", hdr).group(1)) == abi.FTL_PPO_SEG == P.SEG
    assert int(re.search(r"#define\s+FTL_PPO_STATS\s+(\d+)", hdr).group(1)) == abi.FTL_PPO_STATS == P.STATS == 8
    body = re.search(r"typedef struct ftl_ppo_head_args \{(.*?)\} ftl_ppo_head_args;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [f[0] for f in abi.PpoHeadArgs._fields_]                  # the same fields in the same order


def test_workspace_query_against_a_segment_count_by_hand(lib):
    q = lib.ftl_sizeof_ppo_head_workspace
    seg = abi.FTL_PPO_SEG
    # (B, n, n_sets) -> segments of a set's slice, counted by hand
    for Bk, n, sets, sps in ((1, 1, 1, 1), (2, 5, 5, 1), (2, 63, 1, 1), (2, 1024, 1, 1), (2, 1025, 1, 2), (3, 33, 3, 1), (1, 3 * 2049, 3, 3),
                             (7, 4096, 2, 2), (32, 65536, 1024, 1), (32, 65536, 1, 64), (5, 2 * seg + 1, 1, 3), (65535, 64, 64, 1)):
        assert q(Bk, n, sets) == Bk * sets * sps * 72 + sets * 16 == P.workspace_bytes(Bk, n, sets), (Bk, n, sets)
    for Bk in (1, 2, 9):
        for sets in (1, 2, 3, 8):
            for rows in (1, 2, 63, 64, 65, seg - 1, seg, seg + 1, 3 * seg, 3 * seg + 5):
                assert q(Bk, sets * rows, sets) == Bk * sets * ((rows + seg - 1) // seg) * 72 + sets * 16
    for bad in ((0, 4, 2), (-1, 4, 2), (1, 0, 1), (1, -4, 2), (1, 4, 0), (1, 4, -2), (1, 4, 3), (1, 5, 2), (1 << 20, 1 << 20, 1 << 20)):
        assert q(*bad) == -1, bad


def test_null_arguments_are_named(lib, handle):
    assert lib.ftl_ppo_head(None, C.byref(_args()), None) == abi.FTL_E_INVALID and lib.ftl_last_error().endswith(b": h")
    assert lib.ftl_ppo_head(handle, None, None) == abi.FTL_E_INVALID and lib.ftl_last_error().endswith(b": a")
    for p in REQUIRED:
        assert _call(lib, handle, **{p: None}) == abi.FTL_E_INVALID, p
        err = lib.ftl_last_error()
        assert b"ftl_ppo_head" in err and b"null" in err and err.endswith(b": " + p.encode()), (p, err)
    assert _call(lib, handle, value_new=None) == abi.FTL_E_INVALID and b"dvalue without value_new" in lib.ftl_last_error()
    assert _call(lib, handle, dvalue=None) == abi.FTL_E_INVALID and b"value_new without dvalue" in lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, handle, value_new=None, dvalue=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, handle, log_sigma_shift=None), lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, handle, value_new=None, dvalue=None, value_new_block_bytes=0, dvalue_block_bytes=-3)       # unread without the pointers


def test_counts_and_width(lib, handle):
    h = handle
    for kw in (dict(n_blocks=0), dict(n_blocks=-2), dict(n=0), dict(n=-12)):
        assert _call(lib, h, **kw) == abi.FTL_E_INVALID and b"ftl_ppo_head: n_blocks and n" in lib.ftl_last_error(), kw
    for kw in (dict(n_sets=0), dict(n_sets=-1), dict(n_sets=5), dict(n_sets=24)):
        assert _call(lib, h, **kw) == abi.FTL_E_INVALID and b"ftl_ppo_head: n_sets" in lib.ftl_last_error(), kw
    for w in (0, 3, 5, -1, 64):
        assert _call(lib, h, width=w) == abi.FTL_E_UNSUPPORTED, w
        err = lib.ftl_last_error()
        assert b"ftl_ppo_head: width" in err and b"Discrete(5)" in err and b"logarithm" in err
    for kw in (dict(width=1), dict(width=2), dict(n_sets=1), dict(n_sets=12), dict(n_blocks=1), dict(n_blocks=65536, n=64, n_sets=64)):
        assert _passes_all_but_the_last(lib, h, **kw), (kw, lib.ftl_last_error())
    assert _call(lib, h, n_blocks=1 << 20, n=1 << 20, n_sets=1 << 20) == abi.FTL_E_UNSUPPORTED and b"segments" in lib.ftl_last_error()


def test_strides_alignment_clip_and_workspace(lib, handle):
    h = handle
    for p, row in STRIDES.items():
        word = (p + "_block_bytes").encode()
        for bb in (N * row - row, 0, -N * row):
            assert _call(lib, h, **{p + "_block_bytes": bb}) == abi.FTL_E_INVALID, (p, bb)
            assert b"ftl_ppo_head: " + word in lib.ftl_last_error() and b"below" in lib.ftl_last_error(), (p, bb, lib.ftl_last_error())
        if row > 1:
            assert _call(lib, h, **{p + "_block_bytes": N * row + row // 2}) == abi.FTL_E_INVALID and word + b" not aligned" in lib.ftl_last_error(), p
        assert _passes_all_but_the_last(lib, h, **{p + "_block_bytes": N * row + 5 * row}), (p, lib.ftl_last_error())      # padded blocks are fine
    for i, p in enumerate(POINTERS[:-1]):
        el = 1 if p == "kind" else 8 if p in ("head_new", "head_old", "noise", "dhead", "stats") else 4
        if el == 1:
            assert _passes_all_but_the_last(lib, h, kind=FAKE * (i + 1) + 3)
            continue
        for off in {1, 2, el // 2}:
            assert _call(lib, h, **{p: FAKE * (i + 1) + off}) == abi.FTL_E_INVALID, (p, off)
            assert b"ftl_ppo_head: " + p.encode() + b" not aligned" in lib.ftl_last_error(), (p, off, lib.ftl_last_error())
    assert _passes_all_but_the_last(lib, h, width=1, head_new=FAKE + 4, head_old=2 * FAKE + 4, noise=3 * FAKE + 4, dhead=11 * FAKE + 4)    # width 1: 4-byte rows
    nan = float("nan")
    for lo, hi in ((1.2, 0.8), (nan, 1.2), (0.8, nan), (nan, nan), (1.0000001, 1.0)):
        assert _call(lib, h, clip_lo=lo, clip_hi=hi) == abi.FTL_E_INVALID and b"ftl_ppo_head: clip_lo" in lib.ftl_last_error(), (lo, hi)
    for lo, hi in ((1.0, 1.0), (0.0, float("inf")), (0.8, 1.2)):
        assert _passes_all_but_the_last(lib, h, clip_lo=lo, clip_hi=hi), (lo, hi)
    for v in (2, -1):
        assert _call(lib, h, normalize=v) == abi.FTL_E_INVALID and b"ftl_ppo_head: normalize" in lib.ftl_last_error()
    assert _passes_all_but_the_last(lib, h, normalize=0)
    need = lib.ftl_sizeof_ppo_head_workspace(B, N, S)
    assert need == B * S * 72 + S * 16
    for wsb in (need - 1, need - 8, 0, -8):
        assert _call(lib, h, workspace_bytes=wsb) == abi.FTL_E_INVALID and b"ftl_ppo_head: workspace_bytes" in lib.ftl_last_error(), wsb
    assert _passes_all_but_the_last(lib, h, workspace_bytes=need)
    for off in (1, 2, 4, 7):
        assert _call(lib, h, workspace=15 * FAKE + off) == abi.FTL_E_INVALID and LAST in lib.ftl_last_error()


def test_python_surface(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("a library call before the argument checks were through")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(mlp, "_device_handle", no_library)
    p = inspect.signature(mlp.ppo_head).parameters
    assert list(p) == ["head", "head_old", "noise", "sigma_old", "sigma", "adv", "ret", "kind", "value", "log_sigma_shift", "clip", "vf_coef",
                       "normalize", "out"]
    assert [p[k].default for k in list(p)[8:]] == [None, None, 0.2, 0.5, True, None]
    p = inspect.signature(mlp.ppo_loss).parameters
    assert list(p) == ["traj", "head", "log_std", "adv", "ret", "value", "log_std_old", "clip", "vf_coef", "normalize"]
    assert [p[k].default for k in list(p)[5:]] == [None, None, 0.2, 0.5, True]

    T, n, Aw, sets = 3, 6, 2, 2
    z = lambda *s, **k: torch.zeros(*s, **k)
    good = dict(head=z(T, n, Aw), head_old=z(T, n, Aw), noise=z(T, n, Aw), sigma_old=torch.ones(sets, Aw), sigma=torch.ones(sets, Aw),
                adv=z(T, n), ret=z(T, n), kind=z(T, n, dtype=torch.uint8), value=z(T, n), log_sigma_shift=z(sets, Aw))
    bad = [dict(head=None), dict(head=z(T, n, Aw, dtype=torch.float64)), dict(head=z(T, n, 2 * Aw)[:, :, ::2]), dict(head=z(T, n, Aw, requires_grad=True)),
           dict(head=z(Aw)), dict(head=z(0, n, Aw)), dict(head=z(T, n + 1, Aw)),
           dict(head_old=z(T, n, 1)), dict(head_old=None), dict(head_old=z(T, n, Aw, dtype=torch.float64)),
           dict(noise=z(T, n + 1, Aw)), dict(noise=None), dict(noise=z(T, 2 * n, Aw)[:, ::2]),
           dict(sigma=torch.ones(sets, 1)), dict(sigma=torch.ones(Aw)), dict(sigma=None), dict(sigma=torch.ones(4, Aw)), dict(sigma=torch.ones(sets, Aw, requires_grad=True)),
           dict(sigma_old=torch.ones(1, Aw)), dict(sigma_old=None), dict(sigma_old=torch.ones(sets, Aw, dtype=torch.float64)),
           dict(log_sigma_shift=z(1, Aw)), dict(log_sigma_shift=z(sets, Aw, dtype=torch.float64)),
           dict(adv=z(T, n, 1)), dict(adv=None), dict(adv=z(T, n, dtype=torch.float64)), dict(ret=z(n)), dict(ret=None),
           dict(kind=z(T, n)), dict(kind=z(T, n, dtype=torch.bool)), dict(kind=None), dict(kind=z(T, n + 1, dtype=torch.uint8)),
           dict(value=z(T, n, 1)), dict(value=z(T, n, dtype=torch.float64)), dict(value=z(T, n, requires_grad=True)),
           dict(clip=-0.1), dict(clip=float("nan")), dict(clip=float("inf")),
           dict(out=0), dict(out=mlp.PpoHead(z(T, n, Aw), None, z(sets, Aw), z(sets, 8, dtype=torch.float64))),
           dict(out=mlp.PpoHead(z(T, n, Aw), z(T, n), z(sets, Aw), z(sets, 8))), dict(out=mlp.PpoHead(z(T, n, 1), z(T, n), z(sets, Aw), z(sets, 8, dtype=torch.float64))),
           dict(value=None, out=mlp.PpoHead(z(T, n, Aw), z(T, n), z(sets, Aw), z(sets, 8, dtype=torch.float64)))]
    for over in bad:
        with pytest.raises(ValueError):
            mlp.ppo_head(**dict(good, **over))
    for w in (3, 5):
        with pytest.raises(NotImplementedError, match="Discrete"):
            mlp.ppo_head(**dict(good, head=z(T, n, w), head_old=z(T, n, w), noise=z(T, n, w)))
    with pytest.raises(ValueError, match="GPU"):                               # every argument fine but the device: still no library call
        mlp.ppo_head(**good)
    with pytest.raises(ValueError, match="GPU"):
        mlp.ppo_head(**dict(good, value=None, log_sigma_shift=None, out=mlp.PpoHead(z(T, n, Aw), None, z(sets, Aw), z(sets, 8, dtype=torch.float64))))

    traj = mlp.Trajectory(obs=z(T + 1, n, 4), head=z(T, n, Aw), action=z(T, n, Aw), reward=z(T, n, dtype=torch.float64),
                          kind=z(T, n, dtype=torch.uint8), noise=z(T, n, Aw), sigma=torch.ones(sets, Aw))
    head, log_std = z(T, n, Aw, requires_grad=True), z(sets, Aw, requires_grad=True)
    for kw in (dict(head=z(T, n, 1)), dict(head=None), dict(log_std=z(1, Aw)), dict(log_std=z(sets, Aw, dtype=torch.float64)),
               dict(value=z(T, n + 1)), dict(value=z(T, n, 2)), dict(log_std_old=z(1, Aw)), dict(log_std_old=z(sets, Aw, requires_grad=True))):
        with pytest.raises(ValueError):
            mlp.ppo_loss(**dict(dict(traj=traj, head=head, log_std=log_std, adv=z(T, n), ret=z(T, n)), **kw))
    with pytest.raises(ValueError, match="noise"):
        mlp.ppo_loss(mlp.Trajectory(traj.obs, traj.head, traj.action, traj.reward, traj.kind), head, log_std, z(T, n), z(T, n))
    for value in (None, z(T, n, requires_grad=True), z(T, n, 1, requires_grad=True)):
        with pytest.raises(ValueError, match="GPU"):                           # through the autograd function, down to the device check
            mlp.ppo_loss(traj, head, log_std, z(T, n), z(T, n), value)
