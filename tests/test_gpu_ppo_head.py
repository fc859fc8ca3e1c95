"""GPU checks of the PPO loss head (include/ftl.h: ``ftl_ppo_head``; ``mlp.ppo_head``, ``mlp.ppo_loss``): the device against the twin
(tests/ppo_numpy.py) bit for bit, NaNs in the same places -- the segment and lane edges, both widths, every optional part, padded blocks
--, the crafted rows, empty and one-row sets, a NaN row that stays in its set, overwrite, reproducibility, ``ppo_loss`` under autograd
through ``mlp.Net`` and ``rnn.Net`` on recorded trajectories, and the wrapper's refusals on device tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_numpy as M
import ppo_numpy as P
import rnn_numpy as R
import rnn_seq_numpy as RS
from continiousenvironment_follower_leader_amd import _lib, abi, mlp, rnn
from test_gpu_collect import SHORT
from test_gpu_mlp import DEV, _vec
from test_gpu_rnn import _rnn

pytestmark = pytest.mark.gpu
F = np.float32
VOID = abi.FTL_TR_VOID
LO, HI = F(1 - 0.2), F(1 + 0.2)                        # what mlp.ppo_head hands down for clip=0.2: rounded once


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(seed, B, n, sets, A, void=0.2):
    rng = np.random.default_rng(seed)
    e = dict(sigma_old=np.exp(rng.standard_normal((sets, A)) * 0.2 - 1.0).astype(F))
    shift = (rng.standard_normal((sets, A)) * 0.05).astype(F)
    e["shift"], e["sigma_new"] = shift, (e["sigma_old"] * np.exp(shift)).astype(F)
    e["head_old"] = rng.standard_normal((B, n, A)).astype(F)
    e["head_new"] = (e["head_old"] + (rng.standard_normal((B, n, A)) * 0.1).astype(F)).astype(F)
    e["noise"] = rng.standard_normal((B, n, A)).astype(F)
    e["adv"], e["ret"] = rng.standard_normal((B, n)).astype(F), rng.standard_normal((B, n)).astype(F)
    e["value"] = (e["ret"] + rng.standard_normal((B, n)).astype(F) * F(0.3)).astype(F)
    e["kind"] = rng.integers(0, 3, (B, n)).astype(np.uint8)
    e["kind"][rng.random((B, n)) < void] = VOID
    e["kind"].flat[0], e["kind"].flat[-1] = VOID, abi.FTL_TR_STEP            # at least one row of each sort
    return e


def _twin(e, value=True, shift=True, normalize=True, lo=LO, hi=HI, vf=0.5):
    return P.head(e["head_new"], e["head_old"], e["noise"], e["sigma_old"], e["sigma_new"], e["adv"], e["ret"], e["kind"],
                  e["value"] if value else None, e["shift"] if shift else None, lo, hi, vf, normalize)


def _call(e, value=True, shift=True, normalize=True, out=None):
    return mlp.ppo_head(_dev(e["head_new"]), _dev(e["head_old"]), _dev(e["noise"]), _dev(e["sigma_old"]), _dev(e["sigma_new"]), _dev(e["adv"]),
                        _dev(e["ret"]), _dev(e["kind"]), _dev(e["value"]) if value else None, _dev(e["shift"]) if shift else None,
                        0.2, 0.5, normalize, out)


def _eq(got, want, what):
    """Bit for bit, NaNs in the same places."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = np.ascontiguousarray(want, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    u = np.uint32 if got.dtype == F else np.uint64
    bad = (np.ascontiguousarray(got).view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, int(bad.sum()), bad.size, np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _check(got, want, what):
    _eq(got.dhead, want["dhead"], (what, "dhead"))
    if want["dvalue"] is None:
        assert got.dvalue is None
    else:
        _eq(got.dvalue, want["dvalue"], (what, "dvalue"))
    _eq(got.dlog_std, want["dlog_std"], (what, "dlog_std"))
    assert got.stats.dtype == torch.float64
    _eq(got.stats, want["stats"], (what, "stats"))


# ---------------------------------------------------------------- 1. the device equals the twin at the segment and lane edges
SHAPES = [(2, 5, 5), (2, 63, 1), (2, 64, 1), (2, 65, 1), (2, 1024, 1), (2, 1025, 1), (1, 33, 3), (3, 33, 3)]


@pytest.mark.parametrize("parts", [(True, True, True), (False, False, False)], ids=["value-shift-norm", "bare"])
@pytest.mark.parametrize("A", [2, 1])
@pytest.mark.parametrize("B, n, sets", SHAPES, ids=lambda v: str(v))
def test_device_equals_the_twin(B, n, sets, A, parts):
    e = _inputs(100 + B + n + 7 * A, B, n, sets, A)
    want = _twin(e, *parts)
    got = _call(e, *parts)
    assert np.isfinite(want["stats"]).all() and (want["dhead"] != 0).any() and (want["dhead"] == 0).any()
    if n // sets > 4:
        assert (want["stats"][:, 6] > 0).any() and (want["stats"][:, 6] < 1).all()       # some rows clipped, not all
    _check(got, want, (B, n, sets, A, parts))


@pytest.mark.parametrize("parts", [(True, False, False), (False, True, True), (True, True, False), (False, False, True)],
                         ids=["value", "shift-norm", "value-shift", "norm"])
def test_every_optional_part_alone(parts):
    e = _inputs(41, 3, 33, 3, 2)
    _check(_call(e, *parts), _twin(e, *parts), parts)


# ---------------------------------------------------------------- 2. padded blocks; the raw entry point
def _raw(e, A, B, n, sets, pad, lo, hi, vf, normalize, value=True, sentinel=F(12345.678)):
    """``ftl_ppo_head`` itself on buffers whose blocks are ``pad`` elements longer than their rows: NaN in the inputs' padding, a sentinel
    in the outputs'.  Returns the outputs as numpy arrays with the padding, plus dlog_std and stats."""
    lib = _lib.load()
    keep = {}

    def block(name, a, width, dtype, fill):
        buf = torch.full((B, n * width + pad * width), fill, dtype=dtype, device=DEV)
        if a is not None:
            buf[:, :n * width] = _dev(a).view(B, -1)
        keep[name] = buf
        return buf.data_ptr(), (n + pad) * width * buf.element_size()

    a = abi.PpoHeadArgs()
    a.n_blocks, a.n, a.n_sets, a.width = B, n, sets, A
    a.head_new, a.head_new_block_bytes = block("head_new", e["head_new"], A, torch.float32, float("nan"))
    a.head_old, a.head_old_block_bytes = block("head_old", e["head_old"], A, torch.float32, float("nan"))
    a.noise, a.noise_block_bytes = block("noise", e["noise"], A, torch.float32, float("nan"))
    a.adv, a.adv_block_bytes = block("adv", e["adv"], 1, torch.float32, float("nan"))
    a.ret, a.ret_block_bytes = block("ret", e["ret"], 1, torch.float32, float("nan"))
    a.kind, a.kind_block_bytes = block("kind", e["kind"], 1, torch.uint8, 0)
    a.dhead, a.dhead_block_bytes = block("dhead", None, A, torch.float32, float(sentinel))
    if value:
        a.value_new, a.value_new_block_bytes = block("value", e["value"], 1, torch.float32, float("nan"))
        a.dvalue, a.dvalue_block_bytes = block("dvalue", None, 1, torch.float32, float(sentinel))
    for name in ("sigma_old", "sigma_new", "shift"):
        keep[name] = _dev(e[name])
    a.sigma_old, a.sigma_new, a.log_sigma_shift = keep["sigma_old"].data_ptr(), keep["sigma_new"].data_ptr(), keep["shift"].data_ptr()
    a.clip_lo, a.clip_hi, a.vf_coef, a.normalize = float(lo), float(hi), float(vf), normalize
    dls = torch.full((sets, A), float("nan"), dtype=torch.float32, device=DEV)
    stats = torch.full((sets, abi.FTL_PPO_STATS), float("nan"), dtype=torch.float64, device=DEV)
    need = lib.ftl_sizeof_ppo_head_workspace(B, n, sets)
    assert need == P.workspace_bytes(B, n, sets)
    ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=DEV)      # (the workspace needs no clearing)
    a.dlog_std, a.stats, a.workspace, a.workspace_bytes = dls.data_ptr(), stats.data_ptr(), ws.data_ptr(), need
    _lib.check(lib.ftl_ppo_head(mlp._device_handle(torch.device(DEV)), C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    torch.cuda.synchronize()
    return dict(dhead=keep["dhead"].cpu().numpy().reshape(B, n + pad, A), dvalue=keep["dvalue"].cpu().numpy() if value else None,
                dlog_std=dls.cpu().numpy(), stats=stats.cpu().numpy())


@pytest.mark.parametrize("A", [2, 1])
def test_padded_block_strides_keep_their_sentinels(A):
    B, n, sets, pad = 3, 33, 3, 5
    e = _inputs(77 + A, B, n, sets, A)
    sentinel = F(12345.678)
    got = _raw(e, A, B, n, sets, pad, LO, HI, F(0.5), 1, sentinel=sentinel)
    want = _twin(e)
    _eq(np.ascontiguousarray(got["dhead"][:, :n]), want["dhead"], "dhead")
    _eq(np.ascontiguousarray(got["dvalue"][:, :n]), want["dvalue"], "dvalue")
    _eq(got["dlog_std"], want["dlog_std"], "dlog_std")
    _eq(got["stats"], want["stats"], "stats")
    assert (got["dhead"][:, n:].view(np.uint32) == sentinel.view(np.uint32)).all() and (got["dvalue"][:, n:].view(np.uint32) == sentinel.view(np.uint32)).all()


# ---------------------------------------------------------------- 3. the crafted rows
@pytest.mark.parametrize("A", [2, 1])
def test_crafted_rows(A):
    cr = P.crafted(A)
    n = cr["adv"].size
    e = dict(head_new=cr["head_new"][None], head_old=cr["head_old"][None], noise=cr["noise"][None], adv=cr["adv"][None], ret=cr["ret"][None],
             value=cr["value"][None], kind=np.zeros((1, n), np.uint8), sigma_old=cr["sigma"], sigma_new=cr["sigma"], shift=np.zeros((1, A), F))
    r0 = _twin(e, normalize=False)["ratio"][0]
    lo, hi = r0[0], r0[1]                                                    # rows 0 and 1 sit exactly on the bounds
    want = _twin(e, normalize=False, lo=lo, hi=hi)
    r, g, cl = want["ratio"][0], want["dhead"][0, :, 0], want["rows"]["clipped"]
    assert r[0] == lo and r[1] == hi and not cl[0] and not cl[1] and g[0] != 0 and g[1] != 0
    assert r[2] > hi and r[3] < lo and cl[2:6].all() and g[2] == 0 and g[3] != 0 and g[4] != 0 and g[5] == 0
    assert g[6] == 0 and r[7] > 1 and np.isfinite(r[8]) and r[8] > 1e37 and 0 < r[9] < 1e-37
    assert abs(float(r[10]) - 1) <= 2 ** -22 and abs(float(r[11]) - 1) <= 2 ** -22
    assert want["rows"]["d"][8] > 86 and want["rows"]["d"][9] < -86
    got = _raw(e, A, 1, n, 1, 0, lo, hi, F(0.5), 0)
    _eq(got["dhead"], want["dhead"], "dhead")
    _eq(got["dvalue"], want["dvalue"], "dvalue")
    _eq(got["dlog_std"], want["dlog_std"], "dlog_std")
    _eq(got["stats"], want["stats"], "stats")


# ---------------------------------------------------------------- 4. empty sets, one-row sets, a NaN row
def test_a_set_of_void_rows_and_a_set_with_one_valid_row():
    B, n, sets, A = 3, 33, 3, 2
    e = _inputs(9, B, n, sets, A)
    e["kind"][:, 11:22] = VOID
    e["kind"][:, 22:] = VOID
    e["kind"][1, 25] = abi.FTL_TR_TERMINATED
    want, got = _twin(e), _call(e)
    _check(got, want, "void sets")
    st = got.stats.cpu().numpy()
    assert not st[1].any() and not np.signbit(st[1]).any()                   # count 0 and every mean +0.0
    assert not got.dhead[:, 11:22].any() and not got.dvalue[:, 11:22].any() and not got.dlog_std[1].any()
    assert st[2, 0] == 1 and st[2, 2] == 0 and not got.dhead[1, 25].any()    # one row: std 0, a = 0, no policy gradient ...
    assert got.dvalue[1, 25] != 0 and st[2, 4] > 0                           # ... but its value gradient, with 1 / count = 1
    bare = _call(e, value=False, shift=False, normalize=False)
    _check(bare, _twin(e, False, False, False), "void sets, bare")
    assert bare.dhead[1, 25].any()


def test_a_nan_row_stays_in_its_set():
    B, n, sets, A = 2, 33, 3, 2
    e = _inputs(19, B, n, sets, A)
    e["kind"][1, 15] = abi.FTL_TR_STEP
    clean = _call(e)
    e2 = dict(e, head_new=e["head_new"].copy())
    e2["head_new"][1, 15, 0] = np.nan
    want, got = _twin(e2), _call(e2)
    _check(got, want, "nan row")
    assert torch.isnan(got.dhead[1, 15]).all() and torch.isnan(got.dlog_std[1]).all() and torch.isnan(got.stats[1, [3, 5, 7]]).all()
    keep = torch.ones(B, n, dtype=torch.bool, device=DEV)
    keep[1, 15] = False
    assert torch.equal(got.dhead[keep].view(torch.int32), clean.dhead[keep].view(torch.int32))
    assert torch.equal(got.dvalue.view(torch.int32), clean.dvalue.view(torch.int32))
    for s in (0, 2):
        assert torch.equal(got.dlog_std[s].view(torch.int32), clean.dlog_std[s].view(torch.int32))
        assert torch.equal(got.stats[s].view(torch.int64), clean.stats[s].view(torch.int64))
    assert torch.equal(got.stats[1, :3].view(torch.int64), clean.stats[1, :3].view(torch.int64)) and not torch.isnan(got.stats[1, 6])


def test_overwrite_and_reproducibility():
    B, n, sets, A = 2, 1025, 1, 2
    e = _inputs(23, B, n, sets, A)
    nan = lambda *s, **k: torch.full(s, float("nan"), device=DEV, **k)
    out = mlp.PpoHead(nan(B, n, A), nan(B, n), nan(sets, A), nan(sets, 8, dtype=torch.float64))
    got = _call(e, out=out)
    assert got is out and all(bool(torch.isfinite(t).all()) for t in (out.dhead, out.dvalue, out.dlog_std, out.stats))    # every word overwritten
    again = _call(e)
    for k in ("dhead", "dvalue", "dlog_std", "stats"):
        assert torch.equal(getattr(out, k), getattr(again, k)), k


# ---------------------------------------------------------------- 5. ppo_loss under autograd on recorded trajectories
def _twin_of_loss(traj, head_new, log_std, log_std_old, adv, ret, value):
    c = lambda t: t.detach().cpu().numpy()
    return P.head(c(head_new), c(traj.head), c(traj.noise), c(traj.sigma), c(log_std.detach().exp()), c(adv), c(ret), c(traj.kind),
                  None if value is None else c(value), c(log_std.detach() - log_std_old), LO, HI, 0.5, True)


def test_ppo_loss_through_mlp_net_on_a_collected_trajectory():
    n, T, sets = 33, 5, 1
    env = _vec("B_s1_chase", n, over=SHORT)
    W0 = env.policy_obs.shape[1] * env.policy_obs.shape[2]
    rng = np.random.default_rng(15)
    wa, wc = (W0, 64, 64, 2), (W0, 64, 1)
    pa = (rng.standard_normal((sets, M.param_count(wa))) * 0.1).astype(F)
    pc = (rng.standard_normal((sets, M.param_count(wc))) * 0.1).astype(F)
    pol = mlp.MlpPolicy(env, wa, params=_dev(pa), n_sets=sets, activation="tanh")
    crit = mlp.Critic(wc, n_sets=sets, activation="tanh", params=_dev(pc))
    actor, critic = mlp.Net(wa, sets, "tanh", params=pol.params), mlp.Net(wc, sets, "tanh", params=crit.params)
    log_std = torch.nn.Parameter(torch.full((sets, 2), -1.0, device=DEV))
    noise = _dev(rng.standard_normal((T, n, 2)).astype(F))
    env.step(pol.act())
    with torch.no_grad():
        traj = env.collect_mlp(pol, T, noise, log_std.exp())
        adv, ret = mlp.gae(traj, crit.values(traj.obs), gamma=0.99, lam=0.95)
        log_std_old = log_std.detach().clone()
        pol.params.add_(_dev((rng.standard_normal(pa.shape) * 0.01).astype(F)))      # a few optimizer steps later
        log_std.add_(0.03)
    m = traj.valid
    assert bool((~m).any()) and bool(m.any())                                # VOID rows present
    obs = traj.obs[:-1].contiguous()
    head, value = actor(obs), critic(obs)
    loss = mlp.ppo_loss(traj, head, log_std, adv, ret, value, log_std_old)
    want = _twin_of_loss(traj, head, log_std, log_std_old, adv, ret, value[..., 0])
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad
    _eq(loss.stats, want["stats"], "stats")
    assert float(loss.detach()) == float(F(want["stats"][:, 7].sum())) and abs(float(want["stats"][0, 5])) > 1e-4      # the ratio has moved
    loss.backward()
    _eq(actor.params.grad, mlp.backward(wa, pol.params.detach(), obs, _dev(want["dhead"]), "tanh").cpu().numpy(), "actor")
    _eq(critic.params.grad, mlp.backward(wc, crit.params.detach(), obs, _dev(want["dvalue"][..., None]), "tanh").cpu().numpy(), "critic")
    _eq(log_std.grad, want["dlog_std"], "log_std")
    assert bool(actor.params.grad.any()) and bool(critic.params.grad.any()) and bool(log_std.grad.any())
    # default log_std_old is the record's sigma; no value part; a scaled loss scales the gradients
    actor.params.grad = None
    log_std.grad = None
    (2.0 * mlp.ppo_loss(traj, actor(obs), log_std, adv, ret)).backward()
    w2 = _twin_of_loss(traj, head, log_std, traj.sigma.log(), adv, ret, None)
    _eq(log_std.grad, (F(2.0) * w2["dlog_std"]).astype(F), "log_std, scaled")
    _eq(actor.params.grad, mlp.backward(wa, pol.params.detach(), obs, _dev((F(2.0) * w2["dhead"]).astype(F)), "tanh").cpu().numpy(), "actor, scaled")
    env.close()


def test_ppo_loss_through_rnn_net_on_a_collect_rnn_trajectory():
    n, T, sets, cell, A = 66, 12, 2, 33, 2
    env = _vec("B_s1_chase", n, over=SHORT)
    W0 = env.policy_obs.shape[1] * env.policy_obs.shape[2]
    wa, wc = (W0, 20, A), (W0, 16, 1)
    pol, pa = _rnn(env, wa, cell, sets, 502, nasty=False)
    pc = RS.params(602, sets, wc, cell, R.PREV_REWARD, nasty=False)
    crit = rnn.RecurrentCritic(wc, cell, n_sets=sets, params=_dev(pc))
    actor, value = rnn.Net(wa, cell, sets, params=pol.params), rnn.Net(wc, cell, sets, prev_action=False, params=crit.params)
    rng = np.random.default_rng(15)
    noise = _dev(rng.standard_normal((T, n, A)).astype(F))
    log_std = torch.nn.Parameter(_dev(np.array([[-1.0, -0.8], [-1.2, -0.9]], F)))
    env.step(pol.act())
    with torch.no_grad():
        r_in = env.reward.clone()
        v_state = torch.zeros(n, crit.S, device=DEV)
        traj = env.collect_rnn(pol, T, noise, log_std.exp())
        values, _ = crit.values(traj, v_state, r_in)
        adv, ret = mlp.gae(traj, values, gamma=0.99, lam=0.95)
        log_std_old = log_std.detach().clone()
        pol.params.add_(_dev((rng.standard_normal(pa.shape) * 0.01).astype(F)))
        log_std.add_(_dev(np.array([[0.02, -0.03], [-0.01, 0.04]], F)))
    m = traj.valid
    assert bool((~m).any()) and bool(m.any())
    y, v = actor(traj, reward0=r_in), value(traj, v_state, r_in)
    loss = mlp.ppo_loss(traj, y, log_std, adv, ret, v, log_std_old)
    want = _twin_of_loss(traj, y, log_std, log_std_old, adv, ret, v[..., 0])
    _eq(loss.stats, want["stats"], "stats")
    loss.backward()
    got_a, got_c = actor.params.grad.clone(), value.params.grad.clone()
    _eq(log_std.grad, want["dlog_std"], "log_std")
    assert not torch.equal(log_std.grad[0], log_std.grad[1])                 # every member its own
    actor.params.grad = None
    value.params.grad = None
    actor(traj, reward0=r_in).backward(_dev(want["dhead"]))                  # rnn.backward of the twin's dhead
    value(traj, v_state, r_in).backward(_dev(want["dvalue"][..., None]))
    assert bool(got_a.any()) and bool(got_c.any())
    assert torch.equal(got_a.view(torch.int32), actor.params.grad.view(torch.int32))
    assert torch.equal(got_c.view(torch.int32), value.params.grad.view(torch.int32))
    env.close()


# ---------------------------------------------------------------- 6. the wrapper's refusals on device tensors
def test_wrapper_refuses_on_device_tensors():
    T, n, A, sets = 3, 6, 2, 2
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    good = dict(head=z(T, n, A), head_old=z(T, n, A), noise=z(T, n, A), sigma_old=torch.ones(sets, A, device=DEV), sigma=torch.ones(sets, A, device=DEV),
                adv=z(T, n), ret=z(T, n), kind=z(T, n, dtype=torch.uint8), value=z(T, n))
    bad = [dict(head_old=good["head_old"].cpu()), dict(noise=z(T, n, 1)), dict(sigma=torch.ones(4, A, device=DEV)), dict(sigma_old=good["sigma_old"].cpu()),
           dict(adv=z(T, n).double()), dict(kind=z(T, n)), dict(value=z(T, n, 1)), dict(head=z(T, n, 2 * A)[:, :, ::2]),
           dict(head=z(T, n, A, requires_grad=True)), dict(clip=-1.0), dict(log_sigma_shift=z(sets, A).cpu()), dict(out=3)]
    for over in bad:
        with pytest.raises(ValueError):
            mlp.ppo_head(**dict(good, **over))
    with pytest.raises(NotImplementedError):
        mlp.ppo_head(**dict(good, head=z(T, n, 5), head_old=z(T, n, 5), noise=z(T, n, 5)))
    r = mlp.ppo_head(**good)
    assert tuple(r.dhead.shape) == (T, n, A) and tuple(r.dvalue.shape) == (T, n) and tuple(r.dlog_std.shape) == (sets, A) and tuple(r.stats.shape) == (sets, 8)
    assert float(r.stats[:, 0].sum()) == T * n and not r.dhead.any()         # zero advantages: a = 0 everywhere
