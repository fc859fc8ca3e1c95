"""GPU tests of the forward pass on caller-supplied rows (include/ftl.h: ``ftl_mlp_forward``; ``mlp.forward``, ``MlpPolicy.forward``,
``mlp.Critic``): the raw heads against the numpy twin (tests/mlp_tanh_numpy.py: ``population_raw``, per block) bit for bit -- over tile,
set, k-chunk and head-width edges, at the limits of a net, on the constructed rows that carry ties, subnormals and the edges of tanh32
to the head --, block strides and part views with untouched padding, the replay of a recorded trajectory's heads, a critic's values
into ``gae`` and the wrapper's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import collect_numpy as CN
import mlp_numpy as M
import mlp_tanh_numpy as MT
from continiousenvironment_follower_leader_amd import _lib, abi, mlp
from test_gpu_collect import SHORT, _sigma
from test_gpu_mlp import DEV, _vec

pytestmark = pytest.mark.gpu

NETS = [(7, 1), (180, 64, 64, 1), (65, 17, 3), (33, 16, 31, 5), (20, 255, 256)]
ACTS = ("relu", "tanh")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _twin(p, widths, x, eps, activation, env_first=0, **kw):
    """``population_raw`` of every block of ``x`` [..., n, w0]: row r of a block under set (env_first + r) // eps."""
    flat = x.reshape((-1,) + x.shape[-2:])
    y = np.stack([MT.population_raw(p, widths, b, eps, env_first, activation=activation, **kw) for b in flat])
    return y.reshape(x.shape[:-1] + (widths[-1],))


def _call(widths, params, n_sets, eps, env_first, activation, n_blocks, n, x_ptr, xb, y_ptr, yb):
    """``ftl_mlp_forward`` itself, with strides and a first row of the caller's choice, on the current stream."""
    net = abi.Mlp()
    net.params, net.set_stride, net.n_sets, net.n_layers = params.data_ptr(), abi.mlp_param_count(widths), n_sets, len(widths) - 1
    for l, w in enumerate(widths):
        net.width[l] = w
    net.env_first, net.envs_per_set, net.activation = env_first, eps, mlp.ACTIVATIONS[activation]
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(lib.ftl_mlp_forward(mlp._device_handle(torch.device(DEV)), C.byref(net), n_blocks, n, x_ptr, xb, y_ptr, yb, stream), lib)


# ---------------------------------------------------------------- 1. against the twin
@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("n, n_sets", [(33, 3), (15, 1)])
def test_forward_equals_the_twin(n, n_sets, blocks):
    for i, widths in enumerate(NETS):
        rng = np.random.default_rng(100 * n + 10 * blocks + i)
        p = M.nasty_params(rng, n_sets, widths, 0.1)
        x = M.nasty_inputs(rng, blocks * n, widths[0]).reshape((blocks, n, widths[0]) if blocks > 1 else (n, widths[0]))
        got = {}
        for act in ACTS:
            y = mlp.forward(widths, _dev(p), _dev(x), act)
            assert y.dtype == torch.float32 and tuple(y.shape) == x.shape[:-1] + (widths[-1],) and y.is_contiguous()
            got[act] = y.cpu().numpy()
            want = _twin(p, widths, x, n // n_sets, act)
            assert np.array_equal(_bits(got[act]), _bits(want)), (widths, act, int((_bits(got[act]) != _bits(want)).sum()))
        same = np.array_equal(_bits(got["relu"]), _bits(got["tanh"]))
        assert same == (len(widths) == 2), widths                       # the activation reaches the head wherever a hidden layer exists
        if len(widths) > 2:
            assert (_bits(got["relu"]) != _bits(got["tanh"])).any(-1).mean() > 0.9


# ---------------------------------------------------------------- 2. the limits of a net
def test_forward_at_the_limits():
    widths, n = (4096, 256, 256, 256, 256), 2
    rng = np.random.default_rng(7)
    p, x = M.nasty_params(rng, 1, widths, 0.02), M.nasty_inputs(rng, n, widths[0])
    pd, xd = _dev(p), _dev(x)
    for act in ACTS:
        got = mlp.forward(widths, pd, xd, act).cpu().numpy()
        want = _twin(p, widths, x, n, act)
        assert got.shape == (n, 256) and np.array_equal(_bits(got), _bits(want)), (act, int((_bits(got) != _bits(want)).sum()))
        assert len(np.unique(want)) > 256                                # not a saturated or dead head


# ---------------------------------------------------------------- 3. arithmetic edges
@pytest.mark.parametrize("case, wrong", [(M.tie_case, M.fma_f64sum), (M.subnormal_case, M.fma_flush)], ids=["tie", "subnormal"])
def test_forward_keeps_ties_and_subnormals(case, wrong):
    """The constructed ReLU nets of tests/mlp_numpy.py: raw heads that change when a product is rounded twice at a tie, or when a float32
    subnormal is flushed.  The twin re-run with that wrong arithmetic differs in every set; the device equals the exact twin."""
    widths, p, x = case(180)
    exact = _twin(p, widths, x, M.ROWS, "relu")
    bad = _twin(p, widths, x, M.ROWS, "relu", fma=wrong)
    differ = (_bits(exact) != _bits(bad)).any(1).reshape(4, M.ROWS).sum(1)
    assert (differ >= M.ROWS - 1).all(), differ
    got = mlp.forward(widths, _dev(p), _dev(x), "relu").cpu().numpy()
    print("device vs exact twin: %d of %d heads differ; vs the wrong arithmetic: %d" % ((_bits(got) != _bits(exact)).sum(), got.size, (_bits(got) != _bits(bad)).sum()))
    assert np.array_equal(_bits(got), _bits(exact)), np.argwhere(_bits(got) != _bits(exact))[:8]


def test_forward_keeps_the_edges_of_tanh32():
    """The constructed tanh nets of tests/mlp_tanh_numpy.py (edge_case): heads 0.5 * tanh32(+-v) for v in the cancellation range, on both
    sides of the first exact 1, at the rintf ties of the exponent split, at 1e30 and infinity, a NaN row, and a set whose every value is
    -0.  The twin re-run with a float64 ``np.tanh`` changes them in every class in which two float32 tanh can differ; the device equals
    the exact twin."""
    widths, p, x, classes = MT.edge_case(180)
    rows, cls = len(classes), np.array(classes)
    exact = _twin(p, widths, x, rows, "tanh")
    wrong = _twin(p, widths, x, rows, MT.tanh_f64)
    differ = (_bits(exact[:rows]) != _bits(wrong[:rows])).all(1)
    for c in ("tiny", "one", "tie"):
        assert differ[cls == c].any(), c
    assert (_bits(exact[rows:]) == 0x80000000).all()                     # -0 stays -0
    finite = ~np.isnan(exact).any(1)
    assert (~finite).sum() == 1
    got = mlp.forward(widths, _dev(p), _dev(x), "tanh").cpu().numpy()
    print("device vs exact twin: %d of %d heads differ; vs the float64 tanh: %d" % ((_bits(got[finite]) != _bits(exact[finite])).sum(), got[finite].size,
                                                                                  (_bits(got[finite]) != _bits(wrong[finite])).sum()))
    assert np.array_equal(_bits(got[finite]), _bits(exact[finite])), np.argwhere(_bits(got) != _bits(exact))[:8]
    assert np.isnan(got[~finite]).all()
    relu = mlp.forward(widths, _dev(p), _dev(x), "relu").cpu().numpy()
    assert (_bits(relu[rows:]) == 0).all()                               # ... only where the activation keeps the sign


# ---------------------------------------------------------------- 4. strides and part views
@pytest.mark.parametrize("lo, n", [(7, 21), (24, 16)])
def test_forward_on_part_views_with_padded_blocks(lo, n):
    """Rows [lo, lo + n) of a [3, 40, W0] tensor with env_first = lo under sets of 16 rows (the part begins inside a set and crosses
    into the next one), written into a sentinel-filled buffer whose blocks are padded: the rows equal those of the whole-tensor call, and
    no other float of the buffer changes."""
    widths, B, N, eps, sets = (33, 16, 31, 5), 3, 40, 16, 3
    W0, A = widths[0], widths[-1]
    assert lo // eps != (lo + n - 1) // eps and lo % eps != 0 and lo + n <= N
    rng = np.random.default_rng(lo)
    p, x = M.nasty_params(rng, sets, widths, 0.1), M.nasty_inputs(rng, B * N, W0).reshape(B, N, W0)
    pd, xd = _dev(p), _dev(x)
    for act in ACTS:
        whole = torch.empty(B, N, A, dtype=torch.float32, device=DEV)
        _call(widths, pd, sets, eps, 0, act, B, N, xd.data_ptr(), N * W0 * 4, whole.data_ptr(), N * A * 4)
        want = _twin(p, widths, x, eps, act)
        assert np.array_equal(_bits(whole.cpu().numpy()), _bits(want)), act
        pad, sentinel = 3, np.float32(12345.678)
        buf = torch.full((B + 1, N * A + pad), float(sentinel), dtype=torch.float32, device=DEV)
        stride = (N * A + pad) * 4
        _call(widths, pd, sets, eps, lo, act, B, n, xd.data_ptr() + lo * W0 * 4, N * W0 * 4, buf.data_ptr() + lo * A * 4, stride)
        got = buf.cpu().numpy()
        rows = got[:B, :N * A].reshape(B, N, A)
        assert np.array_equal(_bits(rows[:, lo:lo + n]), _bits(want[:, lo:lo + n])), (act, lo)
        untouched = np.ones(got.shape, bool)
        untouched[:B, lo * A:(lo + n) * A] = False
        assert (_bits(got[untouched]) == _bits(sentinel)).all(), (act, lo, int((_bits(got[untouched]) != _bits(sentinel)).sum()))
        assert untouched.sum() == got.size - B * n * A


# ---------------------------------------------------------------- 5. replay equals the record
def _collected(act, cls=None, n=33, sets=3, T=5, seed=500, **kw):
    env = _vec("B_s1_chase", n, cls=cls, over=SHORT, **kw)
    widths = (180, 70, 33, 2)
    p = (np.random.default_rng(seed).standard_normal((sets, M.param_count(widths))) * 0.1).astype(np.float32)
    pol = mlp.MlpPolicy(env, widths, params=_dev(p), n_sets=sets, activation=act)
    noise = _dev(np.random.default_rng(seed + 1).standard_normal((T, n, 2)).astype(np.float32))
    sigma = _dev(_sigma(seed + 2, sets, 2))
    env.step(pol.act())                                            # the first episode of the window is one step short: it ends inside it
    tr = pol.collect(T, noise, sigma)
    return env, pol, p, tr


@pytest.mark.parametrize("act", ACTS)
def test_replay_equals_the_recorded_head(act):
    env, pol, p, tr = _collected(act)
    kind = tr.kind.cpu().numpy()
    for k in (abi.FTL_TR_STEP, abi.FTL_TR_TRUNCATED, abi.FTL_TR_VOID):
        assert (kind == k).any(), k                                # VOID rows too: the sample kernel records every env
    head = pol.forward(tr.obs[:-1])
    assert tuple(head.shape) == tuple(tr.head.shape) and head.dtype == torch.float32
    assert torch.equal(head.view(torch.int32), tr.head.view(torch.int32)), int((head.view(torch.int32) != tr.head.view(torch.int32)).sum())
    assert len(torch.unique(tr.head)) > tr.head.numel() // 2       # a record worth replaying
    buf = torch.full_like(tr.head, 7.0)
    assert pol.forward(tr.obs[:-1], out=buf) is buf and torch.equal(buf.view(torch.int32), tr.head.view(torch.int32))
    one = pol.forward(tr.obs[2])                                   # a single block: no leading axis
    assert tuple(one.shape) == (33, 2) and torch.equal(one.view(torch.int32), tr.head[2].view(torch.int32))
    other = mlp.forward(pol.widths, pol.params, tr.obs[:-1], "relu" if act == "tanh" else "tanh")
    assert not torch.equal(other, tr.head)
    env.close()


def test_replay_on_a_pipelined_batch_after_join():
    from continiousenvironment_follower_leader_amd.vec_game import PipelinedVecGame
    n, sets = 1045, 5
    env, pol, p, tr = _collected("tanh", cls=PipelinedVecGame, n=n, sets=sets, T=4, seed=700, parts=2)
    lo1 = env.shards[1].lo
    assert lo1 % (n // sets) != 0                                  # a set lies in both parts
    env.join()
    head = pol.forward(tr.obs[:-1])
    assert torch.equal(head.view(torch.int32), tr.head.view(torch.int32))
    env.close()


# ---------------------------------------------------------------- 6. a critic's values into gae
def test_critic_values_feed_gae():
    env, pol, _, tr = _collected("relu")
    widths, sets = (180, 64, 1), 3
    p = (np.random.default_rng(900).standard_normal((sets, M.param_count(widths))) * 0.1).astype(np.float32)
    crit = mlp.Critic(widths, n_sets=sets, params=_dev(p))
    assert crit.activation == "tanh" and crit.device == tr.obs.device
    values = crit.values(tr.obs)
    T, N = tr.reward.shape
    assert tuple(values.shape) == (T + 1, N) and values.dtype == torch.float32
    obs = tr.obs.cpu().numpy()
    want_v = _twin(p, widths, obs, N // sets, "tanh")[..., 0]
    assert np.array_equal(_bits(values.cpu().numpy()), _bits(want_v))
    assert len(np.unique(want_v)) > want_v.size // 2
    adv, ret = mlp.gae(tr, values, 0.99, 0.95)
    want_adv, want_ret = CN.gae(tr.reward.cpu().numpy(), tr.kind.cpu().numpy(), want_v, 0.99, 0.95)
    assert np.array_equal(_bits(adv.cpu().numpy()), _bits(want_adv)) and np.array_equal(_bits(ret.cpu().numpy()), _bits(want_ret))
    buf = torch.full((T + 1, N), 7.0, dtype=torch.float32, device=DEV)
    again = crit.values(tr.obs, out=buf)
    assert again.data_ptr() == buf.data_ptr() and torch.equal(buf.view(torch.int32), values.view(torch.int32))
    # a module loaded into one set changes that set's rows only
    module = mlp.torch_module(widths, "tanh")
    crit.load(module, 1)
    v2 = crit.values(tr.obs)
    eps = N // sets
    assert torch.equal(v2[:, :eps], values[:, :eps]) and torch.equal(v2[:, 2 * eps:], values[:, 2 * eps:]) and not torch.equal(v2[:, eps:2 * eps], values[:, eps:2 * eps])
    row = mlp.params_from_torch(module)[2].numpy()
    assert np.array_equal(_bits(v2[:, eps:2 * eps].cpu().numpy()), _bits(_twin(row[None], widths, obs[:, eps:2 * eps], eps, "tanh")[..., 0]))
    env.close()


# ---------------------------------------------------------------- 7. refusals on the device
def test_forward_refusals_on_the_device():
    widths = (5, 4, 3)
    count = abi.mlp_param_count(widths)
    params, x = torch.zeros(2, count, device=DEV), torch.zeros(3, 6, 5, device=DEV)
    assert tuple(mlp.forward(widths, params, x).shape) == (3, 6, 3)
    for kw in (dict(x=torch.zeros(3, 5, 6, device=DEV).transpose(1, 2)), dict(x=torch.zeros(3, 12, 5, device=DEV)[:, ::2]),
               dict(x=torch.zeros(3, 6, 5, dtype=torch.float64, device=DEV)), dict(x=torch.zeros(3, 6, 5, dtype=torch.float16, device=DEV)),
               dict(x=torch.zeros(3, 7, 5, device=DEV)), dict(params=torch.zeros(4, count, device=DEV)),
               dict(out=torch.zeros(3, 6, 4, device=DEV)), dict(out=torch.zeros(18, 3, device=DEV)), dict(out=torch.zeros(3, 6, 3)),
               dict(x=torch.zeros(3, 6, 5)), dict(params=torch.zeros(2, count))):
        with pytest.raises(ValueError):
            mlp.forward(**dict(dict(widths=widths, params=params, x=x), **kw))
    crit = mlp.Critic((5, 4, 1), n_sets=2, device=DEV)
    assert crit.params.is_cuda and tuple(crit.values(x).shape) == (3, 6) and not crit.values(x).any()
    with pytest.raises(ValueError):
        crit.values(x, out=torch.zeros(3, 6, 1, device=DEV))
    with pytest.raises(ValueError):
        crit.values(torch.zeros(3, 7, 5, device=DEV))
