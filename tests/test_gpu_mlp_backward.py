"""GPU checks of the backward pass of the MLP population (include/ftl.h: ``ftl_mlp_backward``; ``mlp.backward``, ``mlp.Net``): the
device against the twin (tests/mlp_backward_numpy.py) bit for bit -- cut tiles, several blocks, every path of the kernel's chunking,
more than two spans --, set independence, padded blocks and ``env_first``, the derivative's edges, overwrite, reproducibility, ``mlp.Net``
under autograd and Adam, the PPO loss of INTEGRATION.md on a recorded trajectory, and the wrapper's refusals on device tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_backward_numpy as MB
import mlp_numpy as M
import test_mlp_backward_abi as BA
from continiousenvironment_follower_leader_amd import _lib, abi, mlp
from test_gpu_collect import SHORT
from test_gpu_mlp import DEV, _vec

pytestmark = pytest.mark.gpu
F = np.float32
ACTS = ("relu", "tanh")
NETS = [(7, 1), (180, 64, 64, 1), (65, 17, 3), (33, 16, 31, 5), (20, 255, 256), (180, 256, 256, 2)]
_ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _case(widths, B, n, sets, seed, scale=0.3):
    """(params [sets, count], x [B, n, W0], dy [B, n, WL]): normal weights, the forward tests' inputs, normal dy with rows of zeros."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((sets, M.param_count(widths))) * scale).astype(F)
    x = M.nasty_inputs(rng, B * n, widths[0]).reshape(B, n, widths[0])
    dy = rng.standard_normal((B, n, widths[-1])).astype(F)
    dy[rng.random((B, n)) < 0.2] = 0.0
    return p, x, dy


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), bad.size, float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64)))))


# ---------------------------------------------------------------- 1. the device equals the twin
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n, sets", [(33, 3), (15, 1)])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("widths", NETS, ids=_ids)
def test_gradient_equals_the_twin(widths, act, n, sets, B):
    p, x, dy = _case(widths, B, n, sets, 1000 + 7 * len(widths) + widths[1] + n + B)
    got = mlp.backward(widths, _dev(p), _dev(x), _dev(dy), act)
    assert tuple(got.shape) == p.shape and got.dtype == torch.float32
    want = MB.population_grad(p, widths, x, dy, n // sets, activation=act)
    assert np.isfinite(want).all() and (want != 0).mean() > 0.2
    _same(got, want, (widths, act, n, B))


@pytest.mark.parametrize("act", ACTS)
def test_more_than_two_spans_with_a_cut_last_span(act):
    widths, rows = (33, 16, 31, 5), 40
    B = (2 * abi.FTL_MLP_BWD_SPAN + 12) // 2                  # two tiles a block (32 + 8 rows): 2 whole spans and 12 tiles of a third
    assert B == 70 or abi.FTL_MLP_BWD_SPAN != 64
    p, x, dy = _case(widths, B, rows, 1, 77)
    assert MB.workspace_bytes(widths, B, rows, rows) == 3 * M.param_count(widths) * 4
    got = mlp.backward(widths, _dev(p), _dev(x), _dev(dy), act)
    _same(got, MB.population_grad(p, widths, x, dy, rows, activation=act), act)


# ---------------------------------------------------------------- 2. a set's gradient is its rows' alone
@pytest.mark.parametrize("act", ACTS)
def test_middle_set_equals_its_rows_alone(act):
    widths = (65, 17, 3)
    p, x, dy = _case(widths, 3, 33, 3, 5)
    pd, xd, dyd = _dev(p), _dev(x), _dev(dy)
    whole = mlp.backward(widths, pd, xd, dyd, act)
    alone = mlp.backward(widths, pd[1:2].contiguous(), xd[:, 11:22].contiguous(), dyd[:, 11:22].contiguous(), act)
    assert torch.equal(whole[1].view(torch.int32), alone[0].view(torch.int32))
    assert not torch.equal(whole[0], whole[1]) and whole[1].abs().sum() > 0


# ---------------------------------------------------------------- 3. padded blocks, env_first, untouched sets
def _raw(widths, pd, sets, eps, env_first, act, B, n, x_ptr, xb, dy_ptr, dyb, grad, stride=None):
    lib = _lib.load()
    net = abi.Mlp()
    net.params, net.set_stride, net.n_sets, net.n_layers = pd.data_ptr(), stride or M.param_count(widths), sets, len(widths) - 1
    for l, w in enumerate(widths):
        net.width[l] = w
    net.env_first, net.envs_per_set, net.activation = env_first, eps, mlp.ACTIVATIONS[act]
    need = lib.ftl_sizeof_mlp_backward_workspace(C.byref(net), B, n)
    assert need == MB.workspace_bytes(widths, B, n, eps, env_first)
    ws = torch.empty(need // 4, dtype=torch.float32, device=DEV)
    _lib.check(lib.ftl_mlp_backward(mlp._device_handle(torch.device(DEV)), C.byref(net), B, n, x_ptr, xb, dy_ptr, dyb, grad.data_ptr(),
                                    ws.data_ptr(), need, C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    torch.cuda.synchronize()


@pytest.mark.parametrize("act", ACTS)
def test_rows_of_a_padded_tensor_and_env_first(act):
    widths, B, N, sets, eps = (65, 17, 3), 3, 40, 4, 10
    W0, A, count = widths[0], widths[-1], M.param_count(widths)
    p, x, dy = _case(widths, B, N, sets, 31)
    pd = _dev(p)
    sentinel = F(12345.678)
    for lo, n in ((13, 21), (10, 10), (0, 40), (25, 6)):          # sets 1 .. 3 (the first and last cut), set 1 alone, all, set 2 cut twice
        xs, dys = np.ascontiguousarray(x[:, lo:lo + n]), np.ascontiguousarray(dy[:, lo:lo + n])
        want = MB.population_grad(p, widths, xs, dys, eps, env_first=lo, activation=act, fill=sentinel)
        # the contiguous call
        grad = torch.full((sets, count), float(sentinel), dtype=torch.float32, device=DEV)
        xd, dyd = _dev(xs), _dev(dys)
        _raw(widths, pd, sets, eps, lo, act, B, n, xd.data_ptr(), n * W0 * 4, dyd.data_ptr(), n * A * 4, grad)
        _same(grad, want, (act, lo, n, "contiguous"))
        # rows [lo, lo + n) of the [B, N, .] tensors with padded block strides
        pad = 3
        xbuf = torch.zeros(B, N * W0 + pad, dtype=torch.float32, device=DEV)
        dybuf = torch.full((B, N * A + pad), float("nan"), dtype=torch.float32, device=DEV)
        xbuf[:, :N * W0] = _dev(x).view(B, -1)
        dybuf[:, :N * A] = _dev(dy).view(B, -1)
        grad2 = torch.full((sets, count), float(sentinel), dtype=torch.float32, device=DEV)
        _raw(widths, pd, sets, eps, lo, act, B, n, xbuf.data_ptr() + lo * W0 * 4, (N * W0 + pad) * 4,
             dybuf.data_ptr() + lo * A * 4, (N * A + pad) * 4, grad2)
        assert torch.equal(grad.view(torch.int32), grad2.view(torch.int32)), (act, lo, n)
        touched = np.unique((lo + np.arange(n)) // eps)
        for s in range(sets):
            if s not in touched:
                assert (_bits(grad2[s].cpu().numpy()) == _bits(sentinel)).all(), (act, lo, n, s)
    # a set stride beyond the parameter count: the padding keeps the sentinel
    stride = count + 5
    pp = torch.zeros(sets, stride, dtype=torch.float32, device=DEV)
    pp[:, :count] = pd
    grad = torch.full((sets, stride), float(sentinel), dtype=torch.float32, device=DEV)
    xd, dyd = _dev(x), _dev(dy)
    _raw(widths, pp, sets, eps, 0, act, B, N, xd.data_ptr(), N * W0 * 4, dyd.data_ptr(), N * A * 4, grad, stride=stride)
    _same(grad[:, :count].contiguous(), MB.population_grad(p, widths, x, dy, eps, activation=act), (act, "stride"))
    assert (_bits(grad[:, count:].cpu().numpy()) == _bits(sentinel)).all()


# ---------------------------------------------------------------- 4. the derivative at its edges
def test_relu_derivative_at_zero_minus_zero_and_subnormals():
    widths, p, x, dy, classes = BA.relu_edge_case()
    want = MB.population_grad(p, widths, x[None], dy[None], x.shape[0], activation="relu")
    wrong = MB.population_grad(p, widths, x[None], dy[None], x.shape[0], activation="relu", relu_ge=True)
    assert not np.array_equal(_bits(want), _bits(wrong))                  # the rows reach acc == 0: the case discriminates
    _same(mlp.backward(widths, _dev(p), _dev(x[None]), _dev(dy[None]), "relu"), want, classes)


def test_tanh_derivative_one_rounding_and_saturation():
    widths, p, x, dy = BA.tanh_edge_case()
    want = MB.population_grad(p, widths, x[None], dy[None], x.shape[0], activation="tanh")
    wrong = MB.population_grad(p, widths, x[None], dy[None], x.shape[0], activation="tanh", tanh_two_roundings=True)
    assert not np.array_equal(_bits(want), _bits(wrong))
    _same(mlp.backward(widths, _dev(p), _dev(x[None]), _dev(dy[None]), "tanh"), want, "tanh edges")


# ---------------------------------------------------------------- 5. overwrite, zero rows, reproducibility
@pytest.mark.parametrize("act", ACTS)
def test_overwrite_zero_rows_and_reproducibility(act):
    widths = (180, 64, 64, 1)
    p, x, dy = _case(widths, 3, 33, 3, 91)
    pd, xd = _dev(p), _dev(x)
    out = torch.full(p.shape, float("nan"), dtype=torch.float32, device=DEV)
    got = mlp.backward(widths, pd, xd, _dev(dy), act, out=out)
    assert got is out and torch.isfinite(out).all()                        # every word overwritten
    again = mlp.backward(widths, pd, xd, _dev(dy), act)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    # rows with dy = 0 contribute nothing: other inputs there, the same gradient (up to the sign of a zero sum)
    zero = (dy == 0).all(-1)
    assert zero.any()
    x2 = x.copy()
    x2[zero] = np.random.default_rng(4).random((int(zero.sum()), widths[0]), dtype=F) * 3
    other = mlp.backward(widths, pd, _dev(x2), _dev(dy), act)
    assert torch.equal(out, other)
    nothing = mlp.backward(widths, pd, xd, torch.zeros_like(_dev(dy)), act, out=torch.full_like(out, float("nan")))
    assert (nothing == 0).all()


# ---------------------------------------------------------------- 6. mlp.Net under autograd
@pytest.mark.parametrize("act", ACTS)
def test_net_under_autograd_and_one_adam_step(act):
    widths, sets, B, n = (20, 64, 64, 2), 2, 3, 24
    p, x, dy = _case(widths, B, n, sets, 61, scale=0.3)
    xd, dyd = _dev(x), _dev(dy)
    net = mlp.Net(widths, n_sets=sets, activation=act, params=_dev(p))
    assert isinstance(net, torch.nn.Module) and [tuple(q.shape) for q in net.parameters()] == [p.shape]
    y = net(xd)
    assert y.requires_grad and torch.equal(y, mlp.forward(widths, _dev(p), xd, act))
    y.backward(dyd)
    want = mlp.backward(widths, _dev(p), xd, dyd, act)
    assert torch.equal(net.params.grad.view(torch.int32), want.view(torch.int32))
    net(xd).backward(dyd)                                                  # a second backward accumulates
    assert torch.equal(net.params.grad, want + want)
    with pytest.raises(ValueError, match="grad"):
        net(xd.clone().requires_grad_())
    with pytest.raises(ValueError, match="backward"):
        mlp.forward(widths, net.params, xd, act)                           # forward() itself keeps refusing
    # shared storage: what the optimizer writes is what forward() reads
    shared = _dev(p)
    net = mlp.Net(widths, n_sets=sets, activation=act, params=shared)
    assert net.params.data_ptr() == shared.data_ptr()
    lr = 1e-3
    opt = torch.optim.Adam(net.parameters(), lr, eps=1.0)                  # eps = 1: the update lr * g / (|g| + 1) is 1-Lipschitz in g
    (net(xd) * dyd).sum().backward()
    opt.step()
    assert not torch.equal(shared, _dev(p))
    for s in range(sets):
        rows = slice(s * (n // sets), (s + 1) * (n // sets))
        g64, bound = BA.f64_grad_and_bound(p[s], widths, x[:, rows], dy[:, rows], act)[1:]
        mod = mlp.torch_module(widths, act, torch.from_numpy(p[s])).double()
        o = torch.optim.Adam(mod.parameters(), lr, eps=1.0)
        (mod(torch.from_numpy(x[:, rows]).double()) * torch.from_numpy(dy[:, rows]).double()).sum().backward()
        o.step()
        after = torch.cat([torch.cat([lin.weight.detach().t().reshape(-1), lin.bias.detach()]) for lin in mod[::2]]).numpy()
        diff = np.abs(shared[s].cpu().numpy().astype(np.float64) - after)
        # lr * bound: the update is 1-Lipschitz in the gradient; the rest is float32 itself: Adam's own arithmetic on the device (under ten
        # roundings of an update of at most lr) and the rounding of the stored parameter
        allow = lr * bound + 10 * BA.U32 * lr + BA.U32 * np.abs(after)
        print("%s set %d: max |net - torch64| after one Adam step %.3e, allowed there %.3e" % (act, s, diff.max(), allow[diff.argmax()]))
        assert (diff <= allow).all(), (act, s, float((diff - allow).max()))


# ---------------------------------------------------------------- 7. the PPO loss of INTEGRATION.md on a recorded trajectory
def test_ppo_loss_on_a_trajectory_with_void_rows():
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
    log_std = torch.full((1, 2), -1.0, device=DEV)
    noise = _dev(rng.standard_normal((T, n, 2)).astype(F))
    env.step(pol.act())
    with torch.no_grad():
        traj = env.collect_mlp(pol, T, noise, log_std.exp())
        adv, ret = mlp.gae(traj, crit.values(traj.obs), gamma=0.99, lam=0.95)
        sigma_old = traj.sigma
        logp_old = (-0.5 * noise ** 2 - sigma_old.log() - 0.9189385332).sum(-1)
        z = traj.head + sigma_old * noise
        m = traj.valid
    assert (~m).any() and m.any()                                          # VOID rows present
    obs = traj.obs[:-1].contiguous()

    def loss_of(actor_out, critic_out, dt):
        sigma = log_std.exp().to(dt)
        logp = (-0.5 * ((z.to(dt) - actor_out) / sigma) ** 2 - sigma.log() - 0.9189385332).sum(-1)
        ratio = (logp - logp_old.to(dt)).exp()
        a = ((adv - adv[m].mean()) / (adv[m].std() + 1e-8)).to(dt)
        return (-torch.min(ratio * a, ratio.clamp(0.8, 1.2) * a) + 0.5 * (critic_out.squeeze(-1) - ret.to(dt)) ** 2)[m].mean()

    loss_of(actor(obs), critic(obs), torch.float32).backward()
    ga, gc = actor.params.grad, critic.params.grad
    assert torch.isfinite(ga).all() and torch.isfinite(gc).all()
    for grad, widths, p in ((ga, wa, pa), (gc, wc, pc)):
        mod = mlp.torch_module(widths, "tanh", torch.from_numpy(p[0])).double().to(DEV)
        other = mlp.torch_module(wc if widths is wa else wa, "tanh", torch.from_numpy((pc if widths is wa else pa)[0])).double().to(DEV)
        a_out, c_out = (mod(obs.double()), other(obs.double())) if widths is wa else (other(obs.double()), mod(obs.double()))
        loss_of(a_out, c_out, torch.float64).backward()
        g64 = torch.cat([torch.cat([lin.weight.grad.t().reshape(-1), lin.bias.grad]) for lin in mod[::2]])
        clear = g64.abs() > 1e-4 * g64.abs().max()
        assert clear.sum() > g64.numel() // 4
        assert (grad[0][clear] != 0).all()
        assert torch.allclose(grad[0].double(), g64, rtol=1e-3, atol=1e-4 * float(g64.abs().max()))
    env.close()


# ---------------------------------------------------------------- 8. the wrapper's refusals on device tensors
def test_wrapper_refuses_on_device_tensors():
    widths = (5, 4, 3)
    count = abi.mlp_param_count(widths)
    params, x, dy = torch.zeros(2, count, device=DEV), torch.zeros(3, 6, 5, device=DEV), torch.zeros(3, 6, 3, device=DEV)
    bad = [dict(params=params.cpu()), dict(dy=dy.cpu()), dict(dy=torch.zeros(3, 6, 4, device=DEV)), dict(dy=dy.double()),
           dict(dy=dy.clone().requires_grad_()), dict(x=x.clone().requires_grad_()), dict(x=torch.zeros(3, 7, 5, device=DEV)),
           dict(out=torch.zeros(2, count + 1, device=DEV)), dict(out=torch.zeros(2, count)), dict(out=torch.zeros(2, count, device=DEV, dtype=torch.float64)),
           dict(dy=torch.zeros(3, 6, 6, device=DEV)[:, :, ::2]), dict(activation="gelu")]
    for over in bad:
        with pytest.raises(ValueError):
            mlp.backward(**dict(dict(widths=widths, params=params, x=x, dy=dy), **over))
    with pytest.raises(NotImplementedError):
        mlp.backward((5, 257, 3), torch.zeros(1, 1, device=DEV), x, dy)
    assert tuple(mlp.backward(widths, params, x, dy).shape) == (2, count)
