"""The baseline follower's contract (include/ftl.h, ftl_baseline_act), restated in tests/baseline_numpy.py, against what the UNMODIFIED
reference's controller did (tests/golden/gen/make_golden_baseline.py): the 4,096-row table of utils/misc.py:move_to_the_point and four
closed-loop episodes of the loop of run_2d.py --mode base.  No GPU."""
import json
import os

import numpy as np
import pytest

import baseline_numpy as BN
from golden_util import GOLDEN, config_for, scenario_arrays
from oracle_batch import OracleBatch

EPISODES = ("A_s0", "B_s1", "Bastar_s1", "E_s3")
V_CAP = 8          # rows of the table whose v may sit one ulp from the reference's (expected: 4096 * 2^-12 = 1)


def load_baseline(name):
    with np.load(os.path.join(GOLDEN, "baseline_%s.npz" % name)) as f:
        z = {k: f[k] for k in f.files}               # (an NpzFile unpacks an array again at every access)
    return z, json.loads(str(z["meta"]))


def ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


@pytest.fixture(scope="module")
def table():
    with np.load(os.path.join(GOLDEN, "baseline_table.npz")) as f:
        return {k: f[k] for k in f.files}


def test_table_covers_every_branch(table):
    """The crafted rows are there: rx == 0, rx < 0, an angle difference of exactly 0, of exactly 180, above 180 in both senses, direction
    359.99, integer and non-integer targets."""
    px, py = table["pos"][:, 0].astype(np.float64), table["pos"][:, 1].astype(np.float64)
    tx, ty = table["target"][:, 0], table["target"][:, 1]
    des = np.array([int(BN.angle_to_point(px[i], py[i], tx[i], ty[i])) for i in range(len(px))])
    cur = table["direction"].astype(np.int64)
    assert len(px) == 4096
    assert (tx == px).any() and (tx < px).any() and (tx > px).any()
    assert (des == cur).any() and (np.abs(des - cur) == 180).any() and (des - cur > 180).any() and (cur - des > 180).any()
    assert (table["direction"] == np.float32(359.99)).any()
    is_int = np.all(table["target"] == np.rint(table["target"]), axis=1)
    assert is_int.sum() > 1000 and (~is_int).sum() > 1000
    assert (table["v"] <= 20.0).sum() > 100 and (table["v"] > 20.0).sum() > 1000


def test_table_w_exact_v_within_one_ulp(table):
    """(a) w exact on every row, v within 1 ulp on every row and bit-identical on all but at most V_CAP; the x87 evaluation reproduces
    the reference's v on every row, so the reference alone is inside the cap."""
    n = len(table["v"])
    got = np.array([BN.move_to_the_point(table["direction"][i], table["pos"][i], table["target"][i]) for i in range(n)])
    x87 = np.array([BN.euclid_x87(table["pos"][i, 0], table["pos"][i, 1], table["target"][i, 0], table["target"][i, 1]) for i in range(n)])
    assert np.array_equal(got[:, 1], table["w"])
    d = ulps(got[:, 0], table["v"])
    print("baseline table: %d of %d rows of v not bit-identical to the reference (max %d ulp)" % (int((d != 0).sum()), n, int(d.max())))
    assert d.max() <= 1
    assert int((d != 0).sum()) <= V_CAP
    assert np.array_equal(x87, table["v"])


@pytest.mark.parametrize("name", EPISODES)
def test_fixture_conditions(name):
    """What the generator promises of a seed: the FIFO never ran empty nor above 64, no v within 4 ulp of the pop threshold."""
    z, _ = load_baseline(name)
    assert z["bl:fifo_len"].min() >= 1 and z["bl:fifo_len"].max() <= 64
    assert (np.abs(z["actions"][:, 0] - 20.0) > 4 * np.spacing(20.0)).all()
    assert np.array_equal(z["bl:fifo_len"][1:], (z["bl:fifo_len"][:-1] + z["bl:append"][:-1].astype(np.int32) - z["bl:pop"][:-1]))
    assert len(z["done"]) <= 300 and (z["done"][-1] or len(z["done"]) == 300)


@pytest.mark.parametrize("name", EPISODES)
def test_replay_recorded_observations(name):
    """(b) Fed the recorded observations, the restatement reproduces every recorded w, FIFO length, append and pop."""
    z, _ = load_baseline(name)
    f = BN.Follower(cap=64)
    T = len(z["actions"])
    for t in range(T):
        num, target = (z["reset:num"], z["reset:target"]) if t == 0 else (z["obs:num"][t - 1], z["obs:target"][t - 1])
        v, w = f.act(num, target, 0 if t == 0 else t)
        assert w == z["actions"][t, 1], (name, t, w, z["actions"][t, 1])
        assert ulps(v, z["actions"][t, 0]) <= 1, (name, t, v, z["actions"][t, 0])
        assert len(f.fifo) == z["bl:fifo_len"][t], (name, t)
        if t:
            assert (f.appended, f.popped) == (bool(z["bl:append"][t - 1]), bool(z["bl:pop"][t - 1])), (name, t)
    assert f.flags == 0


@pytest.mark.parametrize("name", EPISODES)
def test_closed_loop_around_the_oracle(name):
    """(c) The restatement driving the C oracle replays the episode: w, done and status exact at every step, reward within 1e-5."""
    z, meta = load_baseline(name)
    cfg = config_for(meta, scen_route_len=len(z["scen:route"]))
    env = OracleBatch(cfg, 1)
    env.reset([scenario_arrays(z)], [0])
    f = BN.Follower(cap=64)
    for t in range(len(z["actions"])):
        v, w = f.act(env.obs_num[0], env.target[0], int(env.counters()[0][0]))
        assert w == z["actions"][t, 1], (name, t, w, z["actions"][t, 1])
        assert len(f.fifo) == z["bl:fifo_len"][t], (name, t)
        env.step(np.array([[v, w]]))
        assert bool(env.done[0]) == bool(z["done"][t]), (name, t)
        assert tuple(env.status[0]) == tuple(z["info"][t]), (name, t, env.status[0], z["info"][t])
        assert abs(env.reward[0] - z["reward"][t]) <= 1e-5, (name, t, env.reward[0], z["reward"][t])
    assert f.flags == 0


def test_flags_and_restart_rule():
    """The two rules the reference has no counterpart for, and the restart at step count 0."""
    num = np.zeros(10, np.float32)
    num[5], num[6] = 100.0, 100.0
    f = BN.Follower(cap=2)
    f.act(num, (100.0, 100.0), 0)
    assert f.fifo == [(100.0, 100.0)] and f.pending and f.flags == 0
    f.act(num, (100.0, 100.0), 5)                      # the pop would empty the FIFO
    assert f.fifo == [(100.0, 100.0)] and f.flags == BN.FTL_BL_EMPTY
    f = BN.Follower(cap=2)
    f.act(num, (500.0, 100.0), 0)
    f.act(num, (600.0, 100.0), 5)
    f.act(num, (700.0, 100.0), 10)                     # a third point into a ring of two
    assert f.fifo == [(600.0, 100.0), (700.0, 100.0)] and f.flags == BN.FTL_BL_OVERFLOW
    f.act(num, (900.0, 900.0), 0)                      # a reset observation
    assert f.fifo == [(900.0, 900.0)] and f.flags == BN.FTL_BL_OVERFLOW and not f.appended and not f.popped
