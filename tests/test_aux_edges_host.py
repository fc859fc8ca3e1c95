"""The cases of tests/aux_edge_cases.py on the ORACLE alone: each reaches the branch of csrc/ftl_aux.hpp it is built for, so a failure
of tests/test_gpu_aux_edges.py is never "the world missed the branch".  The counts come from a float64 numpy restatement of the
reference's objects_in_range and from the oracle's own tracker state; `pytest -s` prints them."""
import numpy as np
import pytest

import aux_edge_cases as X
from continiousenvironment_follower_leader_amd import abi
from oracle_batch import OracleBatch
from test_gpu_configs import _actions


@pytest.mark.parametrize("variant", ["distances", "all_points"])
def test_dense_worlds_put_every_lidar_in_its_regime(variant):
    """Case a: at every compared step every env has at most 56 objects in range of the range-1 lidar, 73..120 of the range-2 one and at
    least 137 of the range-5 one; no object within 1e-6 px of a threshold; rects of scan index >= 64 stop rays of both longer lidars."""
    cfg = X.dense_config(variant)
    assert cfg.c.n_static == 152 and cfg.c.n_bears == 2
    scen = X.dense_scenarios(cfg)
    for s in scen:                       # what dense_world promises
        r = s["static_rects"]
        d = X.rect_distance(r, s["robot_pos"][1])
        assert r.shape == (152, 4) and (r % 5 == 0).all() and (r[:, 2:] >= 10).all() and (r[:, 2:] <= 30).all() and d.min() >= 60 and d.max() <= 395
    n = X.DENSE_ENVS
    ora = OracleBatch(cfg, n)
    idx = np.arange(n)
    ora.reset(scen, idx)
    lidars = [j for j in range(cfg.c.n_aux)]
    assert [cfg.aux[j].name for j in lidars] == ["lidar_r1", "lidar_r2", "lidar_r5"]
    lo = {j: 10 ** 9 for j in lidars}; hi = {j: 0 for j in lidars}; late = {j: 0 for j in lidars}; gap = np.inf

    def look():
        nonlocal gap
        for j, (cnt, g, lt) in X.lidar_counts(cfg, ora, scen, idx).items():
            lo[j], hi[j], late[j], gap = min(lo[j], int(cnt.min())), max(hi[j], int(cnt.max())), late[j] + int(lt.sum()), min(gap, g)
    look()
    for t in range(X.DENSE_STEPS):
        ora.step(_actions(cfg, n, t, "mixed" if t % 2 else "random", seed=31))
        look()
        r = X.dense_reset(t, idx, len(scen))
        if r is not None:
            idx = r[1]
            ora.reset(scen, idx, mask=r[0])
            look()
    print("aux_edges dense[%s]: objects in range min..max r1 %d..%d, r2 %d..%d, r5 %d..%d; nearest threshold %.3g px; rays stopped first by a "
          "rect of scan index >= 64: r2 %d, r5 %d" % (variant, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], gap, late[1], late[2]))
    assert hi[0] <= X.LIDAR_MASK - 8
    assert lo[1] >= X.LIDAR_MASK + 1 + 8 and hi[1] <= X.LIDAR_RECTS - 8
    assert lo[2] >= X.LIDAR_RECTS + 1 + 8
    assert gap > 1e-6
    assert late[1] > 0 and late[2] > 0
    assert int(np.bitwise_or.reduce(ora.counters()[2])) == 0


@pytest.mark.parametrize("which", ["rays", "all_points"])
def test_split_lidars_hit_something(which):
    """Case b: every lidar of the index-split configs has a ray that ends short of its range (only a hit goes through the index split
    of the march; the leader stands 2 m ahead of the follower, so even the one-ray lidar sees it)."""
    cfg = X.split_config(which)
    scen = X.generated_scenarios(cfg, np.arange(12))[:X.SPLIT_ENVS]
    n = X.SPLIT_ENVS
    assert len(scen) == n
    ora = OracleBatch(cfg, n)
    ora.reset(scen, np.arange(n))
    short = {a.name: 0 for a in cfg.aux}
    for t in range(X.SPLIT_STEPS):
        ora.step(_actions(cfg, n, t, seed=37))
        for j, a in enumerate(cfg.aux):
            A = cfg.c.aux[j]
            blk = ora.lasers[:, a.out_offset:a.out_offset + a.out_len]
            if A.return_all_points:                    # a ray without a hit contributes all its points
                short[a.name] += int((blk[:, 0] < A.n_angles * A.points_number).sum())
            else:
                d = blk if A.return_only_distances else np.hypot(blk[:, 0::2], blk[:, 1::2])
                short[a.name] += int((d < A.range_px * (1 - 1e-3)).sum())
    print("aux_edges split[%s]: readings short of the range" % which, short)
    assert all(v > 0 for v in short.values()), short
    assert max(cfg.c.aux[j].n_angles * cfg.c.aux[j].points_number for j in range(cfg.c.n_aux)) >= 64512


def test_compas_windows_outgrow_the_stage():
    """Case c: at least half the envs end with a corridor of more than 128 points in the newest snapshot, and windows of exactly 128 and
    of 129 points both occur on the way (the two sides of `top - base <= FTL_COMPAS_STAGE`)."""
    cfg = X.compas_config()
    scen = X.generated_scenarios(cfg, np.arange(96))
    n = X.COMPAS_ENVS
    ora = OracleBatch(cfg, n)
    idx = np.arange(n) % len(scen)
    ora.reset(scen, idx)
    seen = set()

    def windows():
        w = X.oracle_counters(ora)[:, 13]
        seen.update(int(v) for v in w)
        return w
    windows()
    for t in range(X.COMPAS_STEPS):
        ora.step(_actions(cfg, n, t, "mixed" if t % 2 else "random", seed=41))
        w = windows()
        r = X.periodic_reset(t, 10, idx, len(scen))
        if r is not None:
            idx = r[1]
            ora.reset(scen, idx, mask=r[0])
            windows()
    print("aux_edges compas: window of the newest snapshot at the last step min %d, median %d, max %d; longest seen %d"
          % (w.min(), np.median(w), w.max(), max(seen)))
    assert (w > X.COMPAS_STAGE).sum() * 2 >= n
    assert X.COMPAS_STAGE in seen and X.COMPAS_STAGE + 1 in seen
    assert int(np.bitwise_or.reduce(ora.counters()[2])) & (abi.FTL_ERR_CORR_OVERFLOW | abi.FTL_ERR_TRAJ_OVERFLOW) == 0


@pytest.mark.parametrize("tracker", X.DETECT_TRACKERS)
def test_detector_histories_outgrow_a_wavefront(tracker):
    """Case d: on the v2 tracker and on the v1 tracker that saves every step and eats nothing the history passes 64 and 65 points in at
    least half the envs -- every position_sequence_length but 300, which stays the zero-filled case; the other v1 settings save a point
    every third or seventh step, or eat what the follower reaches: their history stays short, and is reported."""
    cfg = X.detector_config(tracker)
    assert cfg.c.n_aux == abi.FTL_MAX_AUX
    scen = X.generated_scenarios(cfg, np.arange(64))
    n = X.DETECT_ENVS
    ora = OracleBatch(cfg, n)
    idx = np.arange(n) % len(scen)
    ora.reset(scen, idx)
    top = np.zeros(n, np.int64)
    for t in range(X.DETECT_STEPS):
        ora.step(_actions(cfg, n, t, "mixed" if t % 2 else "random", seed=43))
        top = np.maximum(top, X.oracle_counters(ora)[:, 12])
    print("aux_edges detectors[%s]: longest history per env min %d, median %d, max %d" % (tracker, top.min(), np.median(top), top.max()))
    if tracker in ("v2", "v1_p1_noeat"):
        assert (top > 65).sum() * 2 >= n
    err = int(np.bitwise_or.reduce(ora.counters()[2]))
    assert err & (abi.FTL_ERR_HIST1_OVERFLOW | abi.FTL_ERR_CORR_OVERFLOW | abi.FTL_ERR_TRAJ_OVERFLOW) == 0


def test_seven_detector_configs_cover_every_detector():
    seen, sectors = set(), set()
    assert len(set(X.DETECTORS)) == 20
    for tr in X.DETECT_TRACKERS:
        cfg = X.detector_config(tr)
        mine = [cfg.c.aux[j] for j in range(cfg.c.n_aux)]
        for A in mine:
            seen.add(("vector" if A.kind == abi.AUX_TRACK_VECTOR else "radar", A.seq_len, ("new", "old", "near")[A.detectable]))
            if A.kind == abi.AUX_TRACK_RADAR:
                sectors.add(A.radar_sectors)
        # every tracker setting feeds radars and vector detectors that look at more than a wavefront of points
        assert max(A.seq_len for A in mine if A.kind == abi.AUX_TRACK_VECTOR) > 64, tr
        assert any(A.detectable == 2 or A.seq_len > 64 for A in mine if A.kind == abi.AUX_TRACK_RADAR), tr
        assert max(A.radar_sectors for A in mine if A.kind == abi.AUX_TRACK_RADAR) >= 180, tr
    assert seen == set(X.DETECTORS) and sectors == set(X.SECTORS)
    first = X.detector_config("v2")
    assert not first.aux[0].after_tracker and all(a.after_tracker for a in first.aux[1:])      # one detector ahead of the v2 tracker
