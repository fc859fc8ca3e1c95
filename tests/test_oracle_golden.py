"""The CPU oracle (oracle/ftl_oracle.c) against the golden episodes produced by the UNMODIFIED reference
(tests/golden/gen/make_golden.py).  This is what pins the oracle: every observable of every step --
numerical_features, ray-sensor rows, leader_target_point, reward, done, info codes -- plus the internal
state the generator dumped (robot poses / controller state / integer hitboxes, counters, tracker history
and corridor) must agree.  Integer / flag state bit-exactly, floats to the north_star tolerance (they are in
fact bit-identical in this container; the test keeps the contract tolerance so that it stays meaningful on
a host with a different libm)."""
import numpy as np
import pytest

from golden_util import check_oracle_episode, config_for, episode_names, load_episode
from oracle import OracleEnv


@pytest.mark.parametrize("name", episode_names())
def test_oracle_matches_reference_episode(name):
    z, meta = load_episode(name)
    cfg = config_for(meta, scen_route_len=len(z["scen:route"]))
    env = OracleEnv(cfg)
    check_oracle_episode(name, z, meta, cfg, env)


def test_golden_covers_terminal_modes():
    """The fixture set must exercise every way an episode ends (ENV:960-964, 1077-1107, 1129-1134)."""
    seen = set()
    for name in episode_names():
        z, _ = load_episode(name)
        for row, d in zip(z["info"], z["done"]):
            if d:
                seen.add(tuple(int(v) for v in row))
    assert (1, 1, 0) in seen      # fail / crash
    assert (2, 4, 2) in seen      # success
    assert (3, 0, 0) in seen      # finished_by_time
    assert (1, 2, 0) in seen      # low_reward


def test_golden_reaches_the_staging_edges():
    """The three records made for the capacity edges of csrc/ftl_aux.hpp reach them (a regenerated fixture must not quietly miss its
    target): a corridor longer than the 128 points the compas sensors stage, a v1 history longer than the 100 positions its detector
    takes, a dense lidar with at least 30 rays stopped short of its range."""
    z, _ = load_episode("Clong_s1_chase")
    assert z["dbg:trk"][:, 2].max() > 128
    z, _ = load_episode("Tnoeat_s3_chase")
    assert z["dbg:trk"][:, 1].max() > 100
    z, meta = load_episode("Ledge_s2_chase")
    cfg = config_for(meta)
    a = [a for a in cfg.aux if a.name == "lidar_dense"][0]
    assert a.params["n_angles"] * a.params["points_number"] == 65341
    short = (z["obs:aux:lidar_dense"] < a.params["range_px"] * (1 - 1e-3)).sum(1)
    assert z["obs:aux:lidar_dense"].shape[1] == 361 and short.max() >= 30
