"""The two host-side seams of the batch layer (vec_game.py): the table of per-env output tensors that ``VecGame`` and
``PipelinedVecGame`` allocate from, and the split of global env ids over the parts of a pipelined batch.  No device needed."""
import copy
import itertools
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, config_for, load_episode
from continiousenvironment_follower_leader_amd.shard import shard_range
from continiousenvironment_follower_leader_amd.vec_game import _output_table, _split_ids

F32, F64, U8 = torch.float32, torch.float64, torch.uint8


def _meta_B():
    return json.loads(str(np.load(os.path.join(GOLDEN, "pool_B.npz"))["meta"]))


def _expected(lasers_len, policy_shape, policy_obs, final_obs):
    """The rows of the ``VecGame`` docstring, written out: obs_num f32[10], lasers f32[sum_k H_k * N_k], target f64[2], reward f64[],
    done u8[], status u8[3]; then policy_obs f32[H, sum_k N_k]; then the final buffers, the masks, and final_policy_obs last."""
    rows = [("obs_num", (10,), F32), ("lasers", (lasers_len,), F32), ("target", (2,), F64), ("reward", (), F64), ("done", (), U8),
            ("status", (3,), U8)]
    has_policy = policy_obs and policy_shape is not None
    if has_policy:
        rows.append(("policy_obs", policy_shape, F32))
    if final_obs:
        rows += [("final_obs_num", (10,), F32), ("final_lasers", (lasers_len,), F32), ("final_target", (2,), F64), ("ended", (), U8),
                 ("restarted", (), U8)]
        if has_policy:
            rows.append(("final_policy_obs", policy_shape, F32))
    return rows


# config B: two ray sensors of 12 and 24 lasers, 5 rows of history each -> 5 * 12 + 5 * 24 = 180 values, policy rows of 12 + 24 = 36;
# config D: one ray sensor, its lasers_count set to 180 after construction, 5 rows of history -> 900 values, policy rows of 180
CASES = {"B": (lambda: config_for(dict(kwargs=_meta_B()["kwargs"], post=None)), 180, (5, 36)),
         "D": (lambda: config_for(load_episode("D_s2_chase")[1]), 900, (5, 180))}


@pytest.mark.parametrize("policy_obs,final_obs", list(itertools.product((False, True), (False, True))))
@pytest.mark.parametrize("name", sorted(CASES))
def test_output_table_names_order_shapes_dtypes(name, policy_obs, final_obs):
    make, lasers_len, policy_shape = CASES[name]
    table = _output_table(make(), policy_obs, final_obs)
    got = [(k, tuple(shape), dtype) for k, (shape, dtype) in table.items()]
    assert got == _expected(lasers_len, policy_shape, policy_obs, final_obs)


@pytest.mark.parametrize("final_obs", (False, True))
def test_output_table_without_ray_sensors(final_obs):
    """No ray sensor: ``lasers`` keeps one placeholder column and ``policy_obs`` is absent even when asked for."""
    cfg = config_for(dict(kwargs=dict(_meta_B()["kwargs"], follower_sensors={}), post=None))
    assert cfg.lasers_len == 0 and not cfg.lasers
    got = [(k, tuple(shape), dtype) for k, (shape, dtype) in _output_table(cfg, True, final_obs).items()]
    assert got == _expected(1, None, True, final_obs)


def test_output_table_refuses_unequal_histories():
    kw = copy.deepcopy(_meta_B()["kwargs"])
    kw["follower_sensors"]["LeaderCorridor_lasers_obstacles"]["max_prev_obs"] = 7
    cfg = config_for(dict(kwargs=kw, post=None))
    with pytest.raises(ValueError, match="max_prev_obs"):
        _output_table(cfg, True, False)
    with pytest.raises(ValueError, match="max_prev_obs"):
        _output_table(cfg, True, True)
    # not asked for: no check, and the histories simply add up (5 * 12 + 7 * 24)
    assert _output_table(cfg, False, False)["lasers"] == ((228,), F32)


def test_split_ids_over_parts():
    shards = [shard_range(8, k, 3) for k in range(3)]
    assert [(s.lo, s.hi) for s in shards] == [(0, 3), (3, 6), (6, 8)]
    games = ["g0", "g1", "g2"]
    ids = torch.tensor([5, 0, 7, 5, 2], dtype=torch.int64)
    parts = list(_split_ids(ids, shards, games))
    assert [g for g, _, _ in parts] == games
    assert [(pos.tolist(), local.tolist()) for _, pos, local in parts] == [([1, 4], [0, 2]), ([0, 3], [2, 2]), ([2], [1])]
    back = torch.full_like(ids, -1)                 # scattering every part's ids back by position gives the request
    for g, pos, local in parts:
        back[pos] = local + shards[games.index(g)].lo
    assert torch.equal(back, ids)

    parts = list(_split_ids(torch.tensor([7, 1, 6, 1]), shards, games))        # nothing in [3, 6): that part is skipped
    assert [(g, pos.tolist(), local.tolist()) for g, pos, local in parts] == [("g0", [1, 3], [1, 1]), ("g2", [0, 2], [1, 0])]
    assert list(_split_ids(torch.zeros(0, dtype=torch.int64), shards, games)) == []
