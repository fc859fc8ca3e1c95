"""ctypes mirror of ``include/ftl.h`` (the C-ABI of the HIP library).

Field order and types must match the header exactly; ``tests/test_abi.py`` checks the struct sizes
against ``ftl_sizeof_*`` exported by the library."""
import ctypes as C

FTL_ABI_VERSION = 4
FTL_MAX_BEARS = 6
FTL_MAX_LASERS = 4
FTL_MAX_AUX = 8
AUX_LIDAR, AUX_TRACK_VECTOR, AUX_TRACK_RADAR = 1, 2, 3
FTL_MAX_REGIME = 16
FTL_OBS_NUM = 10
FTL_MAX_CORR_CAP = 512

FTL_OK = 0
FTL_E_INVALID, FTL_E_UNSUPPORTED, FTL_E_DEVICE, FTL_E_STATE = -1, -2, -3, -4

MISSION = ("in_progress", "fail", "success", "finished_by_time")          # ENV:951-955, 963, 1083, 1130
AGENT = ("moving", "crash", "low_reward", "too_far_from_leader", "finished")
LEADER = ("moving", "crash", "finished")

FTL_ERR_TRAJ_OVERFLOW, FTL_ERR_CORR_OVERFLOW, FTL_ERR_EMPTY_CORRIDOR, FTL_ERR_TRACKER_SEED, FTL_ERR_HIST1_OVERFLOW = 1, 2, 4, 8, 16
FTL_ERR_LIDAR_OVERFLOW = 32
FTL_ERR_BAD_ACTION = 64
FTL_ERR_BAD_STREAM = 128
FTL_ACTION_BOX2, FTL_ACTION_DISCRETE, FTL_ACTION_TURN = 0, 1, 2
FTL_STEP_AUTO_RESET = 1
FTL_STEP_NEXT_RESET = 4
FTL_STEP_QUEUE_RESET = 8
FTL_STEP_SAMPLE_RESET = 16
FTL_STEP_NO_SENSORS = 32          # no sensor kernels in this call: lasers / policy_obs keep what they held (ftl_scan refreshes them)
FTL_EPISODE_DONE_AT_RESET = 1
# the baseline follower (include/ftl.h, ftl_baseline_act): sticky bits of a row's flags word, the row's header and size
FTL_BL_EMPTY, FTL_BL_OVERFLOW = 1, 2
BL_HEAD, BL_COUNT, BL_PENDING, BL_FLAGS = range(4)


def baseline_row_bytes(cap):
    """Bytes of one follower row: int32 {head, count, pending, flags} + ``cap`` points of two float64."""
    return 16 + 16 * int(cap)
# columns of a scenario sampler's table (include/ftl.h, ftl_scenario_sampler)
FTL_N_SCEN_STATS = 10
(SS_EPISODES, SS_FRAMES_SUM, SS_SUCCESS, SS_CRASH, SS_LOW_REWARD, SS_TOO_FAR, SS_TIMEOUT, SS_RETURN_Q16, SS_DONE_AT_RESET,
 SS_LAST_CALL) = range(10)
SS_NAMES = ("episodes", "frames_sum", "success", "crash", "low_reward", "too_far", "timeout", "return_q16", "done_at_reset", "last_call")
FTL_N_METRICS = 8
FTL_METRICS_CLEAR = 1
(M_EPISODES, M_RETURN_SUM, M_FRAMES_SUM, M_SUCCESS, M_CRASH, M_LOW_REWARD, M_TOO_FAR, M_TIMEOUT) = range(8)

# env_int indices
(EI_SCEN, EI_TARGET_ID, EI_LEADER_FINISHED, EI_DONE, EI_CRASH, EI_IN_BOX, EI_ON_TRACE, EI_TOO_CLOSE,
 EI_STEP_COUNT, EI_FINISH_TIMER, EI_TRAJ_LEN, EI_TRK_COUNTER, EI_CORR_LO, EI_CORR_HI, EI_SEED_END,
 EI_SNAP_COUNT, EI_DYN_INDEX0, EI_DYN_INDEX1, EI_DYN_INDEX2, EI_DYN_INDEX3, EI_DYN_INDEX4, EI_DYN_INDEX5, EI_ERROR, EI_EPISODES,
 EI_GREEN_COUNT, EI_GREEN_LEN, EI_SCAN_OK, EI_SNAP_HEAD, EI_HINT, EI_GREEN_TINY, EI_RESETS, EI_ACC_CONSUMED,
 EI_HINT_X, EI_HINT_Y, EI_CLR_GREEN, EI_CLR_ALL, EI_FPS, EI_HW0_LO, EI_HW0_HI, EI_HIST1_LEN, EI_ERROR_STICKY, EI_STREAM, EI_COUNT) = range(43)
# ftl_unpack_envs flags (include/ftl.h)
FTL_ENV_SLOT_STATS, FTL_ENV_OWN_STREAM = 1, 2
ED_ACC_PENALTY, ED_OVERALL_REWARD, ED_SPARE0, ED_SPARE1, ED_BEAR_POINTS = range(5)
ED_GREEN_W = ED_BEAR_POINTS + 2 * FTL_MAX_BEARS
ED_CUR_MULT, ED_CUR_ACC, ED_CUM_SPEED = ED_GREEN_W + 1, ED_GREEN_W + 2, ED_GREEN_W + 3
ED_COUNT = ED_CUM_SPEED + 1
RD_DIRECTION, RD_SPEED, RD_ROT_SPEED, RD_DES_SPEED, RD_DES_ROT_SPEED, RD_COUNT = range(6)
RI_X, RI_Y, RI_W, RI_H, RI_ROT_DIR, RI_DES_ROT_DIR, RI_SPARE0, RI_SPARE1, RI_COUNT = range(9)


def rand_frames(rng_seed, env_id, resets, step_count, lo, hi):
    """Twin of ftl_rand_frames (include/ftl.h): the stand-in for np.random.randint(lo, hi) at ENV:405/940."""
    v = lo + int(uniform01(rng_seed, env_id, resets, step_count | (1 << 40)) * (hi - lo))
    return v if v < hi else hi - 1


def rand_range(rng_seed, env_id, resets, frame, bear, k, start, stop):
    """Twin of ftl_rand_range (include/ftl.h): the stand-in for random.randrange(start, stop, 10) at ENV:753-754."""
    n = (stop - start + 9) // 10
    v = int(uniform01(rng_seed, env_id, resets, frame | (1 << 41) | (bear << 44) | (k << 48)) * n)
    return start + 10 * (v if v < n else n - 1)


class RobotParams(C.Structure):
    _fields_ = [("min_speed", C.c_double), ("max_speed", C.c_double), ("max_rotation_speed", C.c_double),
                ("max_speed_change", C.c_double), ("max_rotation_speed_change", C.c_double),
                ("img_w", C.c_int32), ("img_h", C.c_int32), ("_pad", C.c_int32 * 2)]


class LaserCfg(C.Structure):
    _fields_ = [("count", C.c_int32), ("react_corridor", C.c_int32), ("react_green", C.c_int32),
                ("react_obstacles", C.c_int32), ("history", C.c_int32), ("after_tracker", C.c_int32),
                ("out_offset", C.c_int32), ("pad_sectors", C.c_int32), ("lenient", C.c_int32), ("in_policy_obs", C.c_int32),
                ("length", C.c_double), ("angle_offset", C.c_double),
                ("explicit_angles", C.c_int32), ("compas", C.c_int32), ("ray_angles", C.c_double * 8)]


class AuxCfg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("after_tracker", C.c_int32), ("out_offset", C.c_int32), ("out_len", C.c_int32),
                ("n_angles", C.c_int32), ("points_number", C.c_int32), ("return_all_points", C.c_int32),
                ("return_only_distances", C.c_int32), ("range_px", C.c_double), ("in_range_px", C.c_double),
                ("angle_step", C.c_double), ("border_angle", C.c_int32), ("seq_len", C.c_int32),
                ("detectable", C.c_int32), ("radar_sectors", C.c_int32)]


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("frames_per_step", C.c_int32), ("max_steps", C.c_int32), ("warm_start", C.c_int32),
                ("trajectory_saving_period", C.c_int32), ("n_static", C.c_int32), ("n_bears", C.c_int32),
                ("move_bear_v4", C.c_int32), ("ignore_follower_collisions", C.c_int32),
                ("aggregate_reward", C.c_int32), ("has_low_reward", C.c_int32),
                ("has_max_distance_coef", C.c_int32), ("has_tracker", C.c_int32),
                ("tracker_saving_period", C.c_int32), ("tracker_start_behind", C.c_int32),
                ("n_lasers", C.c_int32), ("traj_cap", C.c_int32), ("corr_cap", C.c_int32),
                ("route_cap", C.c_int32), ("init_traj_cap", C.c_int32), ("hist1_cap", C.c_int32), ("trk1_eat_close_points", C.c_int32),
                ("low_reward", C.c_double), ("max_distance_coef", C.c_double),
                ("min_distance", C.c_double), ("max_distance", C.c_double), ("max_dev", C.c_double),
                ("leader_pos_epsilon", C.c_double), ("corridor_length", C.c_double),
                ("corridor_width", C.c_double),
                ("reward_in_box", C.c_double), ("reward_on_track", C.c_double), ("reward_in_dev", C.c_double),
                ("not_on_track_penalty", C.c_double), ("crash_penalty", C.c_double),
                ("too_close_penalty", C.c_double), ("leader_movement_reward", C.c_double),
                ("leader", RobotParams), ("follower", RobotParams), ("bear", RobotParams),
                ("lasers", LaserCfg * FTL_MAX_LASERS),
                ("n_speed_regime", C.c_int32), ("n_acc_regime", C.c_int32),
                ("speed_key", C.c_int32 * FTL_MAX_REGIME), ("speed_is_range", C.c_int32 * FTL_MAX_REGIME),
                ("acc_key", C.c_int32 * FTL_MAX_REGIME), ("env_id_base", C.c_int32),
                ("rand_fps_lo", C.c_int32), ("rand_fps_hi", C.c_int32), ("_pad1", C.c_int32),
                ("speed_lo", C.c_double * FTL_MAX_REGIME), ("speed_hi", C.c_double * FTL_MAX_REGIME),
                ("acc_val", C.c_double * FTL_MAX_REGIME), ("rng_seed", C.c_uint64),
                ("trk1_eat_radius", C.c_double), ("n_aux", C.c_int32), ("_pad2", C.c_int32), ("aux", AuxCfg * FTL_MAX_AUX)]


_M64 = (1 << 64) - 1


def mix64(x):
    x &= _M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x


def uniform01(rng_seed, env_id, resets, frame):
    """Python twin of ftl_uniform01() in include/ftl.h (the stream that replaces random.uniform at ENV:1156)."""
    key = mix64(rng_seed + 0x9E3779B97F4A7C15 * (env_id + 1)) ^ mix64(0xD1B54A32D192ED03 * (resets + 1))
    return (mix64(key + 0x9E3779B97F4A7C15 * (frame + 1)) >> 11) * (1.0 / 9007199254740992.0)


def search_uniform(seed, stream_id, call, it, k, block, j):
    """Python twin of ftl_search_uniform() in include/ftl.h: coordinate ``j`` of hold block ``block`` of candidate ``k`` in round ``it`` of
    search call ``call`` of the env on absolute stream ``stream_id`` (key range bit 43 of the ``uniform01`` stream)."""
    return uniform01(seed, stream_id, call, (1 << 43) | block | (j << 16) | (it << 17) | (k << 24))


def mulhi64(a, b):
    return ((a & _M64) * (b & _M64)) >> 64


def sample_scenario(rng_seed, stream_id, resets, cdf, base=0):
    """Python twin of ftl_sample_scenario() in include/ftl.h, in Python integers: the pool index ``base + idx`` an env on stream
    ``stream_id`` draws when its episode number ``resets`` ends.  ``cdf``: the inclusive prefix sums of the uint32 weights."""
    key = mix64(rng_seed + 0x9E3779B97F4A7C15 * (stream_id + 1)) ^ mix64(0xD1B54A32D192ED03 * (resets + 1))
    x = mix64(key + 0x9E3779B97F4A7C15 * ((1 << 42) + 1))
    count = len(cdf)
    total = int(cdf[count - 1])
    if total == 0:
        return base + mulhi64(x, count)
    r = mulhi64(x, total)
    lo, hi = 0, count - 1
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if int(cdf[mid]) <= r:
            lo = mid + 1
        else:
            hi = mid
    return base + lo


class Scenarios(C.Structure):
    _fields_ = [("n_scenarios", C.c_int32), ("_pad", C.c_int32),
                ("static_rects", C.c_void_p), ("robot_pos", C.c_void_p), ("robot_dir", C.c_void_p),
                ("robot_rect", C.c_void_p), ("route", C.c_void_p), ("route_len", C.c_void_p),
                ("init_traj", C.c_void_p), ("init_traj_len", C.c_void_p)]


class ScenParams(C.Structure):
    """ftl_scen_params: what the reset-time scenario generator needs of Game(**kwargs)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("step_grid", C.c_int32), ("obstacle_number", C.c_int32),
                ("add_obstacles", C.c_int32), ("add_bear", C.c_int32), ("bear_number", C.c_int32), ("bear_behind", C.c_int32),
                ("multiple_end_points", C.c_int32), ("path_finding_iterations", C.c_int32),
                ("bridge_gap", C.c_int32), ("bridge_width", C.c_int32),
                ("trajectory_saving_period", C.c_int32), ("planner", C.c_int32),
                ("min_distance", C.c_double), ("max_distance", C.c_double),
                ("leader_pos_epsilon", C.c_double), ("leader_margin", C.c_double),
                ("leader_w", C.c_double), ("leader_h", C.c_double), ("leader_max_speed", C.c_double),
                ("fixed_route", C.c_void_p), ("fixed_route_len", C.c_int32), ("_pad", C.c_int32)]


SCEN_FOUND, SCEN_DONE_AT_RESET, SCEN_ROUTE_OVERFLOW, SCEN_TRAJ_OVERFLOW, SCEN_REF_RAISES = 1, 2, 4, 8, 16
SCEN_GEN_LIMIT = 32              # ftl_generate_scenarios_device only: a rejection sampler hit its cap of 2^20 draws


class Outputs(C.Structure):
    _fields_ = [("obs_num", C.c_void_p), ("lasers", C.c_void_p), ("target", C.c_void_p),
                ("reward", C.c_void_p), ("done", C.c_void_p), ("status", C.c_void_p), ("policy_obs", C.c_void_p)]

# ftl_tune keys (include/ftl.h)
FTL_TUNE_COSCHEDULED_ENVS, FTL_TUNE_REGROUP_EVERY, FTL_TUNE_TWO_STREAMS = 0, 1, 2


class FinalOutputs(C.Structure):
    """ftl_final_outputs: the terminal rows and the ended / restarted masks of ftl_step_final."""
    _fields_ = [("obs_num", C.c_void_p), ("lasers", C.c_void_p), ("target", C.c_void_p), ("policy_obs", C.c_void_p),
                ("ended", C.c_void_p), ("restarted", C.c_void_p)]


class RolloutOutputs(C.Structure):
    """ftl_rollout_outputs: discounted return, alive steps and terminal status row per env of ftl_rollout."""
    _fields_ = [("ret", C.c_void_p), ("steps", C.c_void_p), ("status", C.c_void_p)]


FTL_SEARCH_OWN_STREAM = 1


class SearchParams(C.Structure):
    """ftl_search_params: candidates per env, horizon, hold, rounds; discount, radius and its decay; seed; flags."""
    _fields_ = [("K", C.c_int32), ("T", C.c_int32), ("hold", C.c_int32), ("iters", C.c_int32),
                ("gamma", C.c_double), ("spread", C.c_double), ("decay", C.c_double), ("seed", C.c_uint64),
                ("flags", C.c_uint32), ("_pad", C.c_int32)]


class SearchBuffers(C.Structure):
    """ftl_search_buffers: the device buffers of one ftl_search call (``search.ActionSearch`` owns them)."""
    _fields_ = [("rows", C.c_void_p), ("row_ids", C.c_void_p), ("env_ids", C.c_void_p), ("nominal", C.c_void_p), ("cand", C.c_void_p),
                ("action", C.c_void_p), ("best_k", C.c_void_p), ("best_ret", C.c_void_p), ("out", C.POINTER(Outputs)),
                ("ro", C.POINTER(RolloutOutputs))]


class GuidedBuffers(C.Structure):
    """ftl_guided_buffers: the fields of ``SearchBuffers`` (``nominal`` / ``cand`` hold residuals), the real batch's outputs, the follower
    rows of the real envs and of the clones with their byte sizes, and ``cap`` (``search.GuidedSearch`` owns them)."""
    _fields_ = SearchBuffers._fields_ + [("real_out", C.POINTER(Outputs)), ("real_bl", C.c_void_p), ("real_bl_bytes", C.c_size_t),
                                         ("search_bl", C.c_void_p), ("search_bl_bytes", C.c_size_t), ("cap", C.c_int32), ("_pad", C.c_int32)]


# the MLP policy population (include/ftl.h, ftl_mlp_act): the limits of a net and the staging sizes of ftl_mlp_kernel (csrc/ftl_mlp.hpp)
FTL_MLP_MAX_LAYERS, FTL_MLP_MAX_WIDTH, FTL_MLP_MAX_IN = 4, 256, 4096
FTL_MLP_ENV_TILE, FTL_MLP_K_CHUNK, FTL_MLP_W_STAGE, FTL_MLP_ENVS_PER_WAVE, FTL_MLP_NEURON_BLOCK, FTL_MLP_THREADS = 32, 64, 4096, 16, 16, 256
FTL_MLP_ACT_RELU, FTL_MLP_ACT_TANH = 0, 1          # ftl_mlp.activation: the hidden layers' function
FTL_MLP_BWD_SPAN, FTL_MLP_BWD_MAX_IN = 64, FTL_MLP_MAX_IN          # ftl_mlp_backward: tiles of a span, the input-width limit


def mlp_param_count(widths):
    """Floats of one weight set (``ftl_mlp_param_count``): per layer W ``[in][out]`` then b ``[out]``."""
    return sum((int(a) + 1) * int(b) for a, b in zip(widths[:-1], widths[1:]))


def mlp_chunk_rows(w_out):
    """Input rows of a layer with ``w_out`` neurons that ftl_mlp_kernel stages at a time (``chunk_rows`` of csrc/ftl_mlp.hpp)."""
    return min(FTL_MLP_K_CHUNK, FTL_MLP_W_STAGE // int(w_out)) & ~3


class Mlp(C.Structure):
    """ftl_mlp: the parameters of a policy population, its shape and which envs use which weight set."""
    _fields_ = [("params", C.c_void_p), ("set_stride", C.c_int64), ("n_sets", C.c_int32), ("n_layers", C.c_int32),
                ("width", C.c_int32 * (FTL_MLP_MAX_LAYERS + 1)), ("env_first", C.c_int32), ("envs_per_set", C.c_int32),
                ("activation", C.c_int32)]


# the kinds of a recorded transition (include/ftl.h, ftl_collect_mlp): kind[t][e] of ftl_collect_buffers, read by ftl_gae
FTL_TR_STEP, FTL_TR_TERMINATED, FTL_TR_TRUNCATED, FTL_TR_VOID = 0, 1, 2, 3


class CollectBuffers(C.Structure):
    """ftl_collect_buffers: where ftl_collect_mlp records a trajectory (block t of an array at base + t * its ``*_step_bytes``)."""
    _fields_ = [("obs", C.c_void_p), ("head", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("kind", C.c_void_p),
                ("noise", C.c_void_p), ("sigma", C.c_void_p),
                ("obs_step_bytes", C.c_int64), ("head_step_bytes", C.c_int64), ("action_step_bytes", C.c_int64),
                ("reward_step_bytes", C.c_int64), ("kind_step_bytes", C.c_int64), ("noise_step_bytes", C.c_int64)]


# the recurrent policy (include/ftl.h, ftl_rnn_act): the cell limit, the bits of ftl_rnn.flags, the flag of a call, the cells of a gate pass
FTL_RNN_MAX_CELL = 128
FTL_RNN_PREV_ACTION, FTL_RNN_PREV_REWARD = 1, 2
FTL_RNN_ZERO_ON_OUT_DONE = 1
FTL_RNN_PASS_CELLS = 64


def rnn_widths(widths, cell, flags):
    """(P, R, U, S) of a recurrent net: the widths of a_prev and r_prev in the cell input, the cell input's width, the floats of a state row."""
    head = int(widths[-1])
    P, R = (head if flags & FTL_RNN_PREV_ACTION else 0), (1 if flags & FTL_RNN_PREV_REWARD else 0)
    return P, R, int(widths[-2]) + P + R + int(cell), 2 * int(cell) + P + 1


def rnn_param_count(widths, cell, flags):
    """Floats of one weight set (``ftl_rnn_param_count``): the trunk ``widths[:-1]`` as in ``mlp_param_count``, W_g ``[U][4C]``, b_g
    ``[4C]``, W_y ``[C][A]``, b_y ``[A]``; ``widths[-1]`` is the head width."""
    U = rnn_widths(widths, cell, flags)[2]
    return mlp_param_count(widths[:-1]) + (U + 1) * 4 * int(cell) + (int(cell) + 1) * int(widths[-1])


class Rnn(C.Structure):
    """ftl_rnn: ftl_mlp's fields (``n_layers`` the trunk's layers, the head width after the trunk's widths), the cell and its state."""
    _fields_ = Mlp._fields_ + [("cell", C.c_int32), ("flags", C.c_uint32), ("state", C.c_void_p), ("state_stride", C.c_int64)]


class RnnSequence(C.Structure):
    """ftl_rnn_sequence: the recorded blocks ``ftl_rnn_forward`` reads (obs, action, reward, kind, reward0) and what it writes (head, h,
    state_out at block ``state_at``); block b of an array lies ``b * *_block_bytes`` past its base."""
    _fields_ = [("obs", C.c_void_p), ("obs_block_bytes", C.c_int64), ("action", C.c_void_p), ("action_block_bytes", C.c_int64),
                ("reward", C.c_void_p), ("reward_block_bytes", C.c_int64), ("kind", C.c_void_p), ("kind_block_bytes", C.c_int64),
                ("reward0", C.c_void_p), ("head", C.c_void_p), ("head_block_bytes", C.c_int64), ("h", C.c_void_p), ("h_block_bytes", C.c_int64),
                ("state_out", C.c_void_p), ("state_at", C.c_int32)]


FTL_RNN_BWD_SPAN = 64                 # ftl_rnn_backward: (tile, block) pairs of a span


def rnn_backward_lds_bytes(widths, cell, flags):
    """LDS bytes of a workgroup of ftl_rnn_backward_kernel (the Limits line of the ``ftl_rnn_backward`` block of include/ftl.h): the
    trunk's hidden buffers, u, dh, the weight stage, and the region that is xs | h' | dy before the gate passes and dz from then on."""
    Lt, A, cell = len(widths) - 2, int(widths[-1]), int(cell)
    U = rnn_widths(widths, cell, flags)[2]
    r32 = lambda w: ((int(w) + 31) & ~31) + 2
    act, us, hs = r32(max([A] + [int(w) for w in widths[1:Lt]])), r32(U), r32(cell)
    cn = min(cell, FTL_RNN_PASS_CELLS)
    products = [int(w) for w in widths[1:Lt + 1]] + [4 * cn] + ([4 * (cell - cn)] if cell > cn and cell % cn else [])
    stage = max([FTL_MLP_W_STAGE + 64] + [mlp_chunk_rows(w) * (((w + 27) & ~31) + 4) for w in products])
    region = max(4 * cn + 2, FTL_MLP_K_CHUNK + 2 + hs + r32(A))
    return 4 * (FTL_MLP_ENV_TILE * ((Lt - 1) * act + us + hs + region) + stage)


FTL_RNN_BWD_MAX_LDS = 160 * 1024      # ftl_rnn_backward: a net whose workgroup needs more is FTL_E_UNSUPPORTED


class RnnGradient(C.Structure):
    """ftl_rnn_gradient: what ``ftl_rnn_backward`` takes beside the sequence -- the head gradients of every block, where the parameter
    gradient goes, the workspace, and the optional gradients of the state after the last block (in) and before the first (out)."""
    _fields_ = [("dhead", C.c_void_p), ("dhead_block_bytes", C.c_int64), ("grad", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("dstate_in", C.c_void_p), ("dstate_out", C.c_void_p)]


# the PPO loss head (include/ftl.h, ftl_ppo_head): rows of a segment, columns of stats
FTL_PPO_SEG, FTL_PPO_STATS = 1024, 8


class PpoHeadArgs(C.Structure):
    """ftl_ppo_head_args: the heads, the record, the advantages and the values of ``ftl_ppo_head``, its scalars, and where the gradients, the
    statistics and the segment partials go (block b of an array at base + b * its ``*_block_bytes``)."""
    _fields_ = [("n_blocks", C.c_int32), ("n", C.c_int32), ("n_sets", C.c_int32), ("width", C.c_int32),
                ("head_new", C.c_void_p), ("head_new_block_bytes", C.c_int64), ("head_old", C.c_void_p), ("head_old_block_bytes", C.c_int64),
                ("noise", C.c_void_p), ("noise_block_bytes", C.c_int64),
                ("sigma_old", C.c_void_p), ("sigma_new", C.c_void_p), ("log_sigma_shift", C.c_void_p),
                ("adv", C.c_void_p), ("adv_block_bytes", C.c_int64), ("ret", C.c_void_p), ("ret_block_bytes", C.c_int64),
                ("value_new", C.c_void_p), ("value_new_block_bytes", C.c_int64), ("kind", C.c_void_p), ("kind_block_bytes", C.c_int64),
                ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("vf_coef", C.c_float), ("normalize", C.c_int32),
                ("dhead", C.c_void_p), ("dhead_block_bytes", C.c_int64), ("dvalue", C.c_void_p), ("dvalue_block_bytes", C.c_int64),
                ("dlog_std", C.c_void_p), ("stats", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class RnnCollectBuffers(C.Structure):
    """ftl_rnn_collect_buffers: ``CollectBuffers`` plus where the state rows every decision read are recorded."""
    _fields_ = [("b", CollectBuffers), ("state", C.c_void_p), ("state_step_bytes", C.c_int64), ("state_steps", C.c_int32), ("_pad", C.c_int32)]


class EpisodeRecord(C.Structure):
    """ftl_episode_record: one row per entry of an episode queue, written once (``RECORD_DTYPE`` is the same row for numpy)."""
    _fields_ = [("state", C.c_int32), ("scenario", C.c_int32), ("env", C.c_int32), ("frames", C.c_int32), ("calls", C.c_int32),
                ("status", C.c_int32 * 3), ("errors", C.c_uint32), ("flags", C.c_uint32), ("ret", C.c_double), ("stream", C.c_int64)]


RECORD_DTYPE = [("state", "<i4"), ("scenario", "<i4"), ("env", "<i4"), ("frames", "<i4"), ("calls", "<i4"), ("status", "<i4", (3,)),
                ("errors", "<u4"), ("flags", "<u4"), ("ret", "<f8"), ("stream", "<i8")]


class EpisodeQueueC(C.Structure):
    """ftl_episode_queue: device pointers of a queue's arrays (``vec_game.EpisodeQueue`` owns them)."""
    _fields_ = [("scenario", C.c_void_p), ("stream", C.c_void_p), ("stream_base", C.c_int64), ("n", C.c_int32), ("_pad", C.c_int32),
                ("head", C.c_void_p), ("records", C.c_void_p), ("ticket", C.c_void_p)]


class ScenarioSamplerC(C.Structure):
    """ftl_scenario_sampler: device pointers of a sampler's arrays (``vec_game.ScenarioSampler`` owns them)."""
    _fields_ = [("weight", C.c_void_p), ("cdf", C.c_void_p), ("base", C.c_int32), ("count", C.c_int32), ("table", C.c_void_p)]


# ftl_render (include/ftl.h): layer bits and the image parameters
RENDER_PATH, RENDER_BOX, RENDER_OBJECTS, RENDER_RECTS, RENDER_SENSORS, RENDER_TARGET = 1, 2, 4, 8, 16, 32
RENDER_ALL = 63


class RenderParams(C.Structure):
    """ftl_render_params: output size, world pixels per output pixel, world coordinate of output pixel (0, 0)'s corner, layers."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("scale", C.c_float), ("origin_x", C.c_float), ("origin_y", C.c_float),
                ("layers", C.c_uint32), ("_pad", C.c_int32)]
