/*
 * ftl.h -- C-ABI of the MI355X-native batched `Game.step()` for the 2-D
 * continuous_grid_arctic follow-the-leader environment.
 *
 * The reference has no FFI layer: the path sits behind the gym API of
 * `class Game(gym.Env)` (reference src/continuous_grid_arctic/
 * follow_the_leader_continuous_env.py, "ENV" below) plus the sensor plugin
 * registry (utils/sensors.py "SEN", utils/classes.py "CLS").  The entry points
 * below are what a ctypes binding inside the reference's `Game` would call in
 * place of its Python hot loop; each one cites the reference interface it
 * replaces.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: plain pointers and sizes only (no torch types); every function
 * returns 0 on success or a negative FTL_E_* code and stores a message
 * retrievable with ftl_last_error(); a handle is bound to one (process,
 * device, stream-at-call-time) and is not thread-safe -- the same contract as
 * the reference (one env object per process, Python exceptions instead of
 * codes).  All buffer arguments of ftl_reset/ftl_step are DEVICE pointers
 * owned by the caller (PyTorch-ROCm tensors); the library only borrows them
 * for the duration of the call.
 */
#ifndef FTL_H
#define FTL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTL_ABI_VERSION 4
#define FTL_MAX_BEARS 6   /* robots per env = 2 + bears <= 8 (one lane each in a group of the frame kernel); bears 5, 7, .. of
                             move_bear_v4 draw their way-points from `random` every frame (ENV:750-754): ftl_rand_range below */
#define FTL_MAX_LASERS 4
#define FTL_MAX_AUX 8     /* lidar / leader-track detectors per env (ftl_aux_cfg) */
#define FTL_MAX_REGIME 16 /* entries of leader_speed_regime / leader_acceleration_regime */
#define FTL_OBS_NUM 10    /* numerical_features, ENV:1793-1802 */
#define FTL_TRAJ_BLOCK 32 /* trajectory points per bounding-box block (state field "traj_bb"; traj_cap is a multiple) */
#define FTL_MAX_CORR_CAP 512 /* largest ftl_config.corr_cap that ftl_create accepts */

/* error codes */
#define FTL_OK 0
#define FTL_E_INVALID (-1)   /* bad argument / config rejected (reference: ValueError, ENV:419-427, SEN:761-762) */
#define FTL_E_UNSUPPORTED (-2) /* reference feature outside the hot-path scope (NotImplementedError) */
#define FTL_E_DEVICE (-3)    /* HIP runtime error */
#define FTL_E_STATE (-4)     /* call order: state not bound / scenarios not loaded */

/* status codes written to `status[n][3]` = info dict of ENV:951-955 */
enum { FTL_MISSION_IN_PROGRESS = 0, FTL_MISSION_FAIL = 1, FTL_MISSION_SUCCESS = 2, FTL_MISSION_FINISHED_BY_TIME = 3 };
enum { FTL_AGENT_MOVING = 0, FTL_AGENT_CRASH = 1, FTL_AGENT_LOW_REWARD = 2, FTL_AGENT_TOO_FAR = 3, FTL_AGENT_FINISHED = 4 };
enum { FTL_LEADER_MOVING = 0, FTL_LEADER_CRASH = 1, FTL_LEADER_FINISHED = 2 };

/* per-env error bits (env_int[FTL_EI_ERROR]); a reference run would have raised here */
#define FTL_ERR_TRAJ_OVERFLOW 1u      /* leader_factual_trajectory longer than traj_cap */
#define FTL_ERR_CORR_OVERFLOW 2u      /* tracker history longer than corr_cap */
#define FTL_ERR_EMPTY_CORRIDOR 4u     /* SEN:893/962: scan with len(corridor) <= 1 (reference: UnboundLocalError) */
#define FTL_ERR_TRACKER_SEED 8u       /* SEN:264-297: fewer than 2 seed points / popleft on empty corridor */
#define FTL_ERR_HIST1_OVERFLOW 16u    /* v1 tracker history longer than hist1_cap */
#define FTL_ERR_LIDAR_OVERFLOW 32u    /* more than 128 objects within range of a LaserSensor: the extra ones were ignored */
#define FTL_ERR_BAD_ACTION 64u        /* ftl_step_encoded: a Discrete(5) action outside 0..4 (reference: KeyError at ENV:922); stepped as action 2 */
#define FTL_ERR_BAD_STREAM 128u       /* episode queue: a stream id of ftl_episode_queue.stream outside 0 .. INT32_MAX (sticky word only); the
                                         entry was played on the id's low 32 bits */

/* robot kinematic limits, px/frame and deg/frame (ENV:330-357, 556-566, 704-714; CLS:59-105) */
typedef struct ftl_robot_params {
    double min_speed, max_speed;
    double max_rotation_speed;
    double max_speed_change;          /* "acceleration" */
    double max_rotation_speed_change; /* 20/100 everywhere in the reference */
    int32_t img_w, img_h;             /* size of the scaled sprite = un-rotated hitbox (CLS:42) */
    int32_t _pad[2];
} ftl_robot_params;

/* one LeaderCorridor_Prev_lasers_v2 instance (SEN:742-769, 873-881) */
typedef struct ftl_laser_cfg {
    int32_t count;            /* lasers_count */
    int32_t react_corridor;   /* react_to_safe_corridor */
    int32_t react_green;      /* react_to_green_zone */
    int32_t react_obstacles;  /* 0 False, 1 True/"all", 2 "static", 3 "dynamic" (SEN:651-660) */
    int32_t history;          /* max_prev_obs (rows of the output) */
    int32_t after_tracker;    /* 1: scanned after the tracker's 2nd scan of the step (dict order, CLS:269-286) */
    int32_t out_offset;       /* filled by the library: offset of this sensor's [history][width] block in `lasers` */
    int32_t pad_sectors;      /* SEN:932-953: rows are [front|right|behind|left], 4*count wide, zeros outside a ray's sector */
    int32_t lenient;          /* 1: LeaderCorridor_lasers_v2 (SEN:736-807) -- one row of the current edges, and a corridor of <= 1 points
                                 reads laser_length on every ray instead of raising (no FTL_ERR_EMPTY_CORRIDOR).
                                 A ray sensor without edges -- of any class: react_corridor 0, react_green 0 and react_obstacles 0, or 3
                                 ("dynamic") with n_bears 0 -- has no segment to hit: every ray reads laser_length and NO error bit is set,
                                 although the reference raises IndexError in reset() there (its empty edge array is 1-D, SEN:706 / 787 /
                                 908).  The case is a property of the config alone: make_config warns about it. */
    int32_t in_policy_obs;    /* 1: the sensor is one of the classes ContinuousObserveModifier_sensorPrev concatenates
                                 (LeaderCorridor_Prev_lasers_v2/_v3 and LeaderCorridor_lasers_compas, utils/wrappers.py:204, 214) */
    double length;            /* laser_length, px */
    double angle_offset;      /* first_laser_angle_offset, deg */
    int32_t explicit_angles;  /* 1: LeaderCorridor_lasers (SEN:571-702) -- ray i points at direction + ray_angles[i] instead of a full circle */
    int32_t compas;           /* 1: LeaderCorridor_lasers_compas (SEN:1138-1288) -- corridor walls only, kept in float64; rows are 5*count wide:
                                 [no wall hit | front | back | left | right] by the orientation of the nearest wall (ftl_aux_kernel) */
    double ray_angles[8];     /* deg: -40, 0, 40 [, -90, 90] [, -150, 150] (SEN:609-632) */
} ftl_laser_cfg;

/* The sensors of the registry (SEN:1291-1307) that are not ray casts against segments: their float32 outputs are further
 * blocks of ftl_outputs.lasers, after the ray sensors' blocks, in dict order. */
enum { FTL_AUX_LIDAR = 1,         /* LaserSensor (SEN:18-145): point-in-rect marching along available_angle / angle_step rays */
       FTL_AUX_TRACK_VECTOR = 2,  /* LeaderTrackDetector_vector (SEN:342-387): vectors follower -> the newest / oldest tracked leader positions */
       FTL_AUX_TRACK_RADAR = 3 }; /* LeaderTrackDetector_radar (SEN:390-487): nearest tracked position per sector of the front half plane */
typedef struct ftl_aux_cfg {
    int32_t kind;
    int32_t after_tracker;        /* 1: scanned after the v2 tracker's 2nd scan of the step (dict order, CLS:269-286) */
    int32_t out_offset, out_len;  /* filled by the library: block inside ftl_outputs.lasers, f32 elements */
    /* lidar */
    int32_t n_angles;             /* 1 + 2 * (number of angle_step increments until border_angle is reached), SEN:88-101 */
    int32_t points_number;
    int32_t return_all_points;    /* the scan returns EVERY marching point up to and including the first hit of every ray (all points_number of a ray
                                     without a hit), rays in order, as the reference's list does (SEN:112-113, 131-134) -- an array whose length K
                                     changes from call to call: out = [K as a float][K points (x, y) or K distances][zeros] in a block of
                                     1 + n_angles * points_number * (2 or 1) floats */
    int32_t return_only_distances; /* out = [n][1] norms instead of [n][2] offsets (SEN:131-134) */
    double  range_px;             /* sensor_range * PIXELS_TO_METER */
    double  in_range_px;          /* range_px + 3 * PIXELS_TO_METER: objects farther than this (distance_to_rect) are ignored, SEN:78-79 */
    double  angle_step;
    int32_t border_angle;         /* int(available_angle / 2) */
    /* detectors */
    int32_t seq_len;              /* position_sequence_length */
    int32_t detectable;           /* 0 "new", 1 "old", 2 "near" (radar only) */
    int32_t radar_sectors;
} ftl_aux_cfg;

/* Game(**kwargs) after unit conversion (ENV:45-105, 283-357) */
typedef struct ftl_config {
    int32_t abi_version;
    int32_t width, height;               /* game_width, game_height */
    int32_t frames_per_step;
    int32_t max_steps;                   /* in frames (ENV:1127-1134) */
    int32_t warm_start;                  /* in frames */
    int32_t trajectory_saving_period;    /* 5, ENV:262 */
    int32_t n_static;                    /* walls + rocks */
    int32_t n_bears;
    int32_t move_bear_v4;
    int32_t ignore_follower_collisions;
    int32_t aggregate_reward;
    int32_t has_low_reward, has_max_distance_coef; /* early_stopping keys, ENV:1088-1107 */
    int32_t has_tracker;                 /* 2: LeaderPositionsTracker_v2 present; 1: the deprecated LeaderPositionsTracker (SEN:148-229: scanned once
                                            per step, corridor half-width max_dev, never trimmed, history thinned by eat_close_points); 0: none */
    int32_t tracker_saving_period;
    int32_t tracker_start_behind;        /* start_corridor_behind_follower */
    int32_t n_lasers;
    int32_t traj_cap;                    /* capacity of leader_factual_trajectory per env (points) */
    int32_t corr_cap;                    /* capacity of tracker history / corridor ring per env */
    int32_t route_cap;                   /* capacity of the planned route per scenario (waypoints) */
    int32_t init_traj_cap;               /* capacity of the initial trajectory per scenario */
    int32_t hist1_cap;                   /* capacity of the v1 tracker's position history per env (points) */
    int32_t trk1_eat_close_points;       /* v1 tracker: eat_close_points */
    double low_reward, max_distance_coef;
    double min_distance, max_distance, max_dev; /* px */
    double leader_pos_epsilon;
    double corridor_length, corridor_width;
    /* Reward dataclass, reward_constructor.py:4-16 with leader_movement_reward=0 (ENV:279) */
    double reward_in_box, reward_on_track, reward_in_dev, not_on_track_penalty;
    double crash_penalty, too_close_penalty, leader_movement_reward;
    ftl_robot_params leader, follower, bear;
    ftl_laser_cfg lasers[FTL_MAX_LASERS];
    /* leader_speed_regime (ENV:382-386, 1143-1157): entries in dict insertion order; the LAST entry with key <=
     * step_count (frames) wins; a [lo, hi] entry draws uniform(lo, hi) EVERY frame.  n_speed_regime < 0: None. */
    int32_t n_speed_regime;
    int32_t n_acc_regime;                /* leader_acceleration_regime (ENV:390-394, 1159-1174); < 0: None */
    int32_t speed_key[FTL_MAX_REGIME];
    int32_t speed_is_range[FTL_MAX_REGIME];
    int32_t acc_key[FTL_MAX_REGIME];
    int32_t env_id_base;                 /* global index of env 0 of this handle (multi-GPU shards draw distinct streams) */
    int32_t rand_fps_lo, rand_fps_hi;    /* random_frames_per_step bounds [lo, hi) (ENV:402-405, 939-940); hi == 0: fixed frames_per_step */
    int32_t _pad1;
    double speed_lo[FTL_MAX_REGIME], speed_hi[FTL_MAX_REGIME];
    double acc_val[FTL_MAX_REGIME];
    uint64_t rng_seed;                   /* seed of the counter-based streams that replace the global `random` (ftl_uniform01) */
    double trk1_eat_radius;              /* v1 tracker: max(follower.width, follower.height) in px (SEN:213) */
    int32_t n_aux, _pad2;
    ftl_aux_cfg aux[FTL_MAX_AUX];
} ftl_config;

/* Counter-based uniform stream that stands in for `random.uniform` at ENV:1156: the draw of
 * frame `frame` of the `resets`-th episode of global env `env_id` is a pure function of (rng_seed, env_id, resets,
 * frame), so the oracle, the device and the golden generator agree without sharing generator state. */
static inline uint64_t ftl_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL; x ^= x >> 27; x *= 0x94D049BB133111EBULL; x ^= x >> 31; return x;
}
static inline double ftl_uniform01(uint64_t rng_seed, uint64_t env_id, uint64_t resets, uint64_t frame) {
    uint64_t key = ftl_mix64(rng_seed + 0x9E3779B97F4A7C15ULL * (env_id + 1)) ^ ftl_mix64(0xD1B54A32D192ED03ULL * (resets + 1));
    return (double)(ftl_mix64(key + 0x9E3779B97F4A7C15ULL * (frame + 1)) >> 11) * (1.0 / 9007199254740992.0);
}

/* np.random.randint(lo, hi) of ENV:405/940 on the same counter stream, in a key range of its own (bit 40 of the frame key):
 * the draw made after the step that ended at frame `step_count` of episode `resets` (0, 0: the constructor's draw). */
static inline int32_t ftl_rand_frames(uint64_t rng_seed, uint64_t env_id, uint64_t resets, uint64_t step_count, int32_t lo, int32_t hi) {
    double u = ftl_uniform01(rng_seed, env_id, resets, step_count | (1ULL << 40));
    int32_t v = lo + (int32_t)(u * (double)(hi - lo));
    return v < hi ? v : hi - 1;
}

/* random.randrange(start, stop, 10) of ENV:753-754 (the way-points of bears with an odd index >= 5 under move_bear_v4: four (x, y)
 * pairs per bear and frame, of which the pair at dynamics_index is used) on the same counter stream, key range bit 41: draw `k`
 * (0..7 = x, y of pair 0..3) of bear `bear` in frame `frame`.  CPython: start + 10 * _randbelow(ceil((stop - start) / 10)). */
static inline int32_t ftl_rand_range(uint64_t rng_seed, uint64_t env_id, uint64_t resets, uint64_t frame, int32_t bear, int32_t k,
                                     int32_t start, int32_t stop) {
    const int32_t n = (stop - start + 9) / 10;
    double u = ftl_uniform01(rng_seed, env_id, resets, frame | (1ULL << 41) | ((uint64_t)bear << 44) | ((uint64_t)k << 48));
    int32_t v = (int32_t)(u * (double)n);
    return start + 10 * (v < n ? v : n - 1);
}

/* The weighted scenario draw of the scenario sampler (ftl_scenario_sampler below) on the same counter stream, in a key range of its own
 * (bit 42 of the frame key): the draw an env on stream `stream_id` makes when its episode number `resets` ends (ftl_sampler_start: before
 * its first).  cdf[i] is the inclusive prefix sum of the uint32 weights 0 .. i, total = cdf[count - 1].  The raw 64 bits x of the mix
 * (not the >> 11 double) are scaled to r = mulhi(x, total) in [0, total); the result is the number of cdf entries <= r, i.e. the first i
 * with cdf[i] > r; total == 0 (every weight zero) gives mulhi(x, count): uniform over the window.  Integers throughout: an entry of
 * weight 0 is never drawn, and the result is the same on any device, in any slot, in any order. */
static inline uint64_t ftl_mulhi64(uint64_t a, uint64_t b) {
    const uint64_t a0 = a & 0xFFFFFFFFULL, a1 = a >> 32, b0 = b & 0xFFFFFFFFULL, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFULL) + (p10 & 0xFFFFFFFFULL);
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
static inline int32_t ftl_sample_scenario(uint64_t rng_seed, uint64_t stream_id, uint64_t resets, const uint64_t* cdf, int32_t count) {
    uint64_t key = ftl_mix64(rng_seed + 0x9E3779B97F4A7C15ULL * (stream_id + 1)) ^ ftl_mix64(0xD1B54A32D192ED03ULL * (resets + 1));
    const uint64_t x = ftl_mix64(key + 0x9E3779B97F4A7C15ULL * ((1ULL << 42) + 1));
    const uint64_t total = cdf[count - 1];
    if (total == 0) return (int32_t)ftl_mulhi64(x, (uint64_t)count);
    const uint64_t r = ftl_mulhi64(x, total);
    int32_t lo = 0, hi = count - 1;                  /* cdf[count - 1] = total > r */
    while (lo < hi) { const int32_t mid = lo + (hi - lo) / 2; if (cdf[mid] <= r) lo = mid + 1; else hi = mid; }
    return lo;
}

/* Scenario pool = output of the reference's reset() (ENV:434-543) for P episodes, device arrays.
 * Robots are ordered leader, follower, bear0.. (R = 2 + n_bears). */
typedef struct ftl_scenarios {
    int32_t n_scenarios;
    int32_t _pad;
    const int32_t* static_rects;   /* [P][n_static][4]  x,y,w,h  (integer pygame.Rect) */
    const float*   robot_pos;      /* [P][R][2]  f32 positions (CLS:47) */
    const double*  robot_dir;      /* [P][R]     start directions, deg */
    const int32_t* robot_rect;     /* [P][R][4] */
    const double*  route;          /* [P][route_cap][2]  planned route waypoints (ENV:1547-1550) */
    const int32_t* route_len;      /* [P] */
    const float*   init_traj;      /* [P][init_traj_cap][2]  initial leader_factual_trajectory (ENV:533-539) */
    const int32_t* init_traj_len;  /* [P] */
} ftl_scenarios;

/* ---- reset-time scenario generation (host side, no GPU involved) ------------------------------
 * The scenario part of Game.reset(): robots (ENV:545-611), bridge walls + rocks by rejection sampling (ENV:613-677),
 * finish point (ENV:1614-1630), grid route (ENV:1493-1612 on utils/dstar.py:84-210), bears (ENV:687-720, 761-770),
 * initial leader trajectory (ENV:533-539).  The draws come from a bit-compatible twin of CPython's `random`
 * (MT19937, seed(int), randrange) so that seed s yields the scenario of `game.seed(s); game.reset()`.
 * planner 1 ("astar") follows utils/astar.py:50-166 literally -- f = g + squared distance, CPython's heapq order on ties, the 1000-iteration
 * cap that returns the path to the last expanded node, the two legs through the bridge (ENV:1670-1700); found_target_point stays False as
 * in the reference (ENV:1537 is D*-only), so FTL_SCEN_FOUND is set whenever the route has at least two points.
 * The (dstar) route is a shortest 8-connected path on the reference's cost model (1 / sqrt 2 per move, inflated obstacle
 * cells); among equal-cost paths the reference's choice depends on CPython set iteration order over object ids and is
 * not reproducible -- the generator breaks such ties by insertion order (documented as unpinned in DESIGN.md).  The route's cost has
 * no bound but the grid's: around dense rocks it exceeds rows + cols several times over (370 on the 150 x 100 grid with 100 rocks), and
 * both generators find such a route as the reference does; it takes a route_cap to match (FTL_SCEN_ROUTE_OVERFLOW otherwise).  A
 * finish point the leader cannot reach leaves FTL_SCEN_FOUND clear and the route empty (the reference's planner would not return). */
typedef struct ftl_scen_params {
    int32_t width, height;                /* game_width, game_height */
    int32_t step_grid, obstacle_number;   /* obstacle_number is 0 when add_obstacles is False (ENV:323-324) */
    int32_t add_obstacles, add_bear, bear_number, bear_behind;
    int32_t multiple_end_points, path_finding_iterations;
    int32_t bridge_gap, bridge_width;     /* bridge_size[0], bridge_size[1] (ENV:617-620) */
    int32_t trajectory_saving_period;
    int32_t planner;                      /* path_finding_algorythm: 0 "dstar" (ENV:1493-1612), 1 "astar" (ENV:1632-1711 on utils/astar.py);
                                             2: the caller-supplied `trajectory=` of the constructor (ENV:229, 469-470): no finish point is drawn, no
                                             planner runs, every scenario gets fixed_route */
    double  min_distance, max_distance;   /* pixels */
    double  leader_pos_epsilon, leader_margin;
    double  leader_w, leader_h;           /* the float pixel sizes the reference keeps on the robot (ENV:352-353, CLS:104-105) */
    double  leader_max_speed;             /* px/frame */
    const double* fixed_route;            /* planner 2: [fixed_route_len][2] way-points (HOST pointer), else NULL */
    int32_t fixed_route_len, _pad;
} ftl_scen_params;

/* per-scenario status bits written by ftl_generate_scenarios */
#define FTL_SCEN_FOUND        1u   /* found_target_point (ENV:1537): the route reaches the finish point */
#define FTL_SCEN_DONE_AT_RESET 2u  /* empty route (ENV:508-510) */
#define FTL_SCEN_ROUTE_OVERFLOW 4u /* route longer than cfg->route_cap: truncated, do not use */
#define FTL_SCEN_TRAJ_OVERFLOW 8u  /* initial trajectory longer than cfg->init_traj_cap: truncated, do not use */
#define FTL_SCEN_REF_RAISES  16u   /* the reference's reset() would raise here (one-point route, ENV:513) */
#define FTL_SCEN_GEN_LIMIT   32u   /* device generator only: a rejection sampler (rocks ENV:651-668, finish point ENV:1614-1630) or
                                      randbelow drew 2^20 times without success -- the reference would go on drawing; unusable.  The
                                      host generator never sets it (no real seed gets there) */

/* Fill `out` (HOST arrays shaped like ftl_scenarios with P = n; cfg gives n_static, R, route_cap, init_traj_cap) with the
 * scenarios of python seeds seeds[0..n); status[i] gets the FTL_SCEN_* bits of scenario i.  n_threads <= 0: all cores. */
int ftl_generate_scenarios(const ftl_config* cfg, const ftl_scen_params* sp, const int64_t* seeds, int32_t n,
                           int32_t n_threads, const ftl_scenarios* out, uint8_t* status);

/* ---- the same generator on the GPU (ftl_scenario_dev.hpp): scenarios straight into device memory --------------------------------
 * Scenario i of ftl_generate_scenarios_device equals scenario i of ftl_generate_scenarios for the same seed, array for array, including
 * the zero padding and the status byte -- robots (ENV:545-611), bridge walls + rocks (ENV:613-677), finish point(s) (ENV:1614-1630, the
 * three legs of multiple_end_points ENV:470-481), the D* route (ENV:1493-1612 on utils/dstar.py:84-210, with its max_iterat cap), bears
 * (ENV:687-720, 761-770), the initial leader trajectory (ENV:533-539) -- except that
 *   - the start directions (atan, f64) and the follower's placements (cos / sin) are evaluated correctly rounded (double-double, rounded
 *     once); glibc's atan / sin / cos round the same way on every generator input measured (seeds 0..4095 of every golden dstar /
 *     trajectory config), but not on every double -- a seed where glibc is off by an ulp would give a start direction an ulp apart;
 *   - a rejection sampler that draws 2^20 times without success stops with FTL_SCEN_GEN_LIMIT (the host would go on drawing).
 * Limits: the D* grid, (width / step_grid + 2) x (height / step_grid + 2) cells, at most 65,536 cells, and at most 1,022 rocks
 * (n_static <= 1,024); beyond either, both entry points return FTL_E_UNSUPPORTED.
 * planner 0 (dstar) and 2 (fixed_route, a HOST pointer, copied into the workspace on `stream`) only; planner 1 (astar: CPython heapq order,
 * inherently sequential) returns FTL_E_UNSUPPORTED before any device work.  dev_seeds [n], the arrays of dev_out (P = n) and dev_status [n]
 * are DEVICE pointers; `workspace` is a device buffer of at least ftl_generate_scenarios_device_workspace(cfg, sp, n) bytes owned by the
 * caller (nothing is allocated here).  Asynchronous on `stream` (NULL: the null stream); the caller keeps every buffer alive until the
 * stream has passed the call. */
int ftl_generate_scenarios_device_workspace(const ftl_config* cfg, const ftl_scen_params* sp, int32_t n, size_t* workspace_bytes);
int ftl_generate_scenarios_device(const ftl_config* cfg, const ftl_scen_params* sp, const int64_t* dev_seeds, int32_t n,
                                  const ftl_scenarios* dev_out, uint8_t* dev_status, void* workspace, size_t workspace_bytes, void* stream);

/* struct sizes as this library was compiled (binding self-check) */
size_t ftl_sizeof_config(void);
size_t ftl_sizeof_scenarios(void);
size_t ftl_sizeof_outputs(void);
size_t ftl_sizeof_scen_params(void);
size_t ftl_sizeof_final_outputs(void);


/* step()/reset() outputs = (obs, reward, done, info) of ENV:945 for n envs, device arrays */
typedef struct ftl_outputs {
    float*   obs_num;    /* [n][10]            numerical_features (ENV:1793-1802) */
    float*   lasers;     /* [n][lasers_len]    per ray sensor k a [history_k][width_k] block at lasers[k].out_offset, width_k = count_k
                            (4*count_k with pad_sectors, 5*count_k for compas); then per aux sensor a block of aux[j].out_len at
                            aux[j].out_offset */
    double*  target;     /* [n][2]             leader_target_point (ENV:1803-1806) */
    double*  reward;     /* [n]                last-frame reward (ENV:935-936, 1136-1141) */
    uint8_t* done;       /* [n] */
    uint8_t* status;     /* [n][3]             mission / agent / leader status codes */
    float*   policy_obs; /* optional (may be NULL): [n][H][sum_k width_k] = ContinuousObserveModifier_sensorPrev.observation
                            (utils/wrappers.py:200-221): per sensor with in_policy_obs set clip(x / laser_length, 0, 1),
                            concatenated along axis 1; those sensors must share one history H (wrappers.py:183-188) */
} ftl_outputs;

typedef struct ftl_handle ftl_handle;

/* flags of ftl_step */
#define FTL_STEP_AUTO_RESET 1u  /* envs that finish are re-initialised from scenario (scen_idx+n_envs) % P inside the
                                   same launch; outputs keep the terminal reward/done/status, obs are the new episode's
                                   (ftl_step_final adds the terminal observations: "same-step" mode, below) */
#define FTL_STEP_NEXT_RESET 4u  /* "next-step" auto-reset (gymnasium 1.x, EnvPool): the call in which an episode ends returns its terminal
                                   observation like a step without auto-reset.  An env whose done word is set on ENTRY (whichever call set it)
                                   is re-initialised instead of stepped -- its action is ignored -- from the reset window's walk
                                   (ftl_set_reset_window) with the bookkeeping of FTL_STEP_AUTO_RESET: FTL_EI_EPISODES + 1, the episode's error
                                   bits OR-ed into the sticky word, FTL_EI_RESETS advanced (the same per-env random streams), ep_stats not
                                   recorded again (the step that set done did).  Its outputs are ftl_reset's for that env: the new episode's first
                                   observation (initial tracker and ray scans, ENV:541), reward 0, done = the new world's done-at-reset bit, status
                                   0/0/0.  Every other env steps as without the flag.  Combined with FTL_STEP_AUTO_RESET: FTL_E_INVALID. */

/* Terminal observations of ftl_step_final, device arrays ([n] = one row per env of the handle).  Rows of envs whose `ended` is 0 are
 * not written. */
typedef struct ftl_final_outputs {
    float*   obs_num;    /* [n][10]           the terminal rows of ftl_outputs.obs_num / lasers / target / policy_obs: what the */
    float*   lasers;     /* [n][lasers_len]   same call without FTL_STEP_AUTO_RESET returns for the env.  Needed (non-NULL) */
    double*  target;     /* [n][2]            under FTL_STEP_AUTO_RESET only; policy_obs may be NULL (needs out->policy_obs) */
    float*   policy_obs; /* [n][H][W]         optional */
    uint8_t* ended;      /* [n]  1: an episode ended in this call (done raised by this call's step; under FTL_STEP_AUTO_RESET every env
                                 whose outputs carry done = 1) -- always written, for every env */
    uint8_t* restarted;  /* [n]  1: this call re-initialised the env -- always written, for every env */
} ftl_final_outputs;

/* Game.__init__ (ENV:45-417): validate + freeze the config. device < 0 is rejected (there is no CPU path). */
int ftl_create(const ftl_config* cfg, int32_t n_envs, int32_t device, ftl_handle** out);
void ftl_destroy(ftl_handle* h);

/* number of f32 elements per env in ftl_outputs.lasers */
int32_t ftl_lasers_len(const ftl_handle* h);
/* copy of the frozen config (out_offset of every laser filled in) */
int ftl_get_config(const ftl_handle* h, ftl_config* out);

/* Per-env mutable state lives in ONE caller-owned device buffer (a torch uint8 tensor).  A fresh buffer MUST be
 * zero-initialised: the reset path relies on zeroed FTL_EI_FPS / FTL_EI_RESETS / FTL_EI_ACC_CONSUMED / FTL_EI_EPISODES /
 * FTL_EI_ERROR_STICKY words and on a zeroed "ep_stats" field (they survive reset() like the attributes of the reference's
 * Game object that reset() does not touch).  A buffer that already holds the state of an earlier run may be bound again. */
size_t ftl_state_bytes(const ftl_handle* h);
int ftl_bind_state(ftl_handle* h, void* dev_state, size_t bytes);

/* State introspection for parity tests: byte offset / element count / dtype code / row stride of a named field
 * ("rb_pos","rb_dbl","rb_int","env_int","env_dbl","fol_cs","snap_rects","snap_win" -- the fields of the per-env record -- and
 * "traj","traj_bb","hist","corr","corr32","ep_stats","hist1").  dtype: 0 i32, 1 f32, 2 f64.  Element j of env e sits at byte
 * offset + e * stride + j * sizeof(dtype), j < per_env: the record fields share one stride (the record size, a multiple of 128), the
 * others are dense [n_envs][per_env] arrays. */
int ftl_state_field(const ftl_handle* h, const char* name, size_t* offset, size_t* per_env, int32_t* dtype, size_t* stride);

/* reset() part 1 (ENV:461-492): hand over the scenario pool produced by reset-time generation. */
int ftl_load_scenarios(ftl_handle* h, const ftl_scenarios* pool);

/* The pool entries the in-kernel auto-reset (FTL_STEP_AUTO_RESET) draws from: a finished env that ran scenario s restarts from
 * base + ((s mod count) + stride) mod count.  ftl_load_scenarios sets the window to the whole pool with stride n_envs (base 0, count
 * n_scenarios), which is the walk documented at FTL_STEP_AUTO_RESET.  stride <= 0 keeps n_envs; a stride that shares a factor with count
 * visits only part of the window (n_envs a multiple of count: the same scenario again and again, which turns the few worlds that start
 * the follower inside a rock into one-step episodes forever) -- pick one that is coprime to count.  A caller that refills one half of a double-sized pool while the envs draw from the other
 * half (the reference builds a fresh world on every reset(), ENV:461-492; scenario.ScenarioRing) moves the window between steps; entries
 * outside the window stay valid for the episodes that are still running on them, so a half may be overwritten once every episode that
 * started before the window left it has ended (at most max_steps / frames_per_step + 1 steps). */
int ftl_set_reset_window(ftl_handle* h, int32_t base, int32_t count, int32_t stride);

/* Scheduling hints of a handle.  Results never depend on them (tests/test_gpu_api.py: regrouping, split path, pipelined parts).
 * FTL_TUNE_COSCHEDULED_ENVS: the number of envs that are stepped on this device at the same time, this handle's included -- a caller that
 *   runs the batch as several handles on several streams (two handles of 32,768 envs each: DESIGN.md section 6, PipelinedVecGame) says
 *   65,536 here.  The handle sorts its envs by expected cost when THAT many envs need more than one round of frame-kernel wavefronts
 *   (by itself it only knows its own batch, which it leaves unsorted when one round holds it).
 * FTL_TUNE_REGROUP_EVERY: rebuild the cost order every k-th step (default 4).
 * FTL_TUNE_TWO_STREAMS: 0 / 1 -- the handle's own two-stream mode (its two halves on two streams, joined every step: the default for
 *   configs with random_frames_per_step); a caller that overlaps whole handles switches it off.
 * The environment switches FTL_NO_REGROUP / FTL_REGROUP_EVERY / FTL_SPLIT (diagnostics) win over the hints. */
enum { FTL_TUNE_COSCHEDULED_ENVS = 0, FTL_TUNE_REGROUP_EVERY = 1, FTL_TUNE_TWO_STREAMS = 2 };
int ftl_tune(ftl_handle* h, int32_t what, int32_t value);

/* reset() (ENV:494-543): place env e at scenario scen_idx[e] for every e with mask[e] != 0 (mask NULL = all),
 * run the initial use_sensors (ENV:541) and write the first observation.  reward/done/status are zeroed. */
int ftl_reset(ftl_handle* h, const int32_t* scen_idx, const uint8_t* mask, const ftl_outputs* out, void* stream);

/* step(action) (ENV:908-945) for all envs: action[n][2] = (speed px/frame, signed rotation deg/frame) as f64. */
int ftl_step(ftl_handle* h, const double* action, const ftl_outputs* out, uint32_t flags, void* stream);

/* step(action) for the two other action spaces of the constructor (ENV:358-378), decoded on the device exactly as ENV:909-925 does:
 *   FTL_ACTION_BOX2      action = f64 [n][2]  (speed, signed rotation)                                   -- the same as ftl_step
 *   FTL_ACTION_DISCRETE  action = int32 [n]   index k of Discrete(5) -> (follower.max_speed, discrete_rotation_speed_to_value[k]) with the
 *                                 table {-max_rot, -max_rot/2, 0, max_rot/2, max_rot} of ENV:362-367 (discrete_action_space=True)
 *   FTL_ACTION_TURN      action = f64 [n]     Box(1) rotation -> (0.25, rotation): np.concatenate([[0.25], action]) of ENV:924-925
 *                                 (constant_follower_speed=True; the speed command of ENV:910-911 is overwritten by ENV:927) */
enum { FTL_ACTION_BOX2 = 0, FTL_ACTION_DISCRETE = 1, FTL_ACTION_TURN = 2 };
int ftl_step_encoded(ftl_handle* h, const void* action, int32_t encoding, const ftl_outputs* out, uint32_t flags, void* stream);

/* ftl_step_encoded plus the masks / terminal observations an RL loop needs (fin NULL: exactly ftl_step_encoded).
 *   FTL_STEP_AUTO_RESET ("same-step", SB3 `terminal_observation`, gymnasium `final_obs`): `out` and every state word are bit-identical to
 *     the same call without `fin`; the rows of fin->obs_num / lasers / target / policy_obs of the ended envs are bit-identical to what a
 *     step WITHOUT auto-reset returns for them; restarted = ended.  The step defers the reset of the envs that finish, the sensors scan
 *     their terminal state, ftl_final_copy_kernel copies those rows and a reset pass (the frame kernel's wavefronts without a finished env
 *     exit at once, the ray / aux kernels skip the others) re-initialises them, on the handle's stream(s) inside this call.
 *   FTL_STEP_NEXT_RESET or no flag: only fin->ended and fin->restarted are written (the final_* pointers may be NULL); under
 *     FTL_STEP_NEXT_RESET restarted marks the envs that were done on entry, ended the envs whose episode ended in this call.
 * Mission status FTL_MISSION_FINISHED_BY_TIME in the terminal status row is the reference's time limit (ENV:1126-1134): a truncation,
 * which a value bootstrap treats differently from the other statuses.  The reference checks the step limit after the frame's crash
 * tests, so an env that crashes in the frame that reaches max_steps reports FINISHED_BY_TIME as well. */
int ftl_step_final(ftl_handle* h, const void* action, int32_t encoding, const ftl_outputs* out, const ftl_final_outputs* fin,
                   uint32_t flags, void* stream);

/* ---- sensor scans on demand: step without them, scan without a step -----------------------------------------------------------------
 * A step is two halves: the frame kernel (plus ftl_tracker1_kernel for the v1 tracker) advances the world -- robots, collisions, tracker,
 * reward, done, obs_num, target --, then ftl_rays_kernel and ftl_aux_kernel turn the new state into `lasers` and `policy_obs`.  Nothing the
 * sensor kernels do feeds back into the state: they recompute every row of every history depth from the snapshots the state keeps.
 *
 * FTL_STEP_NO_SENSORS (ftl_step / ftl_step_encoded / ftl_step_final, alone or with any one reset flag): no pass of the call -- the step,
 * the reset pass of same-step / queue / sample, the restart of FTL_STEP_NEXT_RESET -- launches the two sensor kernels; every other launch
 * is the same.  `lasers` and `policy_obs` are not written and keep what they held (fin->lasers / fin->policy_obs are then copies of those
 * stale rows); every other output and every state word is bit-identical to the same call without the flag, except that a call that does
 * not scan cannot raise FTL_ERR_LIDAR_OVERFLOW (the one error bit a sensor kernel sets).
 *
 * ftl_scan is the other half: the sensor launches of a step on the current state of all envs and nothing else (no frame kernel, no
 * regroup).  It writes `lasers` (ray and aux blocks) and `policy_obs` when given -- the other arrays of `out` are checked as for a step
 * and not touched -- and is asynchronous on `stream`.  ftl_step*(flags | FTL_STEP_NO_SENSORS) followed by ftl_scan leaves outputs and
 * state as ftl_step*(flags) does (no flags, or FTL_STEP_AUTO_RESET without final buffers); after ftl_unpack_envs it reproduces the
 * readings the source env had when it was packed.  FTL_E_INVALID: NULL handle / out, output arrays missing; FTL_E_STATE without bound
 * state / scenarios. */
#define FTL_STEP_NO_SENSORS 32u
int ftl_scan(ftl_handle* h, const ftl_outputs* out, void* stream);

/* ftl_rollout: T steps of an open-loop action sequence with one call (planners: clone, roll out, restore, ftl_scan).  actions +
 * t * step_bytes is the action block of step t in `encoding` (row 0 = env 0 of this handle; the stride lets the parts of a pipelined batch
 * read their rows of one [T][N] array).  The envs are stepped exactly as T calls of ftl_step_encoded without auto-reset step them
 * (finished envs stay done and keep simulating); steps 0 .. T-2 run with FTL_STEP_NO_SENSORS, step T-1 scans unless `flags` carries
 * FTL_STEP_NO_SENSORS -- the only flag accepted.  After every frame launch ftl_rollout_fold_kernel folds out->reward / done / status into
 * `ro`: an env is alive in step t when its done word was 0 on entry to it (the step that raises done counts, later ones do not), and
 * ret = ret + disc_t * reward_t over those steps with disc_0 = 1, disc_{t+1} = disc_t * gamma, all in float64, one rounding per
 * operation.  `out` holds the outputs of step T-1.  FTL_E_INVALID before any device work: NULL pointers (a NULL field of `ro` included),
 * T <= 0, any other flag, an unknown encoding; FTL_E_STATE without bound state / scenarios. */
typedef struct ftl_rollout_outputs {  /* DEVICE pointers, every row written */
    double*  ret;     /* [n]    sum over the steps the env was alive in of disc_t * reward_t */
    int32_t* steps;   /* [n]    number of such steps: T if the episode never ended, 0 if the env was done on entry */
    uint8_t* status;  /* [n][3] status row of the step that ended the episode, 0/0/0 if none did */
} ftl_rollout_outputs;
size_t ftl_sizeof_rollout_outputs(void);
int ftl_rollout(ftl_handle* h, const void* actions, int64_t step_bytes, int32_t encoding, int32_t T, double gamma,
                const ftl_outputs* out, const ftl_rollout_outputs* ro, uint32_t flags, void* stream);

/* ---- baseline follower: the reference's way-point chase as a policy and as closed-loop rollouts -------------------------------------
 * run_2d.py --mode base (lines 109-151) drives the follower with MISC:65-95 (move_to_the_point) along a FIFO of the leader's target points.
 * Here the FIFO of every env lives in caller-owned DEVICE memory `bl`: n_envs rows of 16 + 16 * cap bytes, row e =
 * int32 {head, count, pending, flags} followed by cap points of two doubles used as a ring (front = point head, indices modulo cap).  A
 * row is self-contained -- copying row i to row j moves a follower, so followers can be cloned with their envs -- and a zeroed buffer is a
 * valid fresh state.  cap >= 2; `bl` 8-byte aligned.
 *
 * ftl_baseline_act (ftl_baseline_kernel, one thread per env, asynchronous on `stream`) reads what the last reset / step wrote to `out`
 * (obs_num[5], [6], [8] and target) and the env's step word, and per env:
 *   new episode   env_int[FTL_EI_STEP_COUNT] == 0 -- the env's rows of `out` are a reset observation, under every reset discipline, since
 *                 every step advances the word by at least one frame -- or count == 0 (zeroed row): FIFO = [target], pending cleared.
 *                 This is the only restart rule; there is no mask.
 *   otherwise     the bookkeeping of the step just taken, in the reference's order (run_2d.py:141-145): if target differs from the FIFO's
 *                 back (either coordinate, double ==, as np.array_equal) it is appended; then, if the previous decision left a pending
 *                 pop, the front is popped.
 *   decision      pos = (double)obs_num[5], [6]; cur = (int)obs_num[8]; desirable = (int)angle_to_point(pos, front) (MISC:16-26, the
 *                 float64 operation sequence of the frame kernel); delta_turn and the sign by the four branches of MISC:73-91;
 *                 action = (v, (double)(delta_turn * sign) / 10.0) with v = the euclidean distance pos -> front; pending = v <= 20.0.
 *                 The env clips the action as it clips any Box(2) action.
 * Two places where the reference cannot go on get a rule and a sticky bit in the row's flags word (no env error bit):
 *   FTL_BL_EMPTY     a pop that would empty the FIFO is not made, the follower keeps its last point (the reference raises IndexError on
 *                    its next iteration);
 *   FTL_BL_OVERFLOW  an append to a full FIFO drops the front (the reference's list is unbounded).
 * v: the reference's distance.euclidean is BLAS dnrm2 in x87 extended precision rounded to double; the device returns the correctly
 * rounded sqrt(dx^2 + dy^2) of the float64 differences (exact squares and sum, one final rounding).  A double rounding of the x87 path
 * can sit one ulp away (about 2^-12 of random inputs; counted in tests/test_baseline_host.py).  v matters to the env only below the
 * follower's max speed, i.e. within a few px of a point that is popped at 20 px.
 *
 * ftl_rollout_baseline is ftl_rollout with the action of step t produced on the stream: for t = 0 .. T-1 the act kernel, a step without
 * auto-reset (FTL_STEP_NO_SENSORS for t < T-1, `flags` -- FTL_STEP_NO_SENSORS or 0 -- for the last) and ftl_rollout_fold_kernel; a
 * two-stream handle is handled as ftl_rollout handles it.  actions == NULL: the actions go to an [n][2] scratch the handle owns;
 * otherwise block t is written at actions + t * step_bytes -- the record of what was played.  Precondition: `out` holds the observation
 * of the current state (the last reset / step / rollout on the handle wrote it).  It is bit-identical -- `out`, `ro`, every state byte,
 * every follower row -- to T iterations of ftl_baseline_act + ftl_step_encoded(FTL_ACTION_BOX2) + fold, and its env state and `ro` are
 * those of ftl_rollout on the recorded actions.
 * FTL_E_INVALID before any device work: NULL pointers, cap < 2, bl_bytes below ftl_baseline_bytes, `bl` not 8-byte aligned, T <= 0, any
 * flag but FTL_STEP_NO_SENSORS, step_bytes below one block when `actions` is given; FTL_E_STATE without bound state / scenarios.  The
 * action is Box(2): a config with discrete_action_space or constant_follower_speed decodes another encoding and has no use for it
 * (the Python wrapper refuses such a config). */
#define FTL_BL_EMPTY 1u
#define FTL_BL_OVERFLOW 2u
size_t ftl_baseline_bytes(const ftl_handle* h, int32_t cap);      /* n_envs rows of 16 + 16 * cap bytes; no device access; 0 on a NULL handle or cap < 2 */
int ftl_baseline_act(ftl_handle* h, const ftl_outputs* out, void* bl, size_t bl_bytes, int32_t cap,
                     double* action /* [n][2] */, void* stream);
int ftl_rollout_baseline(ftl_handle* h, int32_t T, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro,
                         void* bl, size_t bl_bytes, int32_t cap,
                         double* actions /* [T] blocks of [n][2], or NULL */, int64_t step_bytes,
                         uint32_t flags /* FTL_STEP_NO_SENSORS only */, void* stream);

/* ---- episode metrics + error report (ENV:941-944 reports overall_reward / step_count at done) --------
 * Every env slot accumulates, at the step in which an episode ends (done set by this step; under FTL_STEP_AUTO_RESET
 * before the slot is re-initialised), the vector below in its "ep_stats" state field (f64[FTL_N_METRICS] per env).
 * ftl_episode_metrics sums those records over the envs of the handle in a fixed order (bit-reproducible) into
 * dev_metrics[FTL_N_METRICS] (DEVICE pointer) -- the 64-byte vector a multi-GPU job all-reduces -- and reports the
 * sticky error words: dev_errors[0] = number of envs whose FTL_EI_ERROR_STICKY is non-zero, dev_errors[1] = OR of them
 * (DEVICE pointer, may be NULL).  FTL_METRICS_CLEAR zeroes the per-env records and sticky words afterwards. */
#define FTL_N_METRICS 8
enum { FTL_M_EPISODES = 0,   /* finished episodes */
       FTL_M_RETURN_SUM,     /* sum of overall_reward at done (ENV:943) */
       FTL_M_FRAMES_SUM,     /* sum of step_count at done, in frames (ENV:944) */
       FTL_M_SUCCESS,        /* mission_status == success at done */
       FTL_M_CRASH,          /* agent_status == crash */
       FTL_M_LOW_REWARD,     /* agent_status == low_reward */
       FTL_M_TOO_FAR,        /* agent_status == too_far_from_leader */
       FTL_M_TIMEOUT };      /* mission_status == finished_by_time */
#define FTL_METRICS_CLEAR 1u
int ftl_episode_metrics(ftl_handle* h, double* dev_metrics, int32_t* dev_errors, uint32_t flags, void* stream);

/* ---- measurement hook (bench.py): per-kernel durations from HIP events on the launch stream ------------------------------
 * While enabled every ftl_step records events around its launches (frame kernel, ray kernel, ftl_aux_kernel, the two regroup kernels);
 * ftl_kernel_times synchronises and returns the SUM of the durations in milliseconds since the last call as
 * ms[4] = {frames (+ the v1 tracker's kernel), rays, aux (row-f3 sensors; ~0 without them), regroup} and the number of steps they cover.  At most 512 steps are held; not available in the
 * two-stream mode (returns FTL_E_UNSUPPORTED).  Off by default: the events cost a few microseconds per step. */
int ftl_kernel_timing(ftl_handle* h, int32_t enable);
int ftl_kernel_times(ftl_handle* h, double* ms, int32_t* n_steps);

/* ---- batched top-down RGB frames (render(), ENV:1196-1202, layers of _show_tick ENV:1229-1281) --------------------------------
 * ftl_render draws k envs of the handle into rgb[k][height][width][3] (uint8, row-major [y][x][r, g, b]: the reference's
 * np.transpose(pygame.surfarray.array3d(.), (1, 0, 2))).  It reads the state, the scenario pool and the `lasers` output of the last
 * ftl_reset / ftl_step* / ftl_scan / ftl_rollout call on the handle (that buffer must still be alive) and writes nothing but `rgb` and the
 * caller's workspace: a render never changes a later step.  The SENSORS layer draws the readings of the last scan, which may be older than
 * the state (FTL_STEP_NO_SENSORS, ftl_unpack_envs).  env_ids are env indices of the handle (not slots of its cost-sorted permutation); repeats are
 * allowed; an id outside [0, n_envs) gives a white frame.  Asynchronous on `stream`.
 *
 * Coverage rules (what a pixel shows).  Output pixel (i, j) samples the world point origin + (i + 0.5, j + 0.5) * scale.  Positions
 * and radii scale; stroke widths w do not: they are max(w / scale, 1) output pixels.  In output pixels:
 *   disc:      distance d to the centre <= r;           ring of width w: r - w < d <= r;
 *   segment:   distance to the segment (round ends) <= w / 2;
 *   rotated rectangle (centre c, unit axes u, v = u rotated by +90 deg, half sizes hw, hh): |dot(p - c, u)| <= hw && |dot(p - c, v)| <= hh;
 *   outline of an integer rect (x, y, w, h): the points inside [x, x + w) x [y, y + h) that lie within one output pixel of its border
 *              (at scale 1 and origin 0 exactly pygame.draw.rect(width=1)'s pixels).
 * The last primitive in painter's order that covers a pixel sets its colour; there is no anti-aliasing; uncovered pixels are white.
 * A pixel centre exactly on a boundary follows the <= / < of the rule; these rules are met wherever the centre is farther than 1e-3
 * output pixels from every boundary, and inside that band the float32 arithmetic may decide either way.  Range of that guarantee: a
 * primitive is stored as float32 output-pixel coordinates and tested in float32 (no fused multiply-add), so with u = 2^-24 every rounding
 * moves a distance by at most u M, M being the largest magnitude among the primitive's output-pixel coordinates (centre, end points,
 * corners, relative to the image's origin) and sizes (radius, half sizes).  The longest chain, the segment's closest point, has 8 such
 * roundings (2 stored end points, the edge vector, the product and the sum of the closest point, its square, the sum of squares, the
 * squared half width): 8 u M <= 1e-3 holds up to M = 2048 output pixels, and that is the guaranteed range.  Zooming in (scale < 1) grows
 * M as world size / scale: a primitive beyond the range that meets the image may be off by more than the band along its boundary
 * (a float32 emulation of the tests finds the first such pixels at M = 32768; tests/test_render_numpy_host.py, profiles/render_edges_checks.txt).
 *
 * Painter's order (layer bits below; FTL_RENDER_TARGET stands for the ring the reference always draws):
 *   PATH     the route (pool route[0..route_len)) as a 1-px red polyline when route_len > 2; the bridge point (mean of the centres of
 *            the two bridge-wall rects = static rects 0 and 1, present when n_static >= 2) as a black disc of r 5; the finish point (the
 *            route's last way-point) as a red disc of r 5.  finish_point2 / 3 of multiple_end_points are not in the pool: not drawn.
 *   BOX      a green disc of r max_dev at each green-zone point when there are more than 5: the reference's green_zone_trajectory_points
 *            (ENV:1828-1841), built in the last frame before that frame's trajectory append (ENV:968-969, 1074-1075) = trajectory points
 *            green_len - 2 down to green_len - 1 - green_count (FTL_EI_GREEN_LEN: the trajectory length the window was built on); then
 *            the red ring of r min_distance around the leader, width 2 when FTL_EI_TOO_CLOSE is set, else 1.
 *   OBJECTS  leader, follower, the static rects (bridge walls, rocks), then the bears (game_object_list, game_dynamic_list): a robot is a
 *            rectangle img_w x img_h centred on its f32 position, u = (cos, sin) of its direction; a static rect is the filled
 *            axis-aligned rect.  RECTS adds the 1-px red outline of the object's hitbox (rb_int / the static rect) right after each
 *            body, so RECTS draws nothing without OBJECTS (show_object, ENV:1217-1227).
 *   SENSORS  in dict order (the ray sensors with after_tracker = 0, the v2 tracker, the others).  A ray sensor draws 1-px lines from the
 *            follower to the end points at laser_length, then discs at the collide points: the follower plus a row's reading along the
 *            ray (the hit, or the end point without one).  LeaderCorridor_lasers / _v2 (explicit_angles or lenient, SEN:728-733): one
 *            r-5 disc per ray from the newest row, lines and discs in FTL_RGB_RAY_V2.  The others (SEN:970-985): per output row, oldest
 *            first, a disc per ray, r 3 in FTL_RGB_RAY_HIT_OLD for the older rows and r 5 in FTL_RGB_RAY_HIT for the newest.  Compas
 *            sensors draw their lines only.  The v2 tracker draws its history points (discs of r 3) and, with more than one corridor
 *            point, the two corridor borders and the two end caps as 3-px segments (sensors.py:329-339).  The v1 tracker and the aux
 *            sensors draw nothing.
 *   TARGET   a red ring of r 10, width 2 at the current way-point route[cur_target_id] (the leader's start with an empty route).
 * State words outside their range are clamped, never followed out of an array: route_len to [0, route_cap], cur_target_id to
 * [0, route_len - 1], the corridor window to max(0, min(FTL_EI_CORR_HI - FTL_EI_CORR_LO, corr_cap)) points from slot FTL_EI_CORR_LO modulo
 * corr_cap; the green zone is drawn only when green_count > 5, green_len <= traj_cap and green_len - 1 - green_count >= 0.  An env
 * whose scenario index FTL_EI_SCEN lies outside the loaded pool has no pool entry to read: no route and no finish point, no static rects
 * and no bridge point, and the TARGET ring around the leader's current position; everything else is drawn as usual. */
enum { FTL_RENDER_PATH = 1, FTL_RENDER_BOX = 2, FTL_RENDER_OBJECTS = 4, FTL_RENDER_RECTS = 8,
       FTL_RENDER_SENSORS = 16, FTL_RENDER_TARGET = 32 };
#define FTL_RENDER_ALL 63u
/* colours, 0xRRGGBB: the reference's colours dict (ENV:206-214) and sensor show() colours; body colours per object class stand in for
 * the sprites */
#define FTL_RGB_WHITE 0xFFFFFFu
#define FTL_RGB_BLACK 0x000000u
#define FTL_RGB_RED 0xFF0000u
#define FTL_RGB_GREEN 0x00FF00u
#define FTL_RGB_LEADER 0x0000FFu
#define FTL_RGB_FOLLOWER 0xFF8C00u
#define FTL_RGB_WALL 0x1E1E1Eu
#define FTL_RGB_ROCK 0x808080u
#define FTL_RGB_BEAR 0x8B4513u
#define FTL_RGB_RAY 0xC86464u        /* (200, 100, 100), SEN:971 */
#define FTL_RGB_RAY_HIT 0xC81440u    /* (200, 20, 64), SEN:981 */
#define FTL_RGB_RAY_HIT_OLD 0xFF4B6Eu /* (255, 75, 110), SEN:984 */
#define FTL_RGB_RAY_V2 0xC80064u     /* (200, 0, 100): LeaderCorridor_lasers_v2 (lenient), SEN:728-733 */
#define FTL_RGB_TRACK_HIST 0x500A0Au /* (80, 10, 10), sensors.py:331 */
#define FTL_RGB_CORRIDOR 0x967832u   /* (150, 120, 50), sensors.py:336-339 */
typedef struct ftl_render_params {
    int32_t  width, height;      /* output image size, pixels */
    float    scale;              /* world pixels per output pixel (> 0) */
    float    origin_x, origin_y; /* world coordinate of the top-left corner of output pixel (0, 0) */
    uint32_t layers;             /* FTL_RENDER_* bits */
    int32_t  _pad;
} ftl_render_params;
size_t ftl_sizeof_render_params(void);
/* device workspace ftl_render needs for k envs (owned by the caller, reusable across calls of the same k) */
int ftl_render_workspace(const ftl_handle* h, int32_t k, size_t* bytes);
/* FTL_E_INVALID before any device work: k <= 0, width / height <= 0, scale <= 0 or not finite, unknown layer bits, NULL pointers,
 * a workspace below ftl_render_workspace; FTL_E_STATE without bound state / scenarios. */
int ftl_render(ftl_handle* h, const int32_t* env_ids, int32_t k, const ftl_render_params* rp, void* workspace, size_t workspace_bytes,
               uint8_t* rgb, void* stream);

/* ---- snapshot, clone and restore of env states (ALE cloneState / restoreState, copy.deepcopy of the reference's Game) ----------------
 * A packed env row holds everything of one env that the state buffer stores, so that unpacking it into any slot of any handle with the
 * same layout id continues the env's episode bit for bit (with the same actions and the same scenario pool):
 *   row = [record][traj][hist][corr][traj_bb][ep_stats][hist1][corr32][zero padding to ftl_env_bytes]
 *   record: the bytes of the per-env record that hold its fields (env_int, fol_cs, rb_pos, rb_dbl, snap_win, snap_rects, env_dbl, rb_int
 *           at their ftl_state_field offsets; the record's tail padding up to its stride is not stored); then every dense field in
 *           ftl_state_field order, each at a 16-byte aligned row offset, its gap zero-filled; a field with per_env 0 takes no bytes.
 *   The whole trajectory (traj_cap points) and every block box are stored, not only the live prefix.
 *   Stream rule: word FTL_EI_STREAM of the row's env_int holds the ABSOLUTE global stream id (env_id_base + env + offset of the source);
 *           unpacking into slot `dst` stores id - env_id_base - dst, so the env keeps drawing from its source's stream in any slot,
 *           handle or shard layout.
 * ftl_env_bytes: bytes of one row (a multiple of 256).  ftl_env_layout_id: 64-bit hash of the frozen config without n_envs and
 * env_id_base, of FTL_ABI_VERSION and of the row format; rows move only between handles with equal ids.  Neither touches the device.
 * ftl_pack_envs copies envs env_ids[0..k) into rows[k][ftl_env_bytes] (DEVICE pointers; rows 16-byte aligned).  ftl_unpack_envs copies
 * rows[i] into env env_ids[i]; env_ids must be distinct, rows must not overlap the state buffer.  By default the destination keeps what
 * belongs to its slot rather than to the episode -- its "ep_stats" record and its FTL_EI_EPISODES / FTL_EI_ERROR_STICKY words -- so that
 * ftl_episode_metrics counts every episode once; FTL_ENV_SLOT_STATS moves them too (checkpoints).  FTL_ENV_OWN_STREAM keeps the
 * destination's FTL_EI_STREAM word (the copy then draws from the destination's own stream and diverges from its source on the first
 * random draw).  Ids are not range-checked on the device (the caller checks them, as for ftl_reset's scenario indices).  Rejected with
 * FTL_E_INVALID before any device work: k < 0, NULL pointers with k > 0, rows not 16-byte aligned, unknown flag bits; FTL_E_STATE
 * without bound state.  k == 0 does nothing.  Asynchronous on `stream`; the outputs (obs, lasers, ...) are the caller's to copy
 * (ftl_scan recomputes `lasers` / `policy_obs` of the unpacked state). */
#define FTL_ENV_SLOT_STATS 1u  /* also move ep_stats, FTL_EI_EPISODES, FTL_EI_ERROR_STICKY (checkpoints); default: dst keeps its own */
#define FTL_ENV_OWN_STREAM 2u  /* dst keeps its own random stream instead of the row's */
size_t   ftl_env_bytes(const ftl_handle* h);
uint64_t ftl_env_layout_id(const ftl_handle* h);
int ftl_pack_envs(const ftl_handle* h, const int32_t* env_ids, int32_t k, void* rows, void* stream);
int ftl_unpack_envs(ftl_handle* h, const void* rows, const int32_t* env_ids, int32_t k, uint32_t flags, void* stream);
/* ftl_unpack_envs with rows[row_ids[i]] in place of rows[i] (row_ids [k] DEVICE, repeats allowed, not range-checked): one packed row fanned
 * out into many slots without a k-row copy of it.  row_ids == NULL is ftl_unpack_envs (the same kernel). */
int ftl_unpack_envs_from(ftl_handle* h, const void* rows, const int32_t* row_ids, const int32_t* env_ids, int32_t k, uint32_t flags,
                         void* stream);

/* ---- action search: K candidate action sequences per env, rolled out on clones, the best one kept (random shooting with a shrinking
 * radius) ------------------------------------------------------------------------------------------------------------------------------
 * Two handles with equal ftl_env_layout_id on one device, used on one stream, with the same scenario pool loaded: the REAL handle of n
 * envs and the SEARCH handle of n * K envs, whose env e * K + k is candidate k of real env e.  One ftl_search call is enqueued on `stream`
 * without a host synchronisation:
 *   1. ftl_pack_envs of the n real envs (b->env_ids[0 .. n)) into b->rows.
 *   2. begin (ftl_search_begin_kernel, one thread per env): if word FTL_EI_STEP_COUNT of the env's row is 0 (a new episode: the baseline
 *      follower's rule), or call == 0, or warm == 0, nominal[t][e] = (follower.max_speed, 0.0) for every t; otherwise nominal[t][e] =
 *      nominal[t + 1][e] for t < T - 1 and the last step is kept (the plan of the last call, one step later).
 *   3. for it = 0 .. iters - 1, with the radius s_0 = spread, s_{it+1} = s_it * decay (host, float64):
 *      sample  (ftl_search_sample_kernel, one thread per (t, clone)): cand[t][e * K][j] = nominal[t][e][j] exactly (candidate 0 is the
 *              incumbent); for k > 0 x = nominal[t][e][j] + (s * (u - 0.5)) * (hi_j - lo_j), cand = fmin(fmax(x, lo_j), hi_j) with
 *              u = ftl_search_uniform(p->seed, stream_e, call, it, k, t / hold, j) and (lo, hi) the Box(2) bounds of ENV:374-378:
 *              (follower.min_speed, -follower.max_rotation_speed), (follower.max_speed, follower.max_rotation_speed).  Float64, this
 *              operation order, one rounding per operation.  stream_e is the ABSOLUTE stream id the row carries at FTL_EI_STREAM, so the
 *              candidates follow an env through clone, restore and re-sharding and do not depend on its slot.
 *      fan-out ftl_unpack_envs_from(search, rows, row_ids, env_ids, n * K, FTL_ENV_OWN_STREAM under FTL_SEARCH_OWN_STREAM else 0).
 *      rollout ftl_rollout(search, cand, ..., FTL_ACTION_BOX2, T, gamma, FTL_STEP_NO_SENSORS) into b->ro: ret[n * K].
 *      select  (ftl_search_select_kernel, one wavefront per env): k* = the candidate with the largest ret, the lowest k among equals (-0.0
 *              equals 0.0); best_k[e] = k*, best_ret[e] = ret[e * K + k*], nominal[t][e] = cand[t][e * K + k*] for every t.  ret is
 *              assumed free of NaN.
 *   4. action[e] = nominal[0][e] (a device copy).
 * Buffers (ftl_search_buffers; all DEVICE memory the caller owns, alive until the stream has passed the call): rows [n][ftl_env_bytes],
 * 16-byte aligned; row_ids / env_ids [n * K] int32, filled by the CALLER with row_ids[i] = i / K and env_ids[i] = i and only read here;
 * nominal [T][n][2], cand [T][n * K][2], action [n][2], best_ret [n] float64; best_k [n] int32; out / ro: the search handle's step and
 * rollout outputs.  nominal carries the plan from call to call; everything else is scratch or result.
 * Properties:
 *   - The real handle is only read (the one ftl_pack_envs): its state and outputs are byte-identical before and after.
 *   - Without FTL_SEARCH_OWN_STREAM a clone keeps its source's random stream, so it is the real env's exact future under the same actions:
 *     best_ret is non-decreasing over the rounds of a call (candidate 0 is the incumbent), and ftl_rollout of `nominal` on the real handle
 *     returns best_ret bit for bit.  It also means that the search SEES THE FUTURE random draws of the env (the leader's speed regime
 *     draws, random frames per step, bear way-points): it plans against the world as it will be, not as a model of it.
 *     FTL_SEARCH_OWN_STREAM is the honest-model switch: every clone draws from its own slot's stream, best_ret is an estimate, and
 *     neither property above holds.
 *   - A real env that is done on entry gives ret = 0 for every clone, hence best_k = 0 and the nominal action.
 *   - Limits of the draw key: T / hold < 65536, iters < 128, K < 2^19.
 * FTL_E_INVALID before any device work: NULL pointers (any field of b, out, ro), K / T / hold / iters < 1 or beyond the limits, spread or
 * decay outside (0, 1], gamma not finite, unknown flag bits, layout ids that differ, devices that differ, search handle size != n * K,
 * n * K beyond INT32_MAX, rows / nominal / cand not 16-byte aligned; FTL_E_STATE: no bound state or no scenario pool on either handle.
 * ftl_search_begin / _sample / _select are the three kernels on plain buffers (the pieces of the sequence above, for callers with a
 * candidate generator of their own); `h` gives the row layout, the Box and the device.  `s` is the round's radius in [0, 1] (0: every candidate is the nominal). */
#define FTL_SEARCH_OWN_STREAM 1u
typedef struct ftl_search_params {
    int32_t K, T, hold, iters;      /* candidates per env, horizon in steps, steps per drawn action, refinement rounds; all >= 1 */
    double  gamma, spread, decay;   /* discount of ftl_rollout; radius as a share of the Box width, 0 < spread <= 1; 0 < decay <= 1 */
    uint64_t seed;
    uint32_t flags;                 /* FTL_SEARCH_OWN_STREAM: clones draw from their own streams (FTL_ENV_OWN_STREAM) */
    int32_t _pad;
} ftl_search_params;
typedef struct ftl_search_buffers {
    void*    rows;                  /* [n][ftl_env_bytes] */
    const int32_t* row_ids;         /* [n * K]  i / K */
    const int32_t* env_ids;         /* [n * K]  i */
    double*  nominal;               /* [T][n][2] */
    double*  cand;                  /* [T][n * K][2] */
    double*  action;                /* [n][2] */
    int32_t* best_k;                /* [n] */
    double*  best_ret;              /* [n] */
    const ftl_outputs* out;         /* of the search handle */
    const ftl_rollout_outputs* ro;  /* of the search handle */
} ftl_search_buffers;
size_t ftl_sizeof_search_params(void);
size_t ftl_sizeof_search_buffers(void);

/* The draw of candidate k > 0 of the env on stream `stream_id` in round `it` of call `call`: coordinate j (0 speed, 1 rotation) of hold
 * block `block` = t / hold, on the counter stream of ftl_uniform01 in a key range of its own (bit 43 of the frame key). */
static inline double ftl_search_uniform(uint64_t seed, uint64_t stream_id, uint64_t call, uint32_t it, uint32_t k, uint32_t block, uint32_t j) {
    return ftl_uniform01(seed, stream_id, call, (1ULL << 43) | block | ((uint64_t)j << 16) | ((uint64_t)it << 17) | ((uint64_t)k << 24));
}

int ftl_search_begin(const ftl_handle* h, const void* rows, int32_t n, int32_t T, uint64_t call, int32_t warm, double* nominal, void* stream);
int ftl_search_sample(const ftl_handle* h, const void* rows, int32_t n, const ftl_search_params* p, uint64_t call, int32_t it, double s,
                      const double* nominal, double* cand, void* stream);
int ftl_search_select(const ftl_handle* h, const double* ret, int32_t n, int32_t K, int32_t T, const double* cand, double* nominal,
                      int32_t* best_k, double* best_ret, void* stream);
int ftl_search(const ftl_handle* real, ftl_handle* search, const ftl_search_params* p, uint64_t call, int32_t warm,
               const ftl_search_buffers* b, void* stream);

/* ---- guided search: the action search over RESIDUALS added to the baseline follower's own closed-loop action, scored over a horizon that
 * ends in a closed-loop baseline tail ----------------------------------------------------------------------------------------------------
 * ftl_baseline_act_guided (ftl_baseline_guided_kernel) is ftl_baseline_act with one more input, resid (DEVICE, [n][2] float64, 8-byte
 * aligned): the follower-row bookkeeping and the decision are those of ftl_baseline_kernel bit for bit (one __device__ function), and with
 * base = the baseline's raw action (v, w) the written action is
 *     a_j = fmin(fmax(fmin(fmax(base_j, lo_j), hi_j) + r_j, lo_j), hi_j)
 * in float64, this operation order, one rounding per operation, (lo, hi) the Box(2) bounds of ftl_search_sample.  The raw action is clipped
 * FIRST: it is almost always saturated (v is a distance in pixels, the turn is in tenths of degrees), so a residual added before the clip
 * would do nothing.  The env clips with the same bounds, so a zero residual steps the env exactly as the unclipped baseline action does.
 *
 * ftl_rollout_guided is ftl_rollout_baseline over T + tail steps whose first T decisions are guided: for t < T the guided act kernel with
 * resid + t * resid_step_bytes, for T <= t < T + tail the plain ftl_baseline_kernel; after each a step without auto-reset and
 * ftl_rollout_fold_kernel, the discount running on across both parts (disc_{t+1} = disc_t * gamma).  All steps but the last run with
 * FTL_STEP_NO_SENSORS, the last with `flags`; a two-stream handle, `actions` / step_bytes (the record of what was played, T + tail blocks)
 * and the precondition on `out` are those of ftl_rollout_baseline.  resid == NULL is ftl_rollout_baseline(T + tail).  FTL_E_INVALID before
 * any device work: what ftl_rollout_baseline refuses, T < 1, tail < 0, resid_step_bytes below one block of [n][2] doubles, resid or
 * resid_step_bytes not 8-byte aligned; FTL_E_STATE without bound state / scenarios.
 *
 * ftl_guided_fanout (ftl_guided_fanout_kernel) gives clone i = e * K + k of the search handle what ftl_unpack_envs_from does not carry: the
 * real follower row e (16 + 16 * cap bytes) -> follower row i of search_bl, and rows e of real_out->obs_num (FTL_OBS_NUM floats) and
 * real_out->target (two doubles) -> rows i of search_out.  After ftl_unpack_envs_from a clone's first decision then reads the observation
 * its source had.  Nothing else is written.  16-byte loads and stores, both follower buffers 16-byte aligned.  FTL_E_INVALID: NULL
 * pointers, cap < 2, a follower buffer below its handle's ftl_baseline_bytes or misaligned, search handle size != n * K, another device,
 * source and destination the same buffer.
 *
 * ftl_search_guided: the two handles of ftl_search, one call enqueued on `stream` without a host synchronisation:
 *   1. ftl_pack_envs of the n real envs.
 *   2. begin: ftl_search_begin_kernel with the default plan (0, 0) in place of (max_speed, 0) -- the zero residual, i.e. the baseline itself;
 *      the new-episode rule and the warm shift are those of ftl_search.  nominal [T][n][2] is the RESIDUAL plan.
 *   3. for it = 0 .. iters - 1 (radius as in ftl_search):
 *      sample  ftl_search_sample_kernel on the residual box [-(hi_j - lo_j) / 2, +(hi_j - lo_j) / 2]: its width is the action Box's, so the
 *              formula and the draws of ftl_search_uniform carry over; candidate 0 is the incumbent residual plan.
 *      fan-out ftl_unpack_envs_from as in ftl_search, then ftl_guided_fanout.
 *      rollout ftl_rollout_guided(search, T, tail, gamma, out, ro, search_bl, ..., resid = cand, FTL_STEP_NO_SENSORS).
 *      select  ftl_search_select_kernel.
 *   4. ftl_baseline_act_guided on the REAL handle with resid = nominal[0], writing `action`: it books the real follower's step exactly once,
 *      as one ftl_baseline_act per step does, and comes last so that every round fans out the follower rows as they were before it.
 * Properties (clones on their source's stream): candidate 0 of a call that starts from the default plan is the baseline itself, so best_ret
 * is never below the baseline's return over T + tail steps, bit for bit equal for K = 1; best_ret is non-decreasing over the rounds;
 * ftl_rollout_guided of `nominal` on the real handle from the same state and a copy of the follower rows returns best_ret bit for bit.
 * The real handle's state and outputs are only read; its follower rows and `action` are written by step 4 alone.
 * FTL_E_INVALID before any device work: what ftl_search refuses, tail < 0, a NULL field of gb, cap < 2, a follower buffer below its
 * handle's ftl_baseline_bytes or not 16-byte aligned; FTL_E_STATE as ftl_search.  FTL_SEARCH_OWN_STREAM means what it means there. */
typedef struct ftl_guided_buffers {
    void*    rows;                  /* the fields of ftl_search_buffers, as there; nominal and cand hold residuals */
    const int32_t* row_ids;
    const int32_t* env_ids;
    double*  nominal;
    double*  cand;
    double*  action;                /* [n][2] the action to play: clip(clip(base) + nominal[0]) */
    int32_t* best_k;
    double*  best_ret;
    const ftl_outputs* out;         /* of the search handle */
    const ftl_rollout_outputs* ro;  /* of the search handle */
    const ftl_outputs* real_out;    /* of the real handle: what its last reset / step wrote */
    void*    real_bl;               /* [n] follower rows of the real envs */
    size_t   real_bl_bytes;
    void*    search_bl;             /* [n * K] follower rows of the clones (scratch) */
    size_t   search_bl_bytes;
    int32_t  cap;
    int32_t  _pad;
} ftl_guided_buffers;
size_t ftl_sizeof_guided_buffers(void);
int ftl_baseline_act_guided(ftl_handle* h, const ftl_outputs* out, void* bl, size_t bl_bytes, int32_t cap,
                            const double* resid /* [n][2] */, double* action /* [n][2] */, void* stream);
int ftl_rollout_guided(ftl_handle* h, int32_t T, int32_t tail, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro,
                       void* bl, size_t bl_bytes, int32_t cap,
                       const double* resid /* [T] blocks of [n][2], or NULL */, int64_t resid_step_bytes,
                       double* actions /* [T + tail] blocks of [n][2], or NULL */, int64_t step_bytes,
                       uint32_t flags /* FTL_STEP_NO_SENSORS only */, void* stream);
int ftl_guided_fanout(const ftl_handle* real, const ftl_handle* search, int32_t K, const ftl_outputs* real_out, const ftl_outputs* search_out,
                      const void* real_bl, size_t real_bl_bytes, void* search_bl, size_t search_bl_bytes, int32_t cap, void* stream);
int ftl_search_guided(ftl_handle* real, ftl_handle* search, const ftl_search_params* p, uint64_t call, int32_t warm, int32_t tail,
                      const ftl_guided_buffers* gb, void* stream);

/* ---- MLP policy population: a dense feed-forward net, or one net per block of envs, as a policy and as closed-loop rollouts ----------
 * The consumer of ftl_outputs.policy_obs on the device: ftl_mlp_act (ftl_mlp_kernel, csrc/ftl_mlp.hpp, one launch, asynchronous on
 * `stream`) reads every env's policy_obs row and writes its action in the encoding the head width implies; ftl_rollout_mlp closes the
 * loop over T steps with one call.  The arithmetic is fixed operation by operation, so the device equals a numpy twin bit for bit
 * (tests/mlp_numpy.py).
 *
 * Net         L = n_layers layers, 1 <= L <= FTL_MLP_MAX_LAYERS; widths width[0 .. L], width[0] the input and width[L] the head width;
 *             width[0] in 1 .. FTL_MLP_MAX_IN, every other width in 1 .. FTL_MLP_MAX_WIDTH.  L = 1 is a linear policy.  Beyond these
 *             limits: FTL_E_UNSUPPORTED before any device work.
 * Parameters  float32 in DEVICE memory, 4-byte aligned: n_sets >= 1 sets, set s at params + s * set_stride (in floats).  One set holds,
 *             layer by layer (l = 1 .. L), W_l as [width[l-1]][width[l]] row-major (input index outer) followed by b_l[width[l]]:
 *             ftl_mlp_param_count(width, L) = sum_l (width[l-1] + 1) * width[l] floats; set_stride >= that.
 * Input       x = env e's policy_obs row flattened, [H][W] -> H * W float32; width[0] must equal H * W of the handle.
 * Neuron j of layer l is a k-ordered float32 fused chain that starts at the bias:
 *                 acc = b[j];  for k = 0 .. width[l-1] - 1:  acc = fmaf(x[k], W[k][j], acc)
 *             one rounding per step, no split-K, no tree, no wider accumulator; f32 subnormals are kept.  Hidden layers (l < L) then apply
 *             acc > 0 ? acc : 0.0f, which maps NaN and -0 to +0.  The head layer (l = L) has no activation: y_j = acc.
 * Activation  ftl_mlp.activation chooses the hidden layers' function for the whole net: FTL_MLP_ACT_RELU (0, what a zeroed struct has
 *             always meant) is the line above; FTL_MLP_ACT_TANH (1) is h_j = tanh32(acc_j), tanh32 exactly the float32 operation
 *             sequence of csrc/ftl_rnn_math.hpp that the ftl_rnn_act block below spells out (tests/mlp_tanh_numpy.py is the twin).  acc_j
 *             is the same chain; the head stays linear, and its maps, the noise rules of ftl_mlp_sample and the weight sets are
 *             untouched.  What differs from ReLU: -0 stays -0 (copysignf); tanh32 returns 0 for |acc| up to 2^-26 (e rounds to 1.0f: the
 *             accepted cancellation; its smallest nonzero result is 2^-25, about 3e-8) and exactly +/-1 from |acc| = 8.66434 on
 *             (1.0f - e rounds to 1.0f), infinities included; a NaN pre-activation stays NaN, spreads through the next chain and reaches the head, where the float64
 *             fmin(fmax(..)) of a Box head sends it to lo and a Discrete(5) NaN never wins.  Any other value of `activation`:
 *             FTL_E_INVALID before any device work, with a message that names `activation`, from ftl_mlp_act, ftl_mlp_sample,
 *             ftl_rollout_mlp and ftl_collect_mlp alike.  (ftl_mlp_tanh_kernel and ftl_mlp_sample_tanh_kernel: the same body compiled
 *             with the other epilogue; the ReLU kernels are the instantiations they were.)
 * Heads       lo / hi are the bounds of the config's action Box (follower.min_speed / max_speed for the speed, -/+ max_rotation_speed for the
 *             rotation: those of ftl_search_sample and of the env's own clip).  Every operation below is one float64 rounding, fmin / fmax as
 *             in C (a NaN operand yields the other one):
 *   width[L] = 2  FTL_ACTION_BOX2      u = fmin(fmax((double)y_j, -1.0), 1.0);  a_j = lo_j + ((u + 1.0) * 0.5) * (hi_j - lo_j);
 *                                      a_j = fmin(fmax(a_j, lo_j), hi_j); j = 0 the speed, j = 1 the rotation; written as f64 [n][2].
 *   width[L] = 1  FTL_ACTION_TURN      the same map of y_0 with the rotation bounds (Box(1) of constant_follower_speed); f64 [n].
 *   width[L] = 5  FTL_ACTION_DISCRETE  k = 0; for j = 1 .. 4: if (y_j > y_k) k = j -- the first maximum; a NaN never beats anything; int32 [n].
 *             Any other head width: FTL_E_INVALID.  (The handle does not know which action space the caller's config declares: the head
 *             width chooses the encoding, and the Python wrapper refuses a head that does not fit the config.)
 * Weight set  env e of the handle uses set (env_first + e) / envs_per_set: contiguous equal blocks of the WHOLE batch, env_first being the
 *             handle's first env in it (0 for a lone handle, the part's first row for a part of a pipelined batch), so a set may straddle
 *             two parts.  (env_first + n_envs - 1) / envs_per_set < n_sets, else FTL_E_INVALID.  A workgroup's tile of envs never crosses a
 *             set boundary, so it stages one set's weights.
 *
 * ftl_rollout_mlp is ftl_rollout with the action of step t produced on the stream by the act kernel from the policy_obs step t - 1 (or
 * the last reset / step / scan) wrote: T steps without auto-reset, EVERY one of them with its sensor kernels -- the next decision reads
 * them -- each followed by ftl_rollout_fold_kernel.  flags must be 0: FTL_STEP_NO_SENSORS would blind the policy and is refused with a
 * message that says so.  actions == NULL: the actions go to a scratch the handle owns; otherwise block t (in the head's encoding: 16, 8 or
 * 4 bytes per env) is written at actions + t * step_bytes.  It is bit-identical -- `out`, `ro`, every state byte -- to T iterations of
 * ftl_mlp_act + ftl_step_encoded + fold, and its env state and `ro` are those of ftl_rollout on the recorded actions.
 * FTL_E_INVALID before any device work: NULL pointers, out->policy_obs NULL (or a handle whose config has no sensor for it),
 * width[0] != H * W, params not 4-byte aligned, set_stride below the param count, n_sets < 1, envs_per_set < 1, env_first < 0, a set index
 * out of range, a head width other than 1 / 2 / 5, T <= 0, any flag, step_bytes below one block when `actions` is given; FTL_E_STATE as for
 * the baseline. */
#define FTL_MLP_MAX_LAYERS 4
#define FTL_MLP_MAX_WIDTH 256
#define FTL_MLP_MAX_IN 4096
#define FTL_MLP_ACT_RELU 0             /* ftl_mlp.activation */
#define FTL_MLP_ACT_TANH 1
typedef struct ftl_mlp {
    const float* params;       /* DEVICE, [n_sets] sets of set_stride floats */
    int64_t  set_stride;       /* floats between two sets */
    int32_t  n_sets;
    int32_t  n_layers;
    int32_t  width[FTL_MLP_MAX_LAYERS + 1];
    int32_t  env_first;        /* index of the handle's env 0 in the whole batch */
    int32_t  envs_per_set;
    int32_t  activation;       /* FTL_MLP_ACT_*: the hidden layers (where _pad was: 0 is ReLU) */
} ftl_mlp;
size_t ftl_sizeof_mlp(void);
int64_t ftl_mlp_param_count(const int32_t* widths, int32_t n_layers);   /* floats of one set; -1 outside the limits above or on NULL */
int ftl_mlp_act(ftl_handle* h, const ftl_outputs* out, const ftl_mlp* net, void* action, void* stream);
int ftl_rollout_mlp(ftl_handle* h, int32_t T, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro, const ftl_mlp* net,
                    void* actions /* [T] blocks in the head's encoding, or NULL */, int64_t step_bytes, uint32_t flags /* 0 */, void* stream);

/* ---- policy-gradient trajectories: stochastic decisions, T recorded closed-loop steps through episode boundaries, advantages ---------
 * What a gradient method (the reference trains its followers with PPO) needs of the device: ftl_mlp_sample is ftl_mlp_act with
 * exploration and a record of what it read and computed, ftl_collect_mlp plays T such decisions with one call and leaves the trajectory
 * on the device, ftl_gae turns rewards, episode boundaries and the caller's values into advantages and value targets.  The backward
 * pass is the caller's (torch autograd on the recorded tensors).  No transcendental function runs on the device, so the numpy twin
 * (tests/collect_numpy.py) stays exact.
 *
 * ftl_mlp_sample (ftl_mlp_sample_kernel, csrc/ftl_mlp.hpp: the body of ftl_mlp_kernel, one launch, one decision).  The net, the layers
 * and the checks are those of ftl_mlp_act; it differs in three places, each optional by pointer (NULL: left out):
 *   obs_rec   float32 [n][width[0]]: while the first layer stages its chunk of the tile's policy_obs rows, the same threads store the same
 *             floats here -- the row is read once and written once, there is no copy kernel.
 *   head_rec  float32 [n][width[L]]: y_j = acc of the head layer, before any map.
 *   noise     float32 [n][width[L]], the caller's draws (row 0 = env 0 of the handle); sigma float32 [n_sets][width[L]], DEVICE memory (a
 *             learnable log_std.exp() costs no host synchronisation), indexed by the env's weight set.  Every operation is one float64
 *             rounding (the unit is built with -ffp-contract=off):
 *     Box heads (width 2 and 1)  z = (double)y_j + (double)sigma_j * (double)noise_j -- the product of two float32 is exact in float64 --,
 *                                u = fmin(fmax(z, -1.0), 1.0), and the rest of the head map of ftl_mlp_act unchanged.
 *     Discrete(5)                s_j = (double)y_j + (double)noise_j: the caller's Gumbel draw; sigma is ignored.  k = 0; for j = 1 .. 4:
 *                                if (s_j > s_k) k = j -- the first maximum, a NaN never beats anything.
 *     noise == NULL              bit for bit the action of ftl_mlp_act (as is a noise of zeros with a finite sigma).
 *   The log-probability of what was played needs no kernel.  Box heads: the action is a deterministic map of z, and under the Gaussian
 *   z ~ N(y, sigma^2) the density of the draw is logp = sum_j (-0.5 * noise_j^2 - log(sigma_j) - 0.5 * log(2 * pi)); with new parameters
 *   the same draw is z_j = head_j + sigma_j * noise_j of the RECORD and logp' = sum_j (-0.5 * ((z_j - y'_j) / sigma'_j)^2 - log(sigma'_j)
 *   - 0.5 * log(2 * pi)).  Discrete(5): logp = log_softmax(head)[action] of the recorded head at the recorded action (Gumbel-max samples
 *   the softmax).
 *   FTL_E_INVALID before any device work: what ftl_mlp_act refuses, a Box head with noise but no sigma, and noise / sigma / head_rec /
 *   obs_rec not 4-byte aligned.
 *
 * ftl_collect_mlp: for t = 0 .. T-1 the sample kernel (reading noise block t, writing obs / head / action block t), the step with
 * `flags` -- every step scans --, then ftl_collect_record_kernel, one thread per env; after step T-1 one device-to-device copy of
 * policy_obs to obs block T.  One call, asynchronous on `stream`, the loop of ftl_rollout_mlp (csrc/ftl_rollout.hpp: rollout_loop)
 * without the fold.  Block t of an array lies at base + t * its *_step_bytes, so the parts of a pipelined batch write their rows of one
 * [T][N] tensor (row 0 of a block = env 0 of the handle).
 *   flags     0, or FTL_STEP_NEXT_RESET: the call in which an episode ends returns its terminal observation, so obs[t+1] is always the
 *             true successor of transition t -- the value bootstrap of a time-limit truncation needs no second buffer -- and the restart
 *             step is a transition to ignore.  FTL_STEP_AUTO_RESET, FTL_STEP_QUEUE_RESET and FTL_STEP_SAMPLE_RESET replace the terminal
 *             observation in `out` by the next episode's and are refused with a message that says so; FTL_STEP_NO_SENSORS is refused as
 *             in ftl_rollout_mlp.
 *   record    reward[t][e] = out->reward[e], and kind[t][e]:
 *     FTL_TR_VOID        the env's done word was set ON ENTRY to step t.  Under FTL_STEP_NEXT_RESET this is the restart step: its action was
 *                        ignored, its reward is 0 and obs[t+1] is the new episode's first observation.  Under flags = 0 it is every step
 *                        after the one that ended the episode.
 *     FTL_TR_TRUNCATED   the step raised done with mission status FTL_MISSION_FINISHED_BY_TIME
 *     FTL_TR_TERMINATED  the step raised done with any other status
 *     FTL_TR_STEP        otherwise
 *             "Done on entry" is a byte per env in the handle's rollout scratch (the one ftl_rollout_fold_kernel keeps): set from the
 *             state's done word before step 0 and from out->done after every step, so an env that is done at reset stays VOID until it
 *             restarts into a live world.
 *   Contract  `out`, every state byte and every recorded block equal T iterations of ftl_mlp_sample + ftl_step_encoded(flags) + the
 *             record, bit for bit.  With flags = 0 and noise = NULL the state and `action` equal ftl_rollout_mlp with a record.
 *   FTL_E_INVALID before any device work: what ftl_mlp_sample refuses, NULL h / out / net / b, a NULL obs / head / action / reward / kind,
 *   T <= 0, a refused flag, a *_step_bytes below one block of its array ([n][width[0]] f32, [n][width[L]] f32, the encoded actions, [n]
 *   f64, [n] u8; noise_step_bytes only with noise), base pointers or strides not aligned to their element (4, 4, the action element, 8,
 *   1, 4).  FTL_E_STATE as for ftl_rollout_mlp.
 *
 * ftl_gae (ftl_gae_kernel, one launch, one thread per env, t from T-1 down to 0, loads coalesced over n; the handle only names the
 * device).  reward / kind are the blocks ftl_collect_mlp wrote (any strides of at least n elements), values is the caller's critic on
 * obs[0 .. T], float32 [T+1][n] dense; adv and ret are float32 [T][n] dense.  All arithmetic is float64 with one rounding per
 * operation; gl = gamma * lambda is rounded once on the host; r = reward[t][e], v_t = (double)values[t][e]; the carry c starts at 0.0:
 *     FTL_TR_VOID        adv = ret = 0.0f; c = 0.0 (and nothing below)
 *     FTL_TR_TERMINATED  c = r - v_t
 *     FTL_TR_TRUNCATED   x = gamma * v_{t+1}; y = r + x; c = y - v_t        (v_{t+1}: the value of the terminal observation)
 *     FTL_TR_STEP        x = gamma * v_{t+1}; y = r + x; d = y - v_t; z = gl * c; c = d + z
 *     then               adv[t][e] = (float)c; ret[t][e] = (float)(c + v_t)
 *   Any other kind byte is read as FTL_TR_STEP.  FTL_E_INVALID before any device work: NULL pointers, T <= 0, n <= 0, a stride below n
 *   elements, reward / reward_step_bytes not 8-byte or values / adv / ret not 4-byte aligned. */
enum { FTL_TR_STEP = 0, FTL_TR_TERMINATED = 1, FTL_TR_TRUNCATED = 2, FTL_TR_VOID = 3 };
typedef struct ftl_collect_buffers {   /* DEVICE pointers; block t of an array at base + t * its *_step_bytes */
    float*   obs;     /* [T+1] blocks [n][width[0]] f32: obs[t] is what decided step t, obs[T] what the last step wrote */
    float*   head;    /* [T]   blocks [n][width[L]] f32: raw head */
    void*    action;  /* [T]   blocks in the head's encoding: what was played */
    double*  reward;  /* [T]   blocks [n] */
    uint8_t* kind;    /* [T]   blocks [n]: FTL_TR_* */
    const float* noise;  /* optional, [T] blocks [n][width[L]] */
    const float* sigma;  /* [n_sets][width[L]]; needed with noise on a Box head */
    int64_t obs_step_bytes, head_step_bytes, action_step_bytes, reward_step_bytes, kind_step_bytes, noise_step_bytes;
} ftl_collect_buffers;
size_t ftl_sizeof_collect_buffers(void);
int ftl_mlp_sample(ftl_handle* h, const ftl_outputs* out, const ftl_mlp* net, const float* noise, const float* sigma, float* head_rec,
                   float* obs_rec, void* action, void* stream);
int ftl_collect_mlp(ftl_handle* h, int32_t T, const ftl_outputs* out, const ftl_mlp* net, const ftl_collect_buffers* b,
                    uint32_t flags /* 0 or FTL_STEP_NEXT_RESET */, void* stream);
int ftl_gae(const ftl_handle* h /* device only */, int32_t T, int32_t n,
            const double* reward, int64_t reward_step_bytes, const uint8_t* kind, int64_t kind_step_bytes,
            const float* values /* [T+1][n], dense */, double gamma, double lambda,
            float* adv, float* ret /* [T][n], dense */, void* stream);

/* ---- the net on recorded rows: an ftl_mlp evaluated on the caller's rows, raw heads out (a critic's values, an actor's replay) -------
 * ftl_mlp_forward (ftl_mlp_forward_kernel / ftl_mlp_forward_tanh_kernel, csrc/ftl_mlp.hpp: the body of ftl_mlp_kernel, ONE launch for
 * all blocks, asynchronous on `stream`; the handle only names the device, as for ftl_gae) evaluates `net` on n_blocks blocks of n rows:
 * block b reads float32 [n][width[0]] at (char*)x + b * x_block_bytes and writes float32 [n][width[L]] at (char*)y + b * y_block_bytes.
 * It is the library's pinned forward pass on anything that is not the live policy_obs of a handle: a trajectory's obs blocks, a replay
 * buffer, a critic -- an ftl_mlp of head width 1 whose y is `values` of ftl_gae.
 *   Arithmetic  row r of every block is evaluated as ftl_mlp_act evaluates an env: per neuron the k-ordered fmaf chain from the bias,
 *               then acc > 0 ? acc : 0.0f (FTL_MLP_ACT_RELU) or tanh32(acc) (FTL_MLP_ACT_TANH) by net->activation on the hidden layers,
 *               and a linear head.  y receives y_j = acc of the head layer, before any map: there is no action encoding here.  On the
 *               rows ftl_mlp_sample / ftl_collect_mlp recorded as obs, with the net that played, y equals the recorded head bit for bit.
 *               Nothing else of y is written: not the bytes between a row's end and the next row (there are none: rows are dense), not
 *               the padding between a block's last row and the next block.
 *   Weight set  row r of every block uses set (env_first + r) / envs_per_set: the rule of the policy stack with n in place of the
 *               handle's env count, the same for every block.  So a part of a pipelined batch passes its rows [lo, lo + n) of a [B][N]
 *               tensor as x + lo * width[0], env_first = lo and x_block_bytes = N * width[0] * 4 (y alike).  (env_first + n - 1) /
 *               envs_per_set < n_sets, else FTL_E_INVALID.
 *   Limits      those of ftl_mlp_act for the layers and widths, except that width[L] may be anything in 1 .. FTL_MLP_MAX_WIDTH.
 *               policy_obs and the handle's H * W play no part.  n_blocks is 1 .. 65,535 (the grid's second dimension) and a block has at
 *               most 2^24 - 1 tiles (tiles of FTL_MLP_ENV_TILE rows that end at set boundaries; over 5e8 rows): beyond either,
 *               FTL_E_UNSUPPORTED before any device work.
 *   Aliasing    x and y must not overlap: a workgroup writes its rows of y while others still read x.  This is the caller's duty; it is
 *               not checked.
 *   State       the call needs no env state and no pool: there is no FTL_E_STATE.
 *   FTL_E_INVALID before any device work, each with a message that names the argument: NULL h, net, net->params, x or y; n_blocks < 1 or
 *   n < 1; what ftl_mlp_act refuses of the net itself, with its messages (n_layers, a width, `activation`, params not 4-byte aligned,
 *   set_stride below the param count, n_sets < 1, envs_per_set < 1, env_first < 0, the last row's set beyond n_sets); x_block_bytes below
 *   n * width[0] * 4 or y_block_bytes below n * width[L] * 4, or either not a multiple of 4; x or y not 4-byte aligned. */
int ftl_mlp_forward(const ftl_handle* h /* device only, as ftl_gae */, const ftl_mlp* net,
                    int32_t n_blocks, int32_t n,
                    const float* x, int64_t x_block_bytes,   /* block b: [n][width[0]] f32 at x + b * x_block_bytes */
                    float* y, int64_t y_block_bytes,         /* block b: [n][width[L]] f32 at y + b * y_block_bytes */
                    void* stream);

/* ---- the backward pass of the net on recorded rows: d loss / d params of an ftl_mlp, per weight set, with pinned arithmetic -----------
 * ftl_mlp_backward (ftl_mlp_backward_kernel / ftl_mlp_backward_tanh_kernel and ftl_mlp_backward_reduce_kernel, csrc/ftl_mlp.hpp: two
 * launches on `stream`, asynchronous; the handle only names the device) is ftl_mlp_forward's counterpart: h, net, n_blocks, n, x and
 * x_block_bytes mean what they mean there, the weight-set rule (env_first + r) / envs_per_set included.  dy is the caller's gradient of a
 * scalar loss with respect to the raw head of every row, float32 [n][width[L]] per block at (char*)dy + b * dy_block_bytes; rows to leave
 * out (FTL_TR_VOID steps) carry zeros there.  grad receives d loss / d params, float32 [net->n_sets][set_stride] in the layout of params
 * (W_l as [in][out], then b_l): every parameter word of every set that the rows touch is OVERWRITTEN, not accumulated; the words of
 * untouched sets and the padding between ftl_mlp_param_count and set_stride are not written.  There is no dx: observations are data.
 *   Contract    the result is a pure function of the arguments: no atomics, no dependence on the machine, the grid or timing.  tests/
 *               mlp_backward_numpy.py is the twin, and the device is pinned to it bit for bit.  Per row r (fmaf: one rounding):
 *                 forward   h_0 = x; the hidden layers h_l, l < L, exactly as ftl_mlp_forward computes them (the head is not needed).
 *                 delta_L   = dy.
 *                 delta_l   for l = L-1 .. 1: c[k] = the fmaf chain over j = 0 .. width[l+1]-1 ascending, from +0, of
 *                           W_{l+1}[k][j] * delta_{l+1}[r][j]; then FTL_MLP_ACT_RELU: delta_l[r][k] = h_l[r][k] > 0 ? c[k] : +0 (the forward
 *                           select kept the value: acc > 0); FTL_MLP_ACT_TANH: delta_l[r][k] = c[k] * d in float32 with
 *                           d = fmaf(-a, a, 1.0f), a = h_l[r][k] = tanh32(acc).
 *               and per set, for every layer l = 1 .. L, dW_l[k][j] = sum_r h_{l-1}[r][k] * delta_l[r][j] and db_l[j] = sum_r 1.0f *
 *               delta_l[r][j] -- the bias is row width[l-1] of the layer's [width[l-1] + 1][width[l]] matrix, its input a constant 1.0f --
 *               summed in this order:
 *                 tiles     the set's tiles are those of ftl_mlp_forward (runs of up to FTL_MLP_ENV_TILE = 32 rows of a block that end at
 *                           the set's last row of the block), enumerated block-major: all tiles of block 0 ascending, then block 1, ...
 *                 spans     consecutive runs of FTL_MLP_BWD_SPAN tiles of that enumeration (the last span of a set may be shorter).
 *                 partial   a span's partial of a word is the fmaf chain from +0 over its tiles ascending and, inside a tile, over 32 row
 *                           slots ascending: acc = fmaf(h_{l-1}[r][k], delta_l[r][j], acc).
 *                 cut tiles a tile of fewer than 32 rows still has 32 slots: in the slots past its end both factors are +0 (the 1.0f of
 *                           the bias too), so each contributes fmaf(+0, +0, acc) -- which turns an acc of -0 into +0 and changes nothing
 *                           else.  A short last span has no slots for the tiles it lacks.
 *                 reduce    grad word = (float)(the float64 sum, from +0.0, of the partials as float64 in ascending span order): float64
 *                           additions, one rounding to float32 at the end.
 *               FTL_MLP_BWD_SPAN, the slot rule and the reduction are constants of this header, not properties of a device or a launch.
 *   Workspace   ftl_sizeof_mlp_backward_workspace(net, n_blocks, n) bytes of device memory, 4-byte aligned, contents irrelevant before
 *               and undefined after: spans * ftl_mlp_param_count * 4, spans = the sum over the touched sets of
 *               ceil(n_blocks * ceil(rows of the set in a block / 32) / FTL_MLP_BWD_SPAN).  Pure host arithmetic; -1 for a NULL net,
 *               counts below 1, envs_per_set < 1, env_first < 0 or widths outside the limits.
 *   Limits      those of ftl_mlp_forward (layers, widths, n_blocks, tiles of a block), width[0] at most FTL_MLP_BWD_MAX_IN, and at most
 *               2^24 - 1 spans in all: beyond any, FTL_E_UNSUPPORTED before any device work.
 *   Aliasing    grad and workspace must not overlap x, dy, params or each other (not checked).
 *   FTL_E_INVALID before any device work, each with a message that names the argument: NULL h, net, net->params, x, dy, grad or workspace;
 *   n_blocks < 1 or n < 1; what ftl_mlp_forward refuses of the net itself, with its messages; x_block_bytes below n * width[0] * 4 or
 *   dy_block_bytes below n * width[L] * 4, or either not a multiple of 4; workspace_bytes below the query's answer; x, dy, grad or
 *   workspace not 4-byte aligned. */
#define FTL_MLP_BWD_SPAN 64            /* tiles of a span: 2,048 row slots in one float32 chain */
#define FTL_MLP_BWD_MAX_IN FTL_MLP_MAX_IN
int64_t ftl_sizeof_mlp_backward_workspace(const ftl_mlp* net, int32_t n_blocks, int32_t n);
int ftl_mlp_backward(const ftl_handle* h /* device only */, const ftl_mlp* net,
                     int32_t n_blocks, int32_t n,
                     const float* x, int64_t x_block_bytes,    /* block b: [n][width[0]] f32 at x + b * x_block_bytes */
                     const float* dy, int64_t dy_block_bytes,  /* block b: [n][width[L]] f32 at dy + b * dy_block_bytes */
                     float* grad,                              /* [n_sets][set_stride] f32, the layout of params */
                     void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the PPO loss head on recorded rows: from heads, record, advantages and values to dhead, dvalue, d log_std and statistics ----------
 * ftl_ppo_head (ftl_ppo_moments_kernel, ftl_ppo_scalars_kernel, ftl_ppo_rows_kernel, ftl_ppo_stats_kernel, csrc/ftl_ppo.hpp: four
 * launches on `stream`, asynchronous, nothing synchronises with the host; the handle only names the device, as for ftl_gae) is the piece
 * between ftl_mlp_forward / ftl_rnn_forward and ftl_mlp_backward / ftl_rnn_backward: the clipped-surrogate loss of PPO with a value term
 * for Box heads (width A = 2, or 1 under constant_follower_speed) with a state-independent Gaussian deviation per weight set, and its
 * derivative with respect to every head, every value and log_std.  Per set s
 *     loss_s = mean over the set's valid rows of [ -min(r * a, clip(r) * a) + vf_coef * 0.5 * (v - ret)^2 ]
 * and the total loss is the sum over the sets, so the gradient of a set depends on its rows alone.  The entropy bonus is not here: with a
 * state-independent sigma it is sum(log_std) plus a constant and touches no row.
 *   Inputs      device pointers; block b of an array lies at base + b * its *_block_bytes.  n_sets must divide n; row r of every block
 *               uses set r / (n / n_sets), the rule of ftl_mlp_forward.  head_new, head_old (the recorded head) and noise are float32
 *               [n][A] a block; sigma_old, sigma_new and log_sigma_shift float32 [n_sets][A] -- log_sigma_shift is the caller's
 *               c = log_std_new - log_std_old, NULL reads as +0 --; adv, ret and value_new float32 [n] a block; value_new == NULL means no
 *               value part (dvalue must then be NULL too, and the reverse); kind uint8 [n] a block: FTL_TR_VOID rows are left out, any
 *               other byte is a row to learn from, as in ftl_gae.  clip_lo and clip_hi are 1 -+ eps rounded once on the host; normalize
 *               is 0 or 1.
 *   Outputs     dhead float32 [n][A] a block, dvalue float32 [n] a block, dlog_std float32 [n_sets][A], stats float64
 *               [n_sets][FTL_PPO_STATS].  Every word of every output is overwritten (block padding is not touched); FTL_TR_VOID rows get
 *               +0.  The result is a pure function of the arguments: no atomics, no dependence on the machine, the grid or timing.
 *               tests/ppo_numpy.py is the twin and the device is pinned to it bit for bit.
 *   Row         float32, one IEEE rounding per line; div32 and exp32 are those of csrc/ftl_rnn_math.hpp; csrc/ftl_ppo_math.hpp is these
 *               lines for host and device.  Per component j:
 *                 e   = head_old_j - head_new_j
 *                 t   = fmaf(sigma_old_j, noise_j, e)
 *                 u_j = div32(t, sigma_new_j)
 *                 p_j = u_j * u_j
 *                 q   = noise_j * noise_j
 *                 w   = q - p_j
 *                 l_j = fmaf(0.5f, w, -c_j)
 *               per row:
 *                 d  = l_0 (A = 1), l_0 + l_1 (A = 2)
 *                 r  = d if d is NaN; exp32(d) if d <= 0; div32(1.0f, exp32(-d)) otherwise
 *                 a  = adv without normalisation; am = adv - mean32_s, a = am * inv32_s with it
 *                 s1 = r * a
 *                 rc = fminf(fmaxf(r, clip_lo), clip_hi)
 *                 s2 = rc * a
 *                 active = !(s2 < s1)                    (a NaN row propagates; a tie goes through s1, as torch's does inside the range)
 *                 g  = -(s1 * invc_s) if active, else +0
 *                 dhead_j = g * div32(u_j, sigma_new_j)
 *                 k_j = g * (p_j - 1.0f)                 (the row's share of d loss / d log_std_new_j; the subtraction is a line)
 *                 hv = v - ret
 *                 dvalue = (vf_coef * hv) * invc_s
 *   Reductions  a segment is up to FTL_PPO_SEG consecutive rows of one set's slice of one block: a slice of fewer rows is one segment,
 *               otherwise the last segment of a slice may be short.  Within a segment lane k of 64 sums the rows at offsets = k (mod 64),
 *               ascending, in float64 from +0.0, FTL_TR_VOID rows skipped; then x[k] += x[k + stride] for stride 32, 16, 8, 4, 2, 1 and
 *               x[0] is the segment's partial.  A set's total is the float64 sum from +0.0 of its partials in ascending (block,
 *               segment) order.  Summed are, each a float32 value widened to float64: 1 (the count); adv; adv * adv, formed in float64;
 *               -(active ? s1 : s2); 0.5f * (hv * hv) (the product is a line); -d; 1 where r < clip_lo || r > clip_hi; k_0; k_1.
 *   Set scalars float64, one rounding per operation: mean = S1 / cnt; var = ((S2 - S1 * mean) / (cnt - 1)), replaced by +0 where it is
 *               below 0 (a NaN stays), and +0 when cnt < 2; std = sqrt(var); inv = 1 / (std + 1e-8); mean32 and inv32 are mean and inv
 *               rounded to float32; invc = (float)(1.0 / cnt), +0 when cnt = 0.  mean is +0 when cnt = 0.
 *   Stats       column 0 count, 1 advantage mean, 2 advantage std, 3 policy loss (total / cnt), 4 value loss, 5 approximate KL (the mean
 *               of -d), 6 clip fraction, 7 column 3 + (double)vf_coef * column 4.  Means over an empty set are +0.0; columns 4 and 7 take
 *               the value part as 0 when value_new is NULL.  dlog_std_j = (float) the set's total of k_j.
 *   Workspace   ftl_sizeof_ppo_head_workspace(n_blocks, n, n_sets) bytes of device memory, 8-byte aligned, contents irrelevant before and
 *               undefined after: segments * 72 + n_sets * 16 with segments = n_blocks * n_sets * ceil((n / n_sets) / FTL_PPO_SEG).  Pure
 *               host arithmetic; -1 for counts that ftl_ppo_head refuses or more than 2^31 - 1 segments.
 *   Aliasing    outputs and workspace must not overlap the inputs or each other (not checked).
 *   FTL_E_UNSUPPORTED before any device work: a width other than 1 or 2 (Discrete(5) needs a pinned logarithm: the follow-up); more than
 *   2^31 - 1 segments.  FTL_E_INVALID before any device work, each with a message that names ftl_ppo_head and the argument: NULL h, a, or
 *   a required pointer; dvalue without value_new or the reverse; n_blocks < 1, n < 1, n_sets < 1 or not dividing n; a *_block_bytes below
 *   one block or not a multiple of its element; a pointer not aligned to its element (A * 4 bytes for head_new, head_old, noise and
 *   dhead, 8 for stats, 4 otherwise); clip_lo > clip_hi or either NaN; normalize other than 0 / 1; workspace_bytes below the query's
 *   answer; last, a workspace that is not 8-byte aligned. */
#define FTL_PPO_SEG 1024               /* rows of a segment: 16 a lane */
#define FTL_PPO_STATS 8                /* columns of stats */
typedef struct ftl_ppo_head_args {
    int32_t n_blocks, n, n_sets, width;                            /* B; rows a block; weight sets; A */
    const float* head_new; int64_t head_new_block_bytes;           /* [n][A] f32 a block */
    const float* head_old; int64_t head_old_block_bytes;
    const float* noise; int64_t noise_block_bytes;
    const float* sigma_old;                                        /* [n_sets][A] f32 */
    const float* sigma_new;
    const float* log_sigma_shift;                                  /* [n_sets][A] f32, or NULL */
    const float* adv; int64_t adv_block_bytes;                     /* [n] f32 a block */
    const float* ret; int64_t ret_block_bytes;
    const float* value_new; int64_t value_new_block_bytes;         /* [n] f32 a block, or NULL */
    const uint8_t* kind; int64_t kind_block_bytes;                 /* [n] u8 a block */
    float clip_lo, clip_hi, vf_coef;
    int32_t normalize;
    float* dhead; int64_t dhead_block_bytes;                       /* out: [n][A] f32 a block */
    float* dvalue; int64_t dvalue_block_bytes;                     /* out: [n] f32 a block, or NULL */
    float* dlog_std;                                               /* out: [n_sets][A] f32 */
    double* stats;                                                 /* out: [n_sets][FTL_PPO_STATS] f64 */
    void* workspace; int64_t workspace_bytes;
} ftl_ppo_head_args;
size_t ftl_sizeof_ppo_head_args(void);
int64_t ftl_sizeof_ppo_head_workspace(int32_t n_blocks, int32_t n, int32_t n_sets);
int ftl_ppo_head(const ftl_handle* h /* device only, as ftl_gae */, const ftl_ppo_head_args* a, void* stream);

/* ---- recurrent policy: a trunk of dense ReLU layers, one LSTM cell and a linear head, as a decision, a rollout and a trajectory -------
 * The memoryless stack above (ftl_mlp_act, ftl_rollout_mlp, ftl_mlp_sample, ftl_collect_mlp) with a state per env that the caller owns
 * and the library zeroes at episode boundaries.  ftl_rnn_act (ftl_rnn_kernel, csrc/ftl_rnn.hpp, one launch per decision, asynchronous on
 * `stream`) is one decision of every env; ftl_rollout_rnn and ftl_collect_rnn are ftl_rollout_mlp and ftl_collect_mlp with it.  The
 * arithmetic is fixed operation by operation, transcendentals included, so the device equals a numpy twin bit for bit
 * (tests/rnn_numpy.py).
 *
 * Net         Trunk: Lt = n_layers dense ReLU layers, 1 <= Lt <= FTL_MLP_MAX_LAYERS - 1, widths width[0 .. Lt]; the limits of the widths,
 *             the chain of a neuron and the ReLU are exactly those of ftl_mlp_act (every trunk layer is a hidden one); width[0] = H * W
 *             of policy_obs.  Then one LSTM cell of C = cell units, 1 <= C <= FTL_RNN_MAX_CELL.  Then a linear head of width
 *             A = width[Lt + 1], which is 2, 1 or 5 with the encodings of ftl_mlp_act (any other: FTL_E_INVALID).  Beyond the limits:
 *             FTL_E_UNSUPPORTED before any device work.  ftl_rnn.activation must be FTL_MLP_ACT_RELU (0): every ftl_rnn_* entry point
 *             answers any other value with FTL_E_UNSUPPORTED and a message that says the trunk is ReLU.
 * Cell input  u = [x | a_prev | r_prev | h] of width U = width[Lt] + P + R + C: x the trunk's output; a_prev of width P under
 *             FTL_RNN_PREV_ACTION (2 for Box(2), 1 for the turn, 5 -- one-hot -- for Discrete(5)), else P = 0; r_prev of width R = 1 under
 *             FTL_RNN_PREV_REWARD, else R = 0; h the cell's last output.
 * Parameters  float32 in DEVICE memory, sets and set_stride as in ftl_mlp.  One set: the trunk layers as in ftl_mlp; then W_g [U][4C]
 *             row-major, rows in the order of u, columns gate-major i | f | g | o (torch's weight_ih.T stacked over weight_hh.T); then
 *             b_g [4C] (a loader adds bias_ih + bias_hh); then W_y [C][A] and b_y [A].  ftl_rnn_param_count returns the count, -1 outside
 *             the limits or on NULL.
 * State       a device block [n][S] float32 the caller owns, row e at state + e * state_stride floats (row 0 = env 0 of the handle),
 *             S = 2C + P + 1, state_stride >= S: a row is h [C] | c [C] | a_prev [P] | live.  live is 1.0f once the row holds a decision
 *             of the running episode; a zeroed row is a fresh episode.
 * One decision of env e, in this order:
 *   1. read the row; in mode BEFORE it is read as all zeros when out->done[e] != 0.  r_prev = live != 0 ? (float)out->reward[e] : 0.0f.
 *   2. x = the trunk.
 *   3. z_j, j < 4C: acc = b_g[j]; for k = 0 .. U - 1: acc = fmaf(u[k], W_g[k][j], acc).
 *   4. the cell, one float32 rounding per line, for j < C:
 *          i = sig32(z[j]); f = sig32(z[C + j]); g = tanh32(z[2C + j]); o = sig32(z[3C + j]);
 *          t = i * g;  c' = fmaf(f, c, t);  h' = o * tanh32(c')
 *   5. y = the chain of the head layer over h'.  The head map, noise, sigma, head_rec and obs_rec are exactly those of ftl_mlp_sample;
 *      noise == NULL is the deterministic map of ftl_mlp_act.
 *   6. a_prev': Box heads (float)a_j of the float64 action just written; Discrete(5) the one-hot of k.
 *   7. write the row: in mode AFTER, when the env was done on entry, zeros; otherwise h' | c' | a_prev' | 1.0f.  The optional
 *      state_rec [n][S] (dense) receives the row as step 1 read it.
 * Mode AFTER  the default: for no reset and next-step reset, where the decision at a finished env is the void one (its action is ignored
 *             by the restart step, or nothing restarts at all), and the zeroed row is what the new episode's first decision reads.  "Done
 *             on entry" is the state's done word env_int[FTL_EI_DONE] in ftl_rnn_act, and inside the loops the byte of the rollout scratch
 *             that ftl_rollout_fold_kernel / ftl_collect_record_kernel keep (the same predicate that marks FTL_TR_VOID).
 * Mode BEFORE FTL_RNN_ZERO_ON_OUT_DONE (a flag of the CALL): for same-step, queue and sample reset, where `out` already holds the next
 *             episode's first observation beside the terminal reward and done.
 * sig32, tanh32, exp32 (csrc/ftl_rnn_math.hpp, __host__ __device__; every line one float32 operation, the unit is built with
 * -ffp-contract=off; divisions IEEE-rounded, subnormals kept):
 *     exp32(a), a <= 0:  a = fmaxf(a, -86.0f); n = rintf(a * 0x1.715476p+0f); r = fmaf(n, -0x1.62e400p-1f, a);
 *                        r = fmaf(n, -0x1.7f7d1cp-20f, r); p = Horner with fmaf over the float32 roundings of 1/5040, 1/720, 1/120, 1/24,
 *                        1/6, 1/2, 1, 1; result ldexpf(p, (int)n)
 *     sig32(x):          e = exp32(-fabsf(x)); d = 1.0f + e; x >= 0 ? 1.0f / d : e / d
 *     tanh32(x):         e = exp32(-2.0f * fabsf(x)); copysignf((1.0f - e) / (1.0f + e), x)
 *   Both return x itself when x != x.  Against float64: exp32 within 0.92 ulp, sig32 within 8.91e-8 and tanh32 within 8.93e-8 absolute.
 *   Near 0 the relative error of tanh32 is large by cancellation ((1 - e) with e close to 1); that is accepted.
 *
 * ftl_rollout_rnn: ftl_rollout_mlp's signature and rules with ftl_rnn_kernel in mode AFTER as the decision; every step scans.
 * ftl_collect_rnn: ftl_collect_mlp's signature, rules and record; ftl_rnn_collect_buffers is ftl_collect_buffers plus `state`: block t
 * (at state + t * state_step_bytes) receives the rows decision t READ, [n][S] dense; state_steps is 1 (only block 0: what
 * back-propagation through time starts from) or T.  Both go through the one rollout loop (csrc/ftl_rollout.hpp).  Contract: `out`, every
 * state byte of the env, the policy's state block and every recorded block equal T iterations of ftl_rnn_act + ftl_step_encoded(flags)
 * (+ fold / record), bit for bit.
 * FTL_E_INVALID / FTL_E_UNSUPPORTED before any device work: what ftl_mlp_sample and ftl_collect_mlp refuse, a NULL state, a state_stride
 * below S, a state not 4-byte aligned, an unknown flag, a cell beyond the limit (UNSUPPORTED), FTL_RNN_ZERO_ON_OUT_DONE given to a loop. */
#define FTL_RNN_MAX_CELL 128
#define FTL_RNN_PREV_ACTION 1u        /* ftl_rnn.flags */
#define FTL_RNN_PREV_REWARD 2u        /* ftl_rnn.flags */
#define FTL_RNN_ZERO_ON_OUT_DONE 1u   /* flags of ftl_rnn_act: mode BEFORE */
typedef struct ftl_rnn {
    const float* params;       /* DEVICE, [n_sets] sets of set_stride floats */
    int64_t  set_stride;
    int32_t  n_sets;
    int32_t  n_layers;         /* Lt: the trunk's layers */
    int32_t  width[FTL_MLP_MAX_LAYERS + 1];   /* width[0 .. Lt] the trunk, width[Lt + 1] the head */
    int32_t  env_first;
    int32_t  envs_per_set;
    int32_t  activation;       /* ftl_mlp's field: FTL_MLP_ACT_RELU (0) only */
    int32_t  cell;             /* C */
    uint32_t flags;            /* FTL_RNN_PREV_ACTION | FTL_RNN_PREV_REWARD */
    float*   state;            /* DEVICE, [n] rows of state_stride floats */
    int64_t  state_stride;     /* floats between two rows, >= S */
} ftl_rnn;
typedef struct ftl_rnn_collect_buffers {
    ftl_collect_buffers b;
    float*   state;            /* [state_steps] blocks [n][S] f32: the rows decision t read */
    int64_t  state_step_bytes;
    int32_t  state_steps;      /* 1 or T */
    int32_t  _pad;
} ftl_rnn_collect_buffers;
size_t ftl_sizeof_rnn(void);
size_t ftl_sizeof_rnn_collect_buffers(void);
int64_t ftl_rnn_param_count(const int32_t* widths /* [n_layers + 2] */, int32_t n_layers, int32_t cell, uint32_t flags);
int ftl_rnn_act(ftl_handle* h, const ftl_outputs* out, const ftl_rnn* net, const float* noise, const float* sigma, float* head_rec,
                float* obs_rec, float* state_rec, void* action, uint32_t flags /* 0 or FTL_RNN_ZERO_ON_OUT_DONE */, void* stream);
int ftl_rollout_rnn(ftl_handle* h, int32_t T, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro, const ftl_rnn* net,
                    void* actions /* [T] blocks in the head's encoding, or NULL */, int64_t step_bytes, uint32_t flags /* 0 */, void* stream);
int ftl_collect_rnn(ftl_handle* h, int32_t T, const ftl_outputs* out, const ftl_rnn* net, const ftl_rnn_collect_buffers* b,
                    uint32_t flags /* 0 or FTL_STEP_NEXT_RESET */, void* stream);

/* ---- the recurrent net on a recorded sequence: an ftl_rnn evaluated on the caller's blocks, raw heads out (the actor's replay, a critic
 * with memory) ------------------------------------------------------------------------------------------------------------------------
 * ftl_rnn_forward (ftl_rnn_forward_kernel, csrc/ftl_rnn.hpp: ONE launch for the whole sequence, the block loop inside the kernel,
 * asynchronous on `stream`; the handle only names the device, as for ftl_gae and ftl_mlp_forward) is ftl_mlp_forward's counterpart for
 * ftl_rnn: it puts n_blocks = B recorded blocks of n rows back through `net`, carrying the state from block to block as ftl_collect_rnn
 * did when it recorded them.  Block b of an array lies at (char*)base + b * its *_block_bytes.
 *   Net, sets   the limits, the parameter layout and the set rule are those of ftl_rnn_act: row r of every block uses set
 *               (env_first + r) / envs_per_set with n in place of the handle's env count; (env_first + n - 1) / envs_per_set < n_sets.
 *               policy_obs and the handle's H * W play no part.  A part of a wider [B][N] record passes its rows [lo, lo + n) as base +
 *               lo * row bytes, env_first = lo and the *_block_bytes of N rows.
 *   State       net->state (rows of state_stride floats, row 0 = row 0 of this call) is the row h | c | a_prev | live every row of the
 *               sequence has BEFORE block 0.  It is read and never written.
 *   Block b     is evaluated operation for operation as ftl_rnn_act in mode AFTER evaluates a decision (tests/rnn_numpy.py: decide):
 *               u = [trunk(obs[b]) | a_prev | r_prev | h], the gate chain, the cell lines, the linear head.
 *                 b = 0: a_prev, live and h, c come from the state row; r_prev = live != 0 ? (float)reward0[r] : 0.0f (reward0 == NULL
 *                        reads as 0.0: it is out->reward as it stood before block 0 was decided).
 *                 b > 0: the row block b reads is the one block b - 1 left: h', c', a_prev = (float) of action[b - 1] (Discrete(5): the
 *                        one-hot of the index, zeros for an index outside 0 .. 4), live = 1 and r_prev = live != 0 ?
 *                        (float)reward[b - 1] : 0.0f -- except under the zero rule.
 *               Zero rule: the row block b + 1 reads is all zeros (h, c, a_prev and live, so r_prev too) where kind[b] == FTL_TR_VOID,
 *               and nowhere else: exactly what ftl_collect_rnn does at a decision whose env was done on entry.
 *   Outputs     head[b] = the head layer's acc, float32 [n][A] dense: no map, no noise.  On the record of ftl_collect_rnn, with the net
 *               that played, the state block 0 of the record and reward0 = out->reward before the call, head equals the recorded head bit
 *               for bit, VOID rows included.  h[b] (optional) = h' of block b, float32 [n][C] dense, before any wipe, as the head reads
 *               it.  state_out (optional) = the rows block state_at READ, [n][S] dense, 0 <= state_at < n_blocks: with state_at = t it
 *               equals block t of ftl_rnn_collect_buffers.state, and it is the net->state of a call that continues at block state_at
 *               (with reward0 = reward[state_at - 1]).  Nothing else is written.
 *   Pointers    action may be NULL without FTL_RNN_PREV_ACTION, reward without FTL_RNN_PREV_REWARD; with n_blocks == 1 action, reward
 *               and kind may all be NULL (they are read for b < n_blocks - 1 only).  Inputs and outputs must not overlap: that is the
 *               caller's duty; it is not checked.
 *   No FTL_E_STATE: the call needs no env state and no pool.
 *   FTL_E_INVALID before any device work, each with a message that names the argument: NULL h, net, net->params, seq, obs, head, or a
 *   record array the net reads; n_blocks < 1 or n < 1; what ftl_rnn_act refuses of the net and its state, with its messages; a
 *   *_block_bytes below one block of n rows or no multiple of the element size; a pointer not aligned to its element; state_at outside
 *   [0, n_blocks) when state_out is given.  FTL_E_UNSUPPORTED: an activation other than ReLU, a cell or a width beyond the limits, more
 *   than 65,535 blocks, more than 2^24 - 1 tiles. */
typedef struct ftl_rnn_sequence {
    const float*   obs;      int64_t obs_block_bytes;     /* [B][n][width[0]] */
    const void*    action;   int64_t action_block_bytes;  /* [B-1][n] in the head's encoding: f64 x2 (head 2), f64 (head 1), int32 (head 5) */
    const double*  reward;   int64_t reward_block_bytes;  /* [B-1][n] */
    const uint8_t* kind;     int64_t kind_block_bytes;    /* [B-1][n] of FTL_TR_* */
    const double*  reward0;                               /* [n]: out->reward before block 0, NULL = 0 */
    float*         head;     int64_t head_block_bytes;    /* out [B][n][A] */
    float*         h;        int64_t h_block_bytes;       /* out [B][n][C], optional */
    float*         state_out; int32_t state_at;           /* out [n][S], optional: the rows block state_at read, 0 <= state_at < B */
} ftl_rnn_sequence;
size_t ftl_sizeof_rnn_sequence(void);
int ftl_rnn_forward(const ftl_handle* h, const ftl_rnn* net, int32_t n_blocks, int32_t n, const ftl_rnn_sequence* seq, void* stream);

/* ---- the backward pass of the recurrent net on a recorded sequence: d loss / d params of an ftl_rnn, per weight set, by back-propagation
 * through time with pinned arithmetic --------------------------------------------------------------------------------------------------
 * ftl_rnn_backward (ftl_rnn_backward_kernel, csrc/ftl_rnn.hpp, and ftl_mlp_backward_reduce_kernel: two launches on `stream`, asynchronous;
 * the handle only names the device) is ftl_rnn_forward's counterpart as ftl_mlp_backward is ftl_mlp_forward's.  h, net, n_blocks = B, n
 * and seq mean what they mean to ftl_rnn_forward: seq->obs, action, reward, kind and reward0 are read exactly as there, with net->state
 * as the rows before block 0 (read, never written); seq->head, h and state_out are neither read nor written and may be NULL.
 *   ftl_rnn_gradient
 *     dhead      the caller's gradient of a scalar loss with respect to the raw head of every row, float32 [n][A] per block at
 *                (char*)dhead + b * dhead_block_bytes; rows to leave out (FTL_TR_VOID steps) carry zeros.
 *     grad       d loss / d params, float32 [net->n_sets][set_stride] in the layout of params: every parameter word of every set the rows
 *                touch is OVERWRITTEN, not accumulated; untouched sets and the padding up to set_stride are not written.
 *     dstate_in  optional, float32 [n][2C] dense: d loss / d (h', c') of block B - 1, from a later piece of the sequence (NULL: zeros).
 *     dstate_out optional, float32 [n][2C] dense: d loss / d (h, c) of the rows block 0 read: the dstate_in of the piece before.  It is
 *                what the arithmetic below leaves, with no regard to the seam: the caller zeroes the rows whose kind at the seam is
 *                FTL_TR_VOID (the row the later piece read was zeros there).
 *     workspace  ftl_sizeof_rnn_backward_workspace(net, B, n) bytes of device memory, 4-byte aligned, contents irrelevant before and
 *                undefined after.
 *   Observations, recorded actions, rewards and live are data: there is no gradient with respect to them.
 *   Contract    the result is a pure function of the arguments: no atomics, no communication between workgroups inside a launch, no
 *               dependence on the machine, the grid or timing.  tests/rnn_backward_numpy.py is the twin and the device is pinned to it bit
 *               for bit.  Per row, for b = B-1 down to 0 (fmaf: one rounding; every other line one float32 operation):
 *                 forward   the values of block b are exactly those of ftl_rnn_forward, zero rule included: u (the cell input), z, the
 *                           gates i f g o, c (the cell state the block read), c', h', the trunk's activations h_0 = obs .. h_Lt = x, and
 *                           tc = tanh32(c').  (The device keeps h' and c' of every block from a forward sweep and recomputes the rest: the
 *                           pinned chains again, so the bits are the same.)
 *                 head      dh[k] = the fmaf chain over j = 0 .. A-1 ascending, from +0, of W_y[k][j] * dy[j]; then dh = dh + dh_next.
 *                 carry     dh_next and dc_next are dstate_in (or +0) at b = B-1; +0 where kind[b] == FTL_TR_VOID (the row block b+1 read
 *                           was zeros); otherwise what block b+1 left (dh_next', dc_next' below).
 *                 cell      q = dh * o;  d = fmaf(-tc, tc, 1.0f);  dc = fmaf(q, d, dc_next);  do = dh * tc;
 *                           di = dc * g;  dg = dc * i;  df = dc * c;  dc_next' = dc * f;
 *                           dz_i = di * fmaf(-i, i, i);  dz_f = df * fmaf(-f, f, f);  dz_o = do * fmaf(-o, o, o);
 *                           dz_g = dg * fmaf(-g, g, 1.0f).
 *                 gate in   du[k], k < U = the fmaf chain from +0 of W_g[k][col] * dz[col] over the columns in PASS order: for
 *                           p = 0 .. ceil(C / FTL_RNN_PASS_CELLS) - 1, for the gates q = i, f, g, o, for the cells j of pass p ascending
 *                           (j0 = p * FTL_RNN_PASS_CELLS <= j < min(C, j0 + FTL_RNN_PASS_CELLS)): col = q * C + j.  For C <=
 *                           FTL_RNN_PASS_CELLS that is col = 0 .. 4C-1 ascending.  Its h columns are dh_next', its x columns feed the
 *                           trunk, its a_prev and r_prev columns are dropped.
 *                 trunk     delta_Lt[k] = x[k] > 0 ? du[k] : +0; then for l = Lt .. 2 the rule of ftl_mlp_backward under FTL_MLP_ACT_RELU:
 *                           c[k] = the fmaf chain over j = 0 .. width[l]-1 ascending, from +0, of W_l[k][j] * delta_l[j];
 *                           delta_{l-1}[k] = h_{l-1}[k] > 0 ? c[k] : +0.
 *               and per set dW_y = sum h' (x) dy, dW_g = sum u (x) dz, dW_l = sum h_{l-1} (x) delta_l over the set's rows of all blocks,
 *               every bias the row of its matrix whose input is a constant 1.0f, summed in this order:
 *                 tiles     the set's tiles are those of ftl_rnn_forward (runs of up to FTL_MLP_ENV_TILE = 32 rows of a block that end at
 *                           the set's last row of the block).
 *                 groups    G = max(1, FTL_RNN_BWD_SPAN / B) (integer division) consecutive tiles of a set; the last group of a set may
 *                           be shorter.  A group's (tile, block) pairs are enumerated tile-major, inside a tile the blocks DESCENDING
 *                           (B-1 first: the order back-propagation visits them).
 *                 spans     runs of FTL_RNN_BWD_SPAN = 64 consecutive pairs of ONE group; a group's last span may be shorter.
 *                 partial   a span's partial of a word is the fmaf chain from +0 over its pairs and, inside a pair, the tile's 32 row
 *                           slots ascending: acc = fmaf(input[r][k], delta[r][j], acc).
 *                 cut tiles in the slots past a cut tile's end both factors are +0 (the bias's 1.0f too): fmaf(+0, +0, acc), which turns
 *                           an acc of -0 into +0 and changes nothing else, as in ftl_mlp_backward.
 *                 reduce    grad word = (float)(the float64 sum, from +0.0, of the set's partials as float64 in ascending (group, span)
 *                           order).
 *               Signed zeros: every other chain above has exactly the terms written -- the chains of dh (A terms), du (4 * cells of a pass
 *               terms per pass, a multiple of 4) and c (width[l] terms; the device finishes a width that is no multiple of 4 with plain
 *               fmaf) have no padded terms, so no -0 is turned into +0 anywhere but in the cut tiles' slots.  A chain from +0 whose
 *               terms are all -0 or of mixed signed zeros gives +0, as fmaf does.
 *               A float32 chain is at most 64 * 32 = 2,048 slots long.  FTL_RNN_BWD_SPAN, the group rule and the pass order are constants
 *               of this header, not properties of a device or a launch.
 *   Workspace   ftl_sizeof_rnn_backward_workspace(net, B, n) = 4 * (spans * ftl_rnn_param_count + B * n * 2C + groups * 32 * U) bytes: the
 *               span partials, the record h' | c' of every block, and one tile of du per group (a cell of two passes carries du between
 *               them).  groups = the sum over the touched sets of ceil(tiles / G), tiles = ceil(rows of the set in a block / 32); spans =
 *               the sum over the touched sets of floor(tiles / G) * ceil(G * B / 64) + ceil((tiles % G) * B / 64).  Pure host arithmetic;
 *               -1 for a NULL net, counts below 1, envs_per_set < 1, env_first < 0, or a net outside the limits of ftl_rnn_param_count.
 *   Limits      those of ftl_rnn_forward (layers, widths, cell, n_blocks, tiles of a block), at most 2^24 - 1 spans, ReLU only (the
 *               message of every ftl_rnn_* entry point otherwise), and the workgroup's LDS: 4 * (32 * ((Lt - 1) * act_stride + u_stride
 *               + h_stride + max(4 * min(C, 64) + 2, 66 + h_stride + 34)) + stage) bytes must not exceed 160 KiB, with act_stride,
 *               u_stride, h_stride = the widest of width[1 .. Lt-1] and A, U, C, each rounded up to a multiple of 32, plus 2, and stage =
 *               at most 4,416 floats.  180-256-256 with C = 128 and a head of 5 needs 152,832 bytes, 128-128-128 with C = 128 fits, three trunk
 *               layers of 256 do not.  Beyond any: FTL_E_UNSUPPORTED before any device work.
 *   Aliasing    grad, workspace and dstate_out must not overlap any input or each other (not checked).
 *   FTL_E_INVALID before any device work, each with a message that names the argument: NULL h, net, net->params, seq, g, seq->obs,
 *   g->dhead, g->grad, g->workspace, or a record array the net reads; n_blocks < 1 or n < 1; what ftl_rnn_forward refuses of the net and
 *   its state, with its messages; a *_block_bytes below one block of n rows or no multiple of the element size; workspace_bytes below
 *   the query's answer; a pointer not aligned to its element. */
#define FTL_RNN_BWD_SPAN 64            /* (tile, block) pairs of a span: 2,048 row slots in one float32 chain */
typedef struct ftl_rnn_gradient {
    const float* dhead;      int64_t dhead_block_bytes;   /* [B][n][A] */
    float*       grad;                                    /* out [n_sets][set_stride], the layout of params */
    void*        workspace;  int64_t workspace_bytes;
    const float* dstate_in;                               /* [n][2C], optional */
    float*       dstate_out;                              /* out [n][2C], optional */
} ftl_rnn_gradient;
size_t ftl_sizeof_rnn_gradient(void);
int64_t ftl_sizeof_rnn_backward_workspace(const ftl_rnn* net, int32_t n_blocks, int32_t n);
int ftl_rnn_backward(const ftl_handle* h /* device only */, const ftl_rnn* net, int32_t n_blocks, int32_t n,
                     const ftl_rnn_sequence* seq, const ftl_rnn_gradient* g, void* stream);

/* ---- episode queue: every entry of a list of scenarios played exactly once, with one record per entry (evaluation, curricula, level
 * replay) ---------------------------------------------------------------------------------------------------------------------------
 * The third reset discipline next to FTL_STEP_AUTO_RESET and FTL_STEP_NEXT_RESET, which restart a finished env at once from the reset
 * window and so play MORE episodes in the slots whose episodes are short.  Here the caller attaches a queue of Q pool indices; each entry
 * is played once, by whichever slot is free; its result goes to row q of `records`; a slot that finds the queue empty parks.
 *
 * Equivalence (the contract): the episode played for entry q -- every observation, reward and status of it, and its record -- is what env q
 * of a FRESH handle with env_id_base = s0, reset with scen_idx = the queue and stepped without auto-reset, gives under the same actions,
 * where s0 + q is the entry's stream id.  It is a pure function of (config, pool entry, stream id, actions): neither the slot, nor the
 * handle, nor what the slot played before enters.  To that end a slot that takes an entry gets the random-stream words of a fresh env:
 * FTL_EI_STREAM = stream id - env_id_base - slot, and FTL_EI_RESETS, FTL_EI_FPS, FTL_EI_ACC_CONSUMED zeroed as in a zeroed state buffer.
 * Stream ids lie in 0 .. INT32_MAX (the step kernels key their draws by a 32-bit id); with stream == NULL that is checked at attach time
 * (FTL_E_INVALID), otherwise on the device (FTL_ERR_BAD_STREAM in the slot's sticky error word).
 *
 * ftl_queue_start is the queue's ftl_reset: slot e = 0 .. n_envs - 1 takes entry head + e (one fetch-add of n_envs on head), is placed and
 * scanned exactly as ftl_reset does, and `out` holds the first observations.  Slots past the end of the queue park: ticket -1; they are
 * placed on the queue's entry 0 and their done word is set, so that they step like a finished env without auto-reset (ENV:908-945 steps a
 * finished env as well).  Outputs of parked slots mean nothing (their done byte stays 1).
 *
 * ftl_step_final / ftl_step_encoded / ftl_step with FTL_STEP_QUEUE_RESET: a step without auto-reset (the sensors scan the terminal state of
 * the envs that finish), then ftl_queue_kernel: every slot whose done byte is set and whose ticket is >= 0 writes the record of its entry
 * from its terminal state and output rows and takes the next entry; then, with `fin`, the terminal rows are copied as under
 * FTL_STEP_AUTO_RESET; then the masked reset pass of ftl_step_final places the slots that took an entry (`out` keeps the terminal reward /
 * done / status and gets the new episode's observation, as under FTL_STEP_AUTO_RESET).  fin->ended = a record was written, fin->restarted =
 * a new entry was taken.  Within one call the finishing slots take entries in ascending slot order: base = fetch-add(head, number of
 * finishing slots), once per call, then base + rank; an entry index >= n is not taken -- the slot parks.  One handle is therefore
 * deterministic down to which slot played what.  Several handles (the parts of a pipelined batch) may share head, records and the entry
 * arrays, each with a ticket array of its own: then who plays what depends on timing, the records do not.
 * A world that is done at reset (empty route, ENV:508-510) is recorded by the next call with frames 0, calls 0, ret 0, status 0/0/0 and
 * FTL_EPISODE_DONE_AT_RESET, and counts as one episode in "ep_stats"; `errors` then holds what that one call raised.
 * "ep_stats", FTL_EI_EPISODES and the sticky error word keep their bookkeeping: ftl_episode_metrics over a drained queue equals the column
 * sums of the records.  Combined with another reset flag: FTL_E_INVALID; without a queue attached: FTL_E_STATE.
 * ftl_set_episode_queue copies the struct (the arrays stay the caller's, alive and unchanged while attached; head and ticket are written by
 * the library only, records too); it touches no device memory.  NULL detaches: the handle is then exactly what it was before. */
#define FTL_STEP_QUEUE_RESET 8u
#define FTL_EPISODE_DONE_AT_RESET 1u
typedef struct ftl_episode_record {   /* one row per queue entry, written once */
    int32_t state;        /* 0 not started, 1 running, 2 finished */
    int32_t scenario;     /* pool index it ran on */
    int32_t env;          /* slot of the handle that ran it */
    int32_t frames;       /* step_count at done (ENV:944) */
    int32_t calls;        /* ftl_step* calls the episode took (while state is 1: the handle's call counter when the entry was taken) */
    int32_t status[3];    /* mission / agent / leader status of the terminal step */
    uint32_t errors;      /* FTL_ERR_* bits the episode raised */
    uint32_t flags;       /* FTL_EPISODE_DONE_AT_RESET: the world was done at reset */
    double  ret;          /* overall_reward at done (ENV:943) */
    int64_t stream;       /* the stream id it was played with */
} ftl_episode_record;
size_t ftl_sizeof_episode_record(void);

typedef struct ftl_episode_queue {    /* all pointers are DEVICE pointers the caller owns */
    const int32_t* scenario;   /* [Q] */
    const int64_t* stream;     /* [Q] or NULL: stream id of entry q = stream_base + q */
    int64_t  stream_base;
    int32_t  n;                /* Q */
    int32_t  _pad;
    int32_t* head;             /* [1]  next entry to hand out; may be SHARED by several handles */
    ftl_episode_record* records;  /* [Q] */
    int32_t* ticket;           /* [n_envs] entry each slot is playing, -1 = parked */
} ftl_episode_queue;
size_t ftl_sizeof_episode_queue(void);

int ftl_set_episode_queue(ftl_handle* h, const ftl_episode_queue* q);   /* NULL detaches */
int ftl_queue_start(ftl_handle* h, const ftl_outputs* out, void* stream);

/* ---- scenario sampler: a finished env draws its next world from caller-controlled weights; per-scenario outcome table (curricula,
 * prioritised level replay, "more of what the policy fails on") ------------------------------------------------------------------------
 * The fourth reset discipline.  FTL_STEP_AUTO_RESET / FTL_STEP_NEXT_RESET restart a finished env from a fixed arithmetic walk over the
 * reset window, the episode queue plays a finite list once; here the caller attaches uint32 weights over the pool entries
 * [base, base + count) and an int64 table of [count][FTL_N_SCEN_STATS], both in device memory it owns, and every env that finishes
 *   - adds the episode it just ended to the table row of the scenario it ran on, and
 *   - restarts on pool entry base + ftl_sample_scenario(rng_seed, its global stream id, its FTL_EI_RESETS word, cdf, count)
 * inside the step call, without the host.  The draw is a pure function of state words (above), so a run is reproducible whatever the
 * batch layout, and integer: a weight of 0 is never drawn.  Unlike the queue this is an ordinary auto-reset -- the bookkeeping of
 * FTL_STEP_AUTO_RESET (FTL_EI_EPISODES + 1, error bits into the sticky word, FTL_EI_RESETS advanced by the reset): FTL_EI_RESETS, FTL_EI_FPS,
 * FTL_EI_ACC_CONSUMED and FTL_EI_STREAM are left alone, the slot's random streams go on.
 *
 * Equivalence (the contract): a batch reset with ftl_sampler_start and stepped with FTL_STEP_SAMPLE_RESET gives, call for call, the
 * outputs and the state of a batch that is stepped without auto-reset and whose host calls ftl_reset(scen, mask = done) after every step
 * with scen = base + ftl_sample_scenario on the slot's own words -- except FTL_EI_EPISODES, which a plain ftl_reset does not count.
 *
 * Table columns, all int64 so that sums are exact and independent of order: FTL_SS_EPISODES; FTL_SS_FRAMES_SUM (step_count at done);
 * FTL_SS_SUCCESS / CRASH / LOW_REWARD / TOO_FAR / TIMEOUT (the predicates of FTL_M_*); FTL_SS_RETURN_Q16 = sum of llrint(overall_reward *
 * 65536), round to nearest even; FTL_SS_DONE_AT_RESET; FTL_SS_LAST_CALL = the largest value of the handle's sample-call counter (the number
 * of FTL_STEP_SAMPLE_RESET calls since the sampler was attached, this one included) at which an episode on the scenario ended (0: none
 * yet).  Rows are updated with agent-scope atomics (add / max on 64-bit integers), so several handles -- the parts of a pipelined batch --
 * may share one table and one cdf and still get the same bits.  An episode whose scenario lies outside [base, base + count) is not
 * recorded (it was drawn before the window moved).  A world that is done at reset (empty route, ENV:508-510) counts in FTL_SS_EPISODES and
 * FTL_SS_DONE_AT_RESET only and as one episode in "ep_stats", as for the queue.  The caller zeroes the table; the library only adds.
 *
 * ftl_set_scenario_sampler copies the struct and touches no device memory (the arrays stay the caller's, alive while attached; cdf is
 * written by the library only); it resets the sample-call counter.  NULL detaches: the handle is then exactly what it was before.
 * FTL_E_INVALID: NULL weight / cdf / table, count <= 0, base < 0, cdf or table not 8-byte aligned.  base + count <= n_scenarios is checked
 * against the pool when a sampling call is issued (FTL_E_INVALID there).
 * ftl_sampler_refresh rebuilds cdf from weight on `stream` (ftl_sampler_scan_kernel): call it once after attach and after every change
 * of the weights; a step issued later on the same stream sees the new cdf.  Handles that share a cdf on other streams must be ordered
 * after it by the caller.
 * ftl_sampler_start is the sampler's ftl_reset: every slot draws with the FTL_EI_RESETS / FTL_EI_STREAM words its state holds (0 in a fresh
 * buffer) and ftl_reset runs on those indices.  No table update.
 * FTL_STEP_SAMPLE_RESET (ftl_step / ftl_step_encoded / ftl_step_final): a step without auto-reset (the sensors scan the terminal state),
 * then ftl_sampler_kernel -- every slot whose done byte is set after the step records its episode and draws --, then with `fin` the
 * terminal-row copy as under FTL_STEP_AUTO_RESET, then the masked reset pass.  `out` keeps the terminal reward / done / status and gets
 * the new episode's observation; fin->ended = fin->restarted = the slot's done byte was set after the step.  A slot that an earlier plain
 * step (or a done-at-reset world) left done is recorded and restarted like any other: mixing reset disciplines on one handle is the
 * caller's business.  Combined with another reset flag: FTL_E_INVALID; without a sampler attached: FTL_E_STATE. */
#define FTL_STEP_SAMPLE_RESET 16u
#define FTL_N_SCEN_STATS 10
enum { FTL_SS_EPISODES = 0, FTL_SS_FRAMES_SUM, FTL_SS_SUCCESS, FTL_SS_CRASH, FTL_SS_LOW_REWARD, FTL_SS_TOO_FAR, FTL_SS_TIMEOUT,
       FTL_SS_RETURN_Q16, FTL_SS_DONE_AT_RESET, FTL_SS_LAST_CALL };
typedef struct ftl_scenario_sampler {   /* all pointers are DEVICE pointers the caller owns */
    const uint32_t* weight;    /* [count] */
    uint64_t* cdf;             /* [count] inclusive prefix sums of weight, written by the library only (ftl_sampler_refresh) */
    int32_t  base, count;      /* the pool entries [base, base + count) the weights cover */
    int64_t* table;            /* [count][FTL_N_SCEN_STATS]; may be SHARED by several handles */
} ftl_scenario_sampler;
size_t ftl_sizeof_scenario_sampler(void);

int ftl_set_scenario_sampler(ftl_handle* h, const ftl_scenario_sampler* s);   /* NULL detaches */
int ftl_sampler_refresh(ftl_handle* h, void* stream);
int ftl_sampler_start(ftl_handle* h, const ftl_outputs* out, void* stream);

const char* ftl_last_error(void);

/* indices into the "env_int" state field */
enum {
    FTL_EI_SCEN = 0, FTL_EI_TARGET_ID, FTL_EI_LEADER_FINISHED, FTL_EI_DONE, FTL_EI_CRASH, FTL_EI_IN_BOX,
    FTL_EI_ON_TRACE, FTL_EI_TOO_CLOSE, FTL_EI_STEP_COUNT, FTL_EI_FINISH_TIMER, FTL_EI_TRAJ_LEN,
    FTL_EI_TRK_COUNTER, FTL_EI_CORR_LO, FTL_EI_CORR_HI, FTL_EI_SEED_END, FTL_EI_SNAP_COUNT,
    FTL_EI_DYN_INDEX0, FTL_EI_DYN_INDEX1, FTL_EI_DYN_INDEX2, FTL_EI_DYN_INDEX3, FTL_EI_DYN_INDEX4, FTL_EI_DYN_INDEX5,
    FTL_EI_ERROR, FTL_EI_EPISODES, FTL_EI_GREEN_COUNT, FTL_EI_GREEN_LEN,
    FTL_EI_SCAN_OK,   /* bit g set: the ray sensors of dict-order group g (before / after the tracker's 2nd scan) scanned this step */
    FTL_EI_SNAP_HEAD, /* ring slot the next snapshot goes to (= snap_count mod max_prev_obs, kept incrementally) */
    FTL_EI_HINT,      /* index of a trajectory point that was close to the follower last frame (search hint only) */
    FTL_EI_GREEN_TINY, /* the green window may hold a segment so short that f64 sums of segment lengths are no longer exact */
    FTL_EI_RESETS,     /* number of resets of this env slot so far (keys the RNG stream of the episode) */
    FTL_EI_ACC_CONSUMED, /* bit i: entry i of leader_acceleration_regime was consumed -- the reference deletes the key for good (ENV:1170) */
    /* search caches of _check_agent_position (float bit patterns; they never change a result, only which points are looked at):
       coordinates of trajectory point FTL_EI_HINT, and lower bounds on the follower's distance to every green point /
       to every trajectory point */
    FTL_EI_HINT_X, FTL_EI_HINT_Y, FTL_EI_CLR_GREEN, FTL_EI_CLR_ALL,
    FTL_EI_FPS,        /* frames of the NEXT step of this env under random_frames_per_step (drawn at the end of a step, ENV:939-940;
                          kept across resets like the reference's attribute; 0 = not drawn yet) */
    FTL_EI_HW0_LO, FTL_EI_HW0_HI, /* tracker history window after the FIRST tracker scan of the step (what a detector that precedes the tracker
                          in dict order sees); after the second one it is FTL_EI_CORR_LO / FTL_EI_CORR_HI */
    FTL_EI_HIST1_LEN,   /* v1 tracker: points in the "hist1" field */
    FTL_EI_ERROR_STICKY, /* OR of every FTL_ERR_* bit this env slot ever raised: survives reset / auto-reset (FTL_EI_ERROR is per
                          episode); cleared by ftl_episode_metrics(FTL_METRICS_CLEAR) */
    FTL_EI_STREAM,      /* offset of the env's random stream from its own global index: every draw of the step kernels is keyed by
                          env_id_base + env + this word (0 in a zeroed state: the env's own stream).  Written only by ftl_unpack_envs;
                          reset / auto-reset keep it, like FTL_EI_RESETS */
    FTL_EI_COUNT
};
/* indices into the "env_dbl" state field; bear waypoints follow at FTL_ED_BEAR_POINTS + 2*b */
enum { FTL_ED_ACC_PENALTY = 0, FTL_ED_OVERALL_REWARD, FTL_ED_SPARE0, FTL_ED_SPARE1, FTL_ED_BEAR_POINTS,
       FTL_ED_GREEN_W = FTL_ED_BEAR_POINTS + 2 * FTL_MAX_BEARS, /* running length of the green-zone window (search acceleration) */
       FTL_ED_CUR_MULT,  /* cur_speed_multiplier (ENV:412, 449, 1150-1156) */
       FTL_ED_CUR_ACC, FTL_ED_CUM_SPEED, /* cur_leader_acceleration, cur_leader_cumulative_speed (ENV:591-592, 1167-1172) */
       FTL_ED_COUNT };
/* per robot: rb_dbl[5] and rb_int[8].  FTL_RI_SPARE0/1 of robots 0 and 1 carry the v2 tracker's running corridor length (search
   acceleration, like FTL_ED_GREEN_W): robot 0 the high / low word of the float64 length of the history window, robot 1 the window
   (corr_lo, corr_hi) it belongs to -- (x, -1): none is kept.  Zeroed or foreign words are re-derived by the next saving scan. */
enum { FTL_RD_DIRECTION = 0, FTL_RD_SPEED, FTL_RD_ROT_SPEED, FTL_RD_DES_SPEED, FTL_RD_DES_ROT_SPEED, FTL_RD_COUNT };
enum { FTL_RI_X = 0, FTL_RI_Y, FTL_RI_W, FTL_RI_H, FTL_RI_ROT_DIR, FTL_RI_DES_ROT_DIR, FTL_RI_SPARE0, FTL_RI_SPARE1, FTL_RI_COUNT };

#ifdef __cplusplus
}
#endif
#endif /* FTL_H */
