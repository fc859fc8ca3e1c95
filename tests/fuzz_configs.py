"""The seeded draws of the config space that tests/test_gpu_fuzz.py walks through.  Importable without a GPU (numpy only): the generator
of the reference records (tests/golden/gen/make_golden.py --fuzz) and the tests that replay them (tests/test_oracle_fuzz_golden.py,
tests/test_gpu_config_space_golden.py) rebuild the same configs from the same seeds.  tests/test_oracle_fuzz_golden.py pins every draw to
the `meta["kwargs"]` of its record, so an edit here has to come with regenerated fixtures."""
import numpy as np

TRACKER = dict(sensor_class="LeaderPositionsTracker_v2", eat_close_points=False, generate_corridor=True, saving_period=8,
               start_corridor_behind_follower=True, corridor_length=250, corridor_width=30)


def _ray_sensor(rng, kind):
    react = dict(react_to_green_zone=bool(rng.integers(2)), react_to_safe_corridor=bool(rng.integers(2)),
                 react_to_obstacles=[True, False, "static", "dynamic", "all"][rng.integers(5)])
    if not (react["react_to_green_zone"] or react["react_to_safe_corridor"] or react["react_to_obstacles"]):
        react["react_to_safe_corridor"] = True
    if kind == "prev":
        return dict(sensor_class="LeaderCorridor_Prev_lasers_v2", lasers_count=int(rng.choice([12, 20, 24, 36])),
                    laser_length=int(rng.integers(60, 220)), max_prev_obs=int(rng.integers(1, 13)), use_prev_obs=True,
                    pad_sectors=bool(rng.integers(3) == 0), **react)
    if kind == "v2":
        return dict(sensor_class="LeaderCorridor_lasers_v2", lasers_count=int(rng.choice([12, 20, 24, 36])),
                    laser_length=int(rng.integers(60, 220)), **react)
    if kind == "front":
        return dict(sensor_class="LeaderCorridor_lasers", front_lasers_count=int(rng.choice([3, 5])), back_lasers_count=int(rng.choice([0, 2])),
                    laser_length=int(rng.integers(60, 180)), **react)
    return dict(sensor_class="LeaderCorridor_lasers_compas", lasers_count=int(rng.choice([12, 20, 36])), laser_length=int(rng.integers(60, 160)),
                max_prev_obs=int(rng.integers(1, 9)), pad_sectors=False, react_to_green_zone=True, react_to_safe_corridor=True,
                react_to_obstacles=False)


def _aux_sensor(rng, kind):
    if kind == "lidar":
        return dict(sensor_class="LaserSensor", available_angle=int(rng.choice([90, 180, 360])), angle_step=int(rng.choice([10, 15, 30])),
                    points_number=int(rng.choice([8, 10, 20])), sensor_range=int(rng.integers(2, 6)), return_only_distances=bool(rng.integers(2)))
    if kind == "vector":
        return dict(sensor_class="LeaderTrackDetector_vector", position_sequence_length=int(rng.integers(4, 40)),
                    detectable_positions=["new", "old"][rng.integers(2)])
    return dict(sensor_class="LeaderTrackDetector_radar", position_sequence_length=int(rng.integers(4, 40)),
                detectable_positions=["new", "old", "near"][rng.integers(3)], radar_sectors_number=int(rng.choice([8, 18, 36])))


def draw_config(seed):
    rng = np.random.default_rng(1000 + seed)
    entries = []
    for k in range(int(rng.integers(1, 4))):                    # 1-3 segment ray sensors
        entries.append(("rays%d" % k, _ray_sensor(rng, ["prev", "prev", "v2", "front"][rng.integers(4)])))
    if rng.integers(3) == 0:
        entries.append(("compas", _ray_sensor(rng, "compas")))
    for k in range(int(rng.integers(0, 3))):                    # 0-2 of lidar / leader-track detectors
        entries.append(("aux%d" % k, _aux_sensor(rng, ["lidar", "vector", "radar"][rng.integers(3)])))
    order = rng.permutation(len(entries))
    at = int(rng.integers(0, len(entries) + 1))                 # the tracker's dict position: sensors before it see the first scan only
    sensors = {}
    for pos, j in enumerate(order):
        if pos == at:
            sensors["LeaderPositionsTracker_v2"] = dict(TRACKER, saving_period=int(rng.choice([4, 8])))
        sensors[entries[j][0]] = entries[j][1]
    if "LeaderPositionsTracker_v2" not in sensors:
        sensors["LeaderPositionsTracker_v2"] = dict(TRACKER, saving_period=int(rng.choice([4, 8])))
    bears = int(rng.integers(0, 5))
    hist = max([s.get("max_prev_obs", 1) for s in sensors.values()] + [1])
    if hist * (1 + bears) > 64:                                 # one wavefront of snapshot rects (ftl_create rejects more)
        bears = 64 // hist - 1
    kw = dict(follower_sensors=sensors, bear_number=bears, add_bear=bears > 0, obstacle_number=int(rng.choice([10, 35, 60])),
              frames_per_step=int(rng.choice([3, 5, 10])), max_distance=float(rng.choice([3, 4, 5])), min_distance=float(rng.choice([0.5, 1, 1.5])),
              max_dev=float(rng.choice([0.5, 1, 1.5])), warm_start=int(rng.choice([0, 50, 500])), max_steps=int(rng.choice([120, 5000])),
              aggregate_reward=bool(rng.integers(4) == 0), move_bear_v4=bool(rng.integers(2)), rng_seed=int(seed), env_id_base=100 * seed)
    if rng.integers(3) == 0:
        kw["leader_speed_regime"] = {0: [0.2, 1], 60: 0.5, 150: [0.6, 1.0]}
    if rng.integers(4) == 0:
        kw["leader_acceleration_regime"] = {0: 0, 40: 0.002, 90: -0.002, 140: 0}
    if rng.integers(4) == 0:
        kw["random_frames_per_step"] = [3, 9]
    if rng.integers(3) == 0:
        kw["early_stopping"] = {"max_distance_coef": 1.5, "low_reward": -80}
    return kw
