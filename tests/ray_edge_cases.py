"""Crafted worlds that drive ftl_rays_kernel (csrc/ftl_device.hpp) to the edges of its tables and lists: the merged / split source layout
of phase 1, more than one and two wavefronts of static rects inside the reach box, class runs that end on the last lane of a chunk, a
candidate list that overflows in either form, arcs that wrap at every ray index, rects at the cull boxes, 1023 rays, the largest
static list ftl_create accepts.  Importable without a GPU (numpy, the oracle and the host library only).  A case is a dict

    name, cfg, scen (keyword dicts of OracleEnv.reset, one per env), n, steps, actions(t) -> [n, 2], twins ([{switch: value}, ...]),
    golden (the envs tests/golden/ray_edges.npz records), trace (per env the oracle's state and readings after the reset and every
    step), expect (what tests/test_ray_edges_host.py asserts of it)

get_case(name) builds it.  Every env is SETTLED while it is built: the builder steps one oracle env through the case and moves the
world (another seed, another sub-pixel start of the follower) until no rect corner and no corridor vertex comes within MARGIN_BUILD of a
ray in any compared step -- the margin condition tests/test_ray_edges_host.py then asserts at MARGIN, so that no reading compared on
these worlds is a knife edge.  `table_counts` restates the COUNTING of phases 1 and 3 in numpy (float32 comparisons as the kernel writes
them); it only proves that a world has the shape a case names and never judges a reading."""
from collections import OrderedDict

import numpy as np

from aux_edge_cases import _config, _route_head, pool_b_scenarios, scenario_pool  # noqa: F401  (scenario_pool: for the GPU tests)
from fuzz_configs import TRACKER

FTL_WAVE, FTL_PAIR_CAP = 64, 192          # csrc/ftl_device.hpp
TRK = "LeaderPositionsTracker_v2"
SHIFT = (0.37, 0.21)                      # follower starts off the 5-px lattice and off the integer diagonals of everything else
MARGIN, MARGIN_BUILD = 1e-3, 1.05e-3      # px; 1000 x the 1e-6 that tests/test_gpu_configs.py::_corner_grazes calls a knife edge
_BASE = []


def prev(count, length=150, H=5, obstacles=True, green=False, corridor=False, pad=False, offset=-45):
    """A LeaderCorridor_Prev_lasers_v2 entry; obstacles-only unless said otherwise."""
    return dict(sensor_class="LeaderCorridor_Prev_lasers_v2", react_to_obstacles=obstacles, react_to_green_zone=green,
                react_to_safe_corridor=corridor, lasers_count=count, laser_length=length, max_prev_obs=H, use_prev_obs=True,
                pad_sectors=pad, first_laser_angle_offset=offset, _allow_any_lasers_count=count not in (12, 20, 24, 36))


def config(before, after, bears, n_static, **kw):
    """Config B's world with `n_static` static rects, `bears` bears and the ray sensors `before` / `after` the tracker ([(name, spec)])."""
    sensors = OrderedDict(list(before) + [(TRK, dict(TRACKER))] + list(after))
    bear_kw = dict(bear_number=bears) if bears else dict(add_bear=False)
    return _config(n_static=n_static, follower_sensors=sensors, **bear_kw, **kw)


# ---- the kernel's counting, restated ----------------------------------------------------------------------------------------------------
def _ltrb(rects):
    q = np.asarray(rects, np.int64).reshape(-1, 4)
    return q[:, 0].astype(np.float32), q[:, 1].astype(np.float32), (q[:, 0] + q[:, 2]).astype(np.float32), (q[:, 1] + q[:, 3]).astype(np.float32)


def in_box(fpos, rects, reach):
    """push_rect's cull, float32 as written: the rects [n, 4] that are NOT wholly outside the box of `reach` around the follower."""
    cx, cy, reach = np.float32(fpos[0]), np.float32(fpos[1]), np.float32(reach)
    l, t, r, b = _ltrb(rects)
    return ~((r < cx - reach) | (l > cx + reach) | (b < cy - reach) | (t > cy + reach))


def facing_edges(fpos, rects):
    """Edges of each rect that push_rect lists: popcount of its four side tests, all four when none holds (follower inside or on the rect)."""
    cx, cy = np.float32(fpos[0]), np.float32(fpos[1])
    l, t, r, b = _ltrb(rects)
    em = (cy > b).astype(int) + (cx > r) + (cy < t) + (cx < l)
    return np.where(em == 0, 4, em)


def class_reach(cfg, which):
    """P.cls_reach[which] of ftl_create: per segment class (static, dynamic, corridor, green) the longest float32 laser_length + 2 among
    the pass's sensors that react to it, or -1."""
    out = [-1.0] * 4
    for l in cfg.lasers:
        if int(bool(l.after_tracker)) != which or l.compas:
            continue
        sees = (l.react_obstacles in (1, 2), l.react_obstacles in (1, 3), bool(l.react_corridor), bool(l.react_green))
        for q in range(4):
            if sees[q]:
                out[q] = max(out[q], float(np.float32(l.length) + np.float32(2.0)))
    return out


def _seg_outside(fpos, reach, seg):
    cx, cy, reach = np.float32(fpos[0]), np.float32(fpos[1]), np.float32(reach)
    ax, ay, bx, by = (np.float32(v) for v in seg)
    x0, x1, y0, y1 = cx - reach, cx + reach, cy - reach, cy + reach
    return bool((ax < x0 and bx < x0) or (ax > x1 and bx > x1) or (ay < y0 and by < y0) or (ay > y1 and by > y1))


def table_counts(cfg, state):
    """Per pass (0: sensors before the tracker, 1: after) what phases 1 and 3 of the ray kernel count on `state`:

        fpos [2] float32, static [n_static, 4], snaps: the hitboxes [R - 1, 4] (leader, bears) of the valid snapshots, newest first,
        corr: [n, 4] the corridor of the newest snapshot (right x, y, left x, y) -- used only while there is ONE snapshot (the reset)

    -> dict(static_in, leaders_in, dynamic_in: rects inside their class box; static_edges, dynamic_edges: their facing edges; corridor,
    green: entries (None past the reset); n_items).  None for a pass without rays."""
    out = []
    fpos, st, snaps = state["fpos"], np.asarray(state["static"]).reshape(-1, 4), [np.asarray(s).reshape(-1, 4) for s in state["snaps"]]
    for which in (0, 1):
        if not any(int(bool(l.after_tracker)) == which and not l.compas for l in cfg.lasers):
            out.append(None)
            continue
        rs, rd, rc, rg = class_reach(cfg, which)
        lead = np.stack([s[0] for s in snaps])
        bears = np.concatenate([s[1:] for s in snaps]) if snaps[0].shape[0] > 1 else np.zeros((0, 4), np.int64)
        d = dict(static_in=0, leaders_in=0, dynamic_in=0, static_edges=0, dynamic_edges=0)
        if rs >= 0:
            m, ml = in_box(fpos, st, rs), in_box(fpos, lead, rs)
            d.update(static_in=int(m.sum()), leaders_in=int(ml.sum()),
                     static_edges=int(facing_edges(fpos, st)[m].sum() + facing_edges(fpos, lead)[ml].sum()))
        if rd >= 0 and len(bears):
            m = in_box(fpos, bears, rd)
            d.update(dynamic_in=int(m.sum()), dynamic_edges=int(facing_edges(fpos, bears)[m].sum()))
        if len(snaps) == 1 and state.get("corr") is not None:
            c = np.asarray(state["corr"], np.float64).reshape(-1, 4).astype(np.float32)
            d["corridor"] = 0 if rc < 0 else sum(int(not _seg_outside(fpos, rc, (c[p, s], c[p, s + 1], c[p + 1, s], c[p + 1, s + 1])))
                                                 for p in range(len(c) - 1) for s in (0, 2))
            d["green"] = 0 if rg < 0 or len(c) == 0 else sum(int(not _seg_outside(fpos, rg, c[p])) for p in (0, len(c) - 1))
            d["n_items"] = d["static_edges"] + d["dynamic_edges"] + d["corridor"] + d["green"]
        else:
            d["corridor"] = d["green"] = d["n_items"] = None
        out.append(d)
    return out


# ---- the oracle's trace of one env, and the margin condition on it ------------------------------------------------------------------------
def trace(cfg, scen, actions, env_id=0):
    """Oracle env `env_id` (its index in the batch: the stream of the bears' random draws) through the reset and the steps `actions`
    [steps, 2]: per compared state fpos (float32), fdir, boxes [R, 4], corr [n, 4], lasers, done, err."""
    from oracle import OracleEnv
    o = OracleEnv(cfg, env_id=env_id)
    o.reset(**scen)
    recs = []

    def rec():
        d = o.debug()
        recs.append(dict(fpos=d["robot_pos"][1].copy(), fdir=float(d["robot_f64"][1, 0]), boxes=d["robot_i32"][:, :4].copy(), corr=d["corr"].copy(),
                         lasers=o.lasers[:cfg.lasers_len].copy(), done=int(d["counters"][9]), err=int(d["counters"][14])))
    rec()
    for a in actions:
        o.step(a)
        rec()
    return recs


def _corners(rects):
    q = np.asarray(rects, np.float64).reshape(-1, 4)
    return np.concatenate([np.stack([q[:, 0] + i * q[:, 2], q[:, 1] + j * q[:, 3]], 1) for i in (0, 1) for j in (0, 1)])


def snapshots(recs, t, H):
    """Hitboxes (leader, bears) of the snapshots valid at state `t`, newest first."""
    return [np.delete(r["boxes"], 1, 0) for r in recs[max(0, t - H + 1):t + 1][::-1]]


def ray_angles(l, fdir):
    """Directions of the rays of sensor `l` in degrees (screen coordinates, y down)."""
    rel = np.array(l.ray_angles, np.float64) if l.ray_angles else l.angle_offset + np.arange(l.count) * (360.0 / l.count)
    return fdir + rel


def margin(cfg, recs, t, static, per_class=False):
    """Float64: the smallest distance of a rect corner (static rects, the hitboxes of the valid snapshots) or a corridor vertex (of the
    valid snapshots) to a ray segment [origin, end] of ANY sensor at state `t` of the trace.  `per_class` (group D alone): a point counts
    against the rays of the sensors that react to its class only -- static rects and the leader, bears, the corridor with its end caps.
    (One world under 720 headings half a degree apart: config B's corridor puts some 200 vertices around the follower, and with the ring's
    132 corners no sub-pixel start keeps all of them off every ray of every heading; D's sensors react to obstacles only.)"""
    H = max(l.history for l in cfg.lasers)
    past = recs[max(0, t - H + 1):t + 1]
    cls = [np.concatenate([_corners(static)] + [_corners(r["boxes"][:1]) for r in past]),
           np.concatenate([_corners(r["boxes"][2:]) for r in past]),
           np.concatenate([np.asarray(r["corr"], np.float64).reshape(-1, 2) for r in past])]
    best = np.inf
    for l in cfg.lasers:
        if l.compas:
            continue
        sees = (l.react_obstacles in (1, 2), l.react_obstacles in (1, 3), bool(l.react_corridor) or bool(l.react_green)) if per_class else (True,) * 3
        pts = [cls[q] for q in range(3) if sees[q] and len(cls[q])]
        if not pts:
            continue
        rel = np.concatenate(pts) - recs[t]["fpos"].astype(np.float64)
        a = np.radians(ray_angles(l, recs[t]["fdir"]))
        d = np.stack([np.cos(a), np.sin(a)], 1) * l.length
        tt = np.clip((rel @ d.T) / (l.length * l.length), 0.0, 1.0)
        best = min(best, float(np.hypot(rel[:, None, 0] - tt * d[None, :, 0], rel[:, None, 1] - tt * d[None, :, 1]).min()))
    return best


def newest_row(cfg, l, lasers):
    """The newest row [count] of sensor `l` in an env's readings (pad_sectors: the four sector blocks summed back into one row)."""
    row = lasers[l.out_offset + (l.history - 1) * l.width:l.out_offset + l.history * l.width]
    return row.reshape(4, l.count).sum(0) if l.pad_sectors else row


# ---- worlds -----------------------------------------------------------------------------------------------------------------------------
def base(i, bears, shift=SHIFT, near=True):
    """pool_B scenario `i` with its follower moved to floor(position) + `shift` and `bears` bears on a circle of 62-97 px around the
    follower, behind and beside it (`near` False: the pool's own single bear, where the pool put it)."""
    if not _BASE:
        _BASE.extend(pool_b_scenarios(32))
    s = {k: np.array(v) for k, v in _BASE[i % len(_BASE)].items()}
    s["robot_pos"] = s["robot_pos"].astype(np.float32)
    s["robot_pos"][1] = np.floor(s["robot_pos"][1]) + np.asarray(shift, np.float32)
    w, h = int(s["robot_rect"][2][2]), int(s["robot_rect"][2][3])
    pos, dirs, rects = list(s["robot_pos"][:2]), list(s["robot_dir"][:2]), list(s["robot_rect"][:2])
    f, head = s["robot_pos"][1].astype(np.float64), np.radians(float(s["robot_dir"][1]))
    for b in range(bears):
        if bears == 1 and not near:
            pos.append(s["robot_pos"][2]); dirs.append(s["robot_dir"][2]); rects.append(s["robot_rect"][2])
            continue
        ang = head + np.radians(180.0 if bears == 1 else 110.0 + 140.0 * b / (bears - 1))    # behind it: 110 .. 250 degrees off the heading
        p = np.floor(f + (62.0 + 7.0 * b) * np.array([np.cos(ang), np.sin(ang)]))
        pos.append(p.astype(np.float32)); dirs.append(s["robot_dir"][2])
        rects.append(np.array([int(p[0]) - w // 2, int(p[1]) - h // 2, w, h], np.int32))
    s["robot_pos"], s["robot_dir"], s["robot_rect"] = np.stack(pos).astype(np.float32), np.array(dirs, np.float64), np.stack(rects).astype(np.int32)
    return s


class Sites:
    """Integer rects around the follower of scenario `s` that leave the robots (hitboxes inflated by 14 px), the first 300 px of the
    route (25 px) and a lane 80 px ahead of the follower free, do not touch each other and lie inside the field."""

    def __init__(self, s, cfg, seed, lane=True):
        self.s, self.cfg, self.rng, self.lane, self.taken = s, cfg, np.random.default_rng(9100 + seed), lane, []
        self.f = s["robot_pos"][1].astype(np.float64)
        hd = np.radians(float(s["robot_dir"][1]))
        self.u = np.array([np.cos(hd), np.sin(hd)])
        self.head = _route_head(s["route"])
        self.boxes = np.asarray(s["robot_rect"], np.int64).reshape(-1, 4)

    def free(self, x, y, w, h, apart=True):
        c, bx = self.cfg.c, self.boxes
        if x < 1 or y < 1 or x + w > c.width - 1 or y + h > c.height - 1:
            return False
        if np.any((x < bx[:, 0] + bx[:, 2] + 14) & (x + w > bx[:, 0] - 14) & (y < bx[:, 1] + bx[:, 3] + 14) & (y + h > bx[:, 1] - 14)):
            return False
        gx = np.maximum(np.maximum(x - self.head[:, 0], self.head[:, 0] - (x + w)), 0.0)
        gy = np.maximum(np.maximum(y - self.head[:, 1], self.head[:, 1] - (y + h)), 0.0)
        if np.any(np.hypot(gx, gy) < 25.0):
            return False
        if self.lane:
            d = np.array([x + w / 2.0, y + h / 2.0]) - self.f
            along, across = d @ self.u, abs(d[0] * self.u[1] - d[1] * self.u[0])
            if -22.0 < along < 80.0 and across < 24.0 + w:
                return False
        if apart:
            for (tx, ty, tw, th) in self.taken:
                if x < tx + tw + 2 and x + w > tx - 2 and y < ty + th + 2 and y + h > ty - 2:
                    return False
        return True

    def take(self, x, y, w, h):
        self.taken.append((int(x), int(y), int(w), int(h)))
        return [int(x), int(y), int(w), int(h)]

    def ring(self, count, rmin, rmax, size=8, want=None):
        """`count` size x size rects whose centres lie `rmin`..`rmax` px from the follower (uniform over the area); `want(rect)` filters."""
        out = []
        for _ in range(400000):
            if len(out) == count:
                break
            rad, ang = np.sqrt(self.rng.uniform(rmin ** 2, rmax ** 2)), self.rng.uniform(0, 2 * np.pi)
            x, y = int(np.floor(self.f[0] + rad * np.cos(ang) - size / 2.0)), int(np.floor(self.f[1] + rad * np.sin(ang) - size / 2.0))
            if self.free(x, y, size, size) and (want is None or want([x, y, size, size])):
                out.append(self.take(x, y, size, size))
        assert len(out) == count, ("no room for the ring", count, len(out), rmin, rmax)
        return out

    def grid(self, count, rmin, size=6, pitch=8):
        """The `count` free cells of a `pitch`-px grid nearest to the follower beyond `rmin` px: a dense disc of size x size rects."""
        fx, fy = int(self.f[0]), int(self.f[1])
        k = np.arange(-60, 61) * pitch
        gx, gy = np.meshgrid(fx + k + int(self.rng.integers(pitch)), fy + k + int(self.rng.integers(pitch)))
        cells = np.stack([gx.ravel(), gy.ravel()], 1)
        dist = np.hypot(cells[:, 0] + size / 2.0 - self.f[0], cells[:, 1] + size / 2.0 - self.f[1])
        out = []
        for j in np.argsort(dist, kind="stable"):
            if len(out) == count:
                break
            if dist[j] >= rmin and self.free(int(cells[j, 0]), int(cells[j, 1]), size, size, apart=False):
                out.append([int(cells[j, 0]), int(cells[j, 1]), size, size])
        assert len(out) == count, ("no room for the grid", count, len(out))
        return out


def _still(cfg, n):
    return lambda t: np.zeros((n, 2))


def _drive(cfg, n, speed=1.0):
    ms, mr = cfg.c.follower.max_speed, cfg.c.follower.max_rotation_speed

    def act(t):
        a = np.zeros((n, 2))
        a[:, 0] = speed * ms
        a[:, 1] = np.where((np.arange(n) + t) % 2 == 0, mr, -mr)      # left and right in turn: the path stays in the free lane
        return a
    return act


def _case(name, cfg, n, steps, actions, make, twins=(), golden=2, accept=None, tries=400, per_class=False, **expect):
    """Builds and settles the envs: make(e, trial) is the scenario of env e at attempt `trial`."""
    scen, traces, trials = [], [], 0
    acts = np.stack([actions(t) for t in range(steps)]) if steps else np.zeros((0, n, 2))
    for e in range(n):
        for trial in range(tries):
            s = make(e, trial)
            recs = trace(cfg, s, acts[:, e], e)
            if all(margin(cfg, recs, t, s["static_rects"], per_class) >= MARGIN_BUILD for t in range(steps + 1)) and (accept is None or accept(e, s, recs)):
                break
        else:
            raise AssertionError((name, e, "no world within %d attempts keeps the margin" % tries))
        scen.append(s); traces.append(recs); trials += trial
    return dict(name=name, cfg=cfg, scen=scen, n=n, steps=steps, actions=actions, twins=list(twins), golden=list(range(min(golden, n))),
                trace=traces, trials=trials, per_class=per_class, expect=expect)


def _shift(trial):
    return (SHIFT[0] + 0.013 * (trial % 37), SHIFT[1] + 0.017 * (trial % 29))


# ---- group A: the source layout of phase 1 ----------------------------------------------------------------------------------------------
# (n_static, bears, H): n_static + H * (1 + bears) = 63, 64 (merged: one source per lane), 65 (split); one, two and three wavefronts of static
# rects and one more; the largest snapshot products ftl_create allows, each on either side of the merged / split boundary
A_SHAPES = [(39, 1, 12), (40, 1, 12), (41, 1, 12), (64, 1, 12), (65, 1, 12), (128, 1, 12), (129, 1, 12), (193, 1, 12),
            (1, 6, 9), (2, 6, 9), (4, 4, 12), (5, 4, 12)]
A_ENVS = 16


def group_a(shape, motion):
    n_static, bears, H = shape
    cfg = config([], [("rays", prev(36, 150, H))], bears, n_static)

    def make(e, trial):
        s = base(e, bears, _shift(trial))
        s["static_rects"] = np.array(Sites(s, cfg, e + 1000 * trial).ring(n_static, 30.0, 132.0), np.int32)
        return s
    act = _still(cfg, A_ENVS) if motion == "still" else _drive(cfg, A_ENVS)
    return _case("A-%d-%d-%d-%s" % (n_static, bears, H, motion), cfg, A_ENVS, H + 3, act, make, twins=[{"FTL_RAYS_ONE_PASS": "0"}], golden=8, group="A",
                 sources=n_static + H * (1 + bears))


# ---- group B: chunk and class-run edges of phase 3 --------------------------------------------------------------------------------------
B_ENVS, B_STATIC = 8, 84


def _edge_world(s, cfg, seed, target, reach):
    """B_STATIC rects of which those inside the box of `reach` show exactly `target` facing edges: rects diagonal to the follower (two
    edges), rects straight above, below or beside it (one), and the rest beyond the box."""
    S = Sites(s, cfg, seed)
    f = s["robot_pos"][1]
    ones = (target % 2) + (4 if target >= 5 else 0)
    twos = (target - ones) // 2
    assert target >= 0 and ones + 2 * twos == target and ones + twos <= B_STATIC, (target, ones, twos)
    out, fx, fy = [], int(np.floor(f[0])), int(np.floor(f[1]))
    arms = [(fx - 4, fy + d) for d in range(34, 130, 12)] + [(fx - 4, fy - d - 8) for d in range(34, 130, 12)] + \
           [(fx + d, fy - 4) for d in range(34, 130, 12)] + [(fx - d - 8, fy - 4) for d in range(34, 130, 12)]
    for k in S.rng.permutation(len(arms)):
        x, y = arms[k]
        if len(out) < ones and S.free(x, y, 8, 8) and facing_edges(f, [x, y, 8, 8])[0] == 1:
            out.append(S.take(x, y, 8, 8))
    assert len(out) == ones, ("no room on the axes", ones, len(out))
    out += S.ring(twos, 32.0, 130.0, want=lambda q: facing_edges(f, q)[0] == 2)
    out += S.ring(B_STATIC - len(out), reach + 30.0, reach + 260.0, want=lambda q: not in_box(f, q, reach)[0])
    return np.array(out, np.int32)[S.rng.permutation(B_STATIC)]


def group_b(kind, target):
    """kind "static": an obstacles="static" sensor and `target` facing edges in all (the leader's included).  kind "run-static" /
    "run-dynamic" / "run-corridor", a sensor that reacts to everything: that class run ends on item `target` - 1 of the table (64: the
    last lane of the first chunk, 65: the first lane of the second).  The other classes' counts come from the oracle's reset on the
    same world without near rects; should they alone pass `target`, the run ends a chunk later."""
    everything = kind.startswith("run-")
    sensor = prev(36, 150, 5, True, True, True) if everything else prev(36, 150, 5, "static")
    cfg = config([], [("rays", sensor)], 1, B_STATIC)

    def make(e, trial):
        s = base(e, 1, _shift(trial))
        s["static_rects"] = _edge_world(s, cfg, e + 1000 * trial, 0, 152.0)
        o = reset_counts(cfg, s)[1]
        lead = o["static_edges"]                                    # the leader's facing edges (no static rect is in the box yet)
        after = {"static": 0, "run-static": 0, "run-dynamic": o["dynamic_edges"], "run-corridor": o["dynamic_edges"] + o["corridor"]}[kind]
        want = target - lead - after
        s["static_rects"] = _edge_world(s, cfg, e + 1000 * trial, want if want >= 0 else want + FTL_WAVE, 152.0)
        return s
    return _case("B-%s-%d" % (kind, target), cfg, B_ENVS, 2, _drive(cfg, B_ENVS, 0.5), make, twins=[{"FTL_RAYS_ONE_PASS": "0"}], golden=B_ENVS,
                 group="B", kind=kind, target=target)


# ---- group C: the candidate list ------------------------------------------------------------------------------------------------------------
C_ENVS = 9
C_PASSES = OrderedDict([("12", (12,)), ("36", (36,)), ("40+24", (40, 24)), ("41+24", (41, 24)), ("180", (180,)), ("256", (256,))])
C_PLACES = ("inside", "border", "nested")


def _near_world(s, place):
    """Three static rects: `inside` -- a 40 x 40 rect around the follower; `border` -- a rect whose left edge runs through the follower's x
    (an integer); `nested` -- a 3 x 3 rect around the follower inside two 5 x 5 rects, each of which shares two edges with it: 8 edges
    within 2 px of the follower.  The rects a placement does not use lie beyond every reach."""
    f = s["robot_pos"][1]
    fx, fy = int(np.floor(f[0])), int(np.floor(f[1]))
    far = [[fx - 400 if fx > 700 else fx + 400, fy + 40 * k, 8, 8] for k in range(3)]
    if place == "inside":
        near = [[fx - 17, fy - 22, 40, 40]]
    elif place == "border":
        s["robot_pos"][1, 0] = np.float32(fx)
        near = [[fx, fy - 13, 30, 30]]
    else:
        s["robot_pos"][1] += np.float32(1.0)                          # (1.37, 1.21) inside the 3 x 3 rect at (fx, fy)
        near = [[fx, fy, 3, 3], [fx - 2, fy - 2, 5, 5], [fx, fy, 5, 5]]
    return np.array(near + far[:3 - len(near)], np.int32)


def edges_within_2px(fpos, rects):
    """Rect edges (of all four) whose closest approach to `fpos` is under 2 px, float64."""
    n = 0
    for x, y, w, h in np.asarray(rects, np.float64).reshape(-1, 4):
        for ax, ay, bx, by in ((x, y + h, x + w, y + h), (x + w, y, x + w, y + h), (x + w, y, x, y), (x, y + h, x, y)):
            ex, ey = bx - ax, by - ay
            t = np.clip(((fpos[0] - ax) * ex + (fpos[1] - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
            n += int(np.hypot(ax + t * ex - fpos[0], ay + t * ey - fpos[1]) < 2.0)
    return n


def group_c(passname, two_sided):
    """The follower in, on and next to static rects (it ignores collisions, so the envs stay alive, and turns on the spot) under
    the rays of C_PASSES[passname], all behind the tracker; `two_sided`: a 24-ray obstacles sensor ahead of the tracker as well (the loop
    form, pass_base > 0)."""
    counts = C_PASSES[passname]
    after = [("rays%d" % k, prev(c, 150 if k == 0 else 120, 3, True, k == 0, k == 0)) for k, c in enumerate(counts)]
    before = [("ahead", prev(24, 130, 3))] if two_sided else []
    cfg = config(before, after, 1, 3, ignore_follower_collisions=True)

    def make(e, trial):
        s = base(e, 1, _shift(trial))
        s["robot_dir"][1] += 3.7 + 0.61 * trial          # (the pool's headings are whole degrees: a ray would run along a rect edge)
        s["static_rects"] = _near_world(s, C_PLACES[e % 3])
        return s
    return _case("C-%s-%s" % (passname, "two" if two_sided else "one"), cfg, C_ENVS, 3, _drive(cfg, C_ENVS, 0.0), make,
                 twins=[{"FTL_DEBUG_PAIR_WINDOW": "16"}], golden=C_ENVS, group="C", rays=sum(counts))


# ---- group D: every bearing under every heading ---------------------------------------------------------------------------------------------
D_ENVS, D_THIN = 720, 8
_NOW = dict(sensor_class="LeaderCorridor_lasers_v2", react_to_obstacles=True, react_to_green_zone=False, react_to_safe_corridor=False,
            lasers_count=24, laser_length=120)
_EXPL = dict(sensor_class="LeaderCorridor_lasers", react_to_obstacles=True, react_to_green_zone=False, react_to_safe_corridor=False,
             front_lasers_count=5, back_lasers_count=2, laser_length=110)
D_CONFIGS = OrderedDict([("12pad+36", [("r12", prev(12, 100, 3, pad=True)), ("r36", prev(36, 120, 3))]),
                         ("20+24", [("r20", prev(20, 100, 3)), ("r24", prev(24, 120, 3))]),
                         ("now24+12", [("now24", dict(_NOW)), ("r12", prev(12, 100, 3))]),
                         ("expl7+12", [("expl", dict(_EXPL)), ("r12", prev(12, 100, 3))])])
D_BASE = 0


def d_world(s):
    """24 rects of 6 x 6 on a ring of radius 60 around the follower, every 15 degrees from 7 degrees, and 9 of them at radius 90 every 40
    degrees from 3: every ray of every sensor meets one under some heading."""
    f = s["robot_pos"][1].astype(np.float64)
    out = []
    for rad, k, a0 in ((60.0, 24, 7.0), (90.0, 9, 3.0)):
        for j in range(k):
            a = np.radians(a0 + j * 360.0 / k)
            out.append([int(np.floor(f[0] + rad * np.cos(a))) - 3, int(np.floor(f[1] + rad * np.sin(a))) - 3, 6, 6])
    return np.array(out, np.int32)


def group_d(which):
    """One world, 720 envs that differ in the follower's heading alone (0, 0.5, ..., 359.5 degrees), turning at full rate.  The world is
    settled as a whole: the follower's sub-pixel start moves until all 720 envs keep the margin."""
    cfg = config([], D_CONFIGS[which], 1, 33)
    mr = cfg.c.follower.max_rotation_speed
    act = lambda t: np.stack([np.zeros(D_ENVS), np.full(D_ENVS, mr)], 1)  # noqa: E731

    for trial in range(1000):
        def make(e, _):
            s = base(D_BASE, 1, _shift(trial), near=False)
            s["robot_dir"][1] = 0.5 * e
            s["static_rects"] = d_world(s)
            return s
        try:
            c = _case("D-" + which, cfg, D_ENVS, 2, act, make, twins=[{"FTL_RAYS_ONE_PASS": "0"}], golden=0, tries=1, per_class=True, group="D")
        except AssertionError:
            continue
        c["golden"], c["trials"] = list(range(0, D_ENVS, D_THIN)), trial
        return c
    raise AssertionError(("D", which, "no sub-pixel start keeps the margin under all headings"))


# ---- group E: the cull boxes ----------------------------------------------------------------------------------------------------------------
# two sensors of 24 rays from straight ahead (the follower heads along +x: rays along both axes and the diagonals), one sees the static
# class and one the dynamic class, lengths 100 and 150 and the other way round.  A rect's near edge lies OFFSETS px beyond the ray's
# length straight along an axis; on a diagonal the integer lattice allows (m + 0.5) * sqrt(2): the nearest of those on either side.
E_OFFSETS = (-0.5, 0.5, 1.5, 2.5)
E_DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
E_RAY = {(1, 0): 0, (1, 1): 3, (0, 1): 6, (-1, 1): 9, (-1, 0): 12, (-1, -1): 15, (0, -1): 18, (1, -1): 21}
E_ROLES = OrderedDict([("static100-dynamic150", (100, 150)), ("static150-dynamic100", (150, 100))])


def e_placements(length):
    """(direction, half-integer distance of the near edge from the follower along x and / or y, distance along the ray - length)."""
    out = []
    for d in E_DIRS:
        if 0 in d:
            out += [(d, length + o, o) for o in E_OFFSETS]
        else:
            m = int(np.floor(length / np.sqrt(2.0) - 0.5))
            out += [(d, m + k + 0.5, (m + k + 0.5) * np.sqrt(2.0) - length) for k in range(3)]
    return out


def _e_rect(f, d, gap, w, h):
    """The w x h integer rect whose near edge lies `gap` (half-integer) px from the half-integer point `f` in direction `d`: straight ahead
    it straddles the ray (3.5 px to one side); on a diagonal the ray crosses its near vertical edge 2 px from the corner."""
    x = f[0] + gap if d[0] > 0 else (f[0] - gap - w if d[0] < 0 else f[0] - 3.5)
    if d[0] == 0:
        y = f[1] + gap if d[1] > 0 else f[1] - gap - h
    elif d[1] == 0:
        y = f[1] - 3.5
    else:
        y = f[1] + gap - 2 if d[1] > 0 else f[1] - gap - h + 2
    assert x == int(x) and y == int(y)
    return [int(x), int(y), w, h]


def group_e(roles):
    ls, ld = E_ROLES[roles]
    cfg = config([], [("static", prev(24, ls, 2, "static", offset=0)), ("dynamic", prev(24, ld, 2, "dynamic", offset=0))], 1, 1)
    places = [("static",) + p for p in e_placements(ls)] + [("dynamic",) + p for p in e_placements(ld)]
    k_s, k_d = [k for k, l in enumerate(cfg.lasers)]

    def make(e, trial):
        cls, d, gap, _ = places[e]
        s = base(trial, 1, (0.5, 0.5), near=False)                     # another pool scenario per attempt: the leader and the bear stand elsewhere
        s["robot_dir"][1] = 0.0
        f = s["robot_pos"][1].astype(np.float64)
        far = [int(f[0]) + (420 if f[0] < 700 else -420), int(f[1]), 8, 8]
        if cls == "static":
            s["static_rects"] = np.array([_e_rect(f, d, gap, 8, 8)], np.int32)
        else:
            w, h = int(s["robot_rect"][2][2]), int(s["robot_rect"][2][3])
            q = _e_rect(f, d, gap, w, h)
            s["static_rects"] = np.array([far], np.int32)
            s["robot_rect"][2] = q
            s["robot_pos"][2] = (q[0] + w // 2, q[1] + h // 2)
        c = cfg.c
        ok = all(0 < r[0] and r[0] + r[2] < c.width and 0 < r[1] and r[1] + r[3] < c.height for r in (s["static_rects"][0], s["robot_rect"][2]))
        return s if ok else None

    def accept(e, s, recs):
        cls, d, gap, over = places[e]
        l, other = (cfg.lasers[k_s], cfg.lasers[k_d]) if cls == "static" else (cfg.lasers[k_d], cfg.lasers[k_s])
        got = newest_row(cfg, l, recs[0]["lasers"])[E_RAY[d]]
        mine = got < np.float32(l.length) if over < 0 else got == np.float32(l.length)
        # nothing else in the way: the other sensor's ray of the same direction sees nothing, and this sensor's ray sees nothing nearer
        return bool(mine) and (over > 0 or got > l.length - 1.0)
    c = _case("E-" + roles, cfg, len(places), 0, _still(cfg, len(places)), _retry(make), twins=[{"FTL_RAYS_CLASS_CULL": "0"}], golden=len(places),
              accept=accept, group="E")
    c["places"] = places
    return c


def _retry(make):
    """make(e, trial) may return None (the placement leaves the field on that pool scenario): take the next attempt that does not."""
    def wrapped(e, trial):
        k, seen = 0, -1
        while True:
            s = make(e, k)
            if s is not None:
                seen += 1
                if seen == trial:
                    return s
            k += 1
            assert k < 2000
    return wrapped


# ---- group G: limits ------------------------------------------------------------------------------------------------------------------------
G_ENVS, G_DENSE_ENVS = 8, 4


def group_g(passes):
    """1023 rays: 256 + 256 ahead of the tracker and 256 + 255 behind it (`passes` 2), or all four behind it (1)."""
    sens = [("g%d" % k, prev(c, 100 + 10 * k, 2)) for k, c in enumerate((256, 256, 256, 255))]
    cfg = config(sens[:2] if passes == 2 else [], sens[2:] if passes == 2 else sens, 1, 24)

    def make(e, trial):
        s = base(e, 1, _shift(trial))
        s["static_rects"] = np.array(Sites(s, cfg, e + 1000 * trial).ring(24, 30.0, 100.0), np.int32)
        return s
    return _case("G-1023-%dpass" % passes, cfg, G_ENVS, 3, _drive(cfg, G_ENVS, 0.5), make, twins=[{"FTL_RAYS_ONE_PASS": "0"}] if passes == 1 else [], golden=G_ENVS, group="G")


def too_many_rays_config():
    return config([], [("g%d" % k, prev(256, 100, 2)) for k in range(4)], 1, 24)


def dense_config(n_static):
    """A 12-ray sensor with one row of history over `n_static` static rects, no bears.  (Of the 64 KiB LDS rules of ftl_create the frame
    kernel's -- static rects x frames per step -- is the one that binds: the ray kernel's own table would take some 2,200 rects.)"""
    return config([], [("rays", prev(12, 100, 1))], 0, n_static)


def largest_n_static(lo=64, hi=1 << 15):
    """The largest n_static for which ftl_create accepts dense_config (bisection over its own answer); (n, the message one above it)."""
    import ctypes as C
    from continiousenvironment_follower_leader_amd import _lib
    lib = _lib.load()

    def ok(n):
        h = C.c_void_p()
        rc = lib.ftl_create(C.byref(dense_config(n).c), G_DENSE_ENVS, 0, C.byref(h))
        if rc == 0:
            lib.ftl_destroy(h)
            return True, ""
        return False, lib.ftl_last_error().decode()
    assert ok(lo)[0] and not ok(hi)[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid)[0] else (lo, mid)
    return lo, ok(hi)[1]


def group_g_dense(n_static):
    cfg = dense_config(n_static)

    def make(e, trial):
        s = base(e, 0, _shift(trial))
        s["static_rects"] = np.array(Sites(s, cfg, e + 1000 * trial).grid(n_static, 26.0), np.int32)
        return s
    return _case("G-dense-%d" % n_static, cfg, G_DENSE_ENVS, 2, _drive(cfg, G_DENSE_ENVS, 0.5), make, golden=G_DENSE_ENVS, group="G")


def case_names():
    """Every case but the dense one of group G, whose size comes from probing ftl_create (largest_n_static)."""
    names = ["A-%d-%d-%d-%s" % (s + (m,)) for s in A_SHAPES for m in ("still", "drive")]
    names += ["B-static-%d" % t for t in (63, 64, 65, 127, 128, 129)]
    names += ["B-run-%s-%d" % (k, t) for k in ("static", "dynamic", "corridor") for t in (64, 65)]
    names += ["C-%s-%s" % (p, o) for p in C_PASSES for o in ("one", "two")]
    names += ["D-" + k for k in D_CONFIGS]
    names += ["E-" + k for k in E_ROLES]
    names += ["G-1023-2pass", "G-1023-1pass"]
    return names


_CASES = {}


def get_case(name):
    """The case `name` (cached: worlds are built and settled once per session)."""
    if name in _CASES:
        return _CASES[name]
    g, rest = name.split("-", 1)
    if g == "A":
        n, b, h, m = rest.split("-")
        c = group_a((int(n), int(b), int(h)), m)
    elif g == "B":
        kind, target = rest.rsplit("-", 1)
        c = group_b(kind, int(target))
    elif g == "C":
        p, o = rest.rsplit("-", 1)
        c = group_c(p, o == "two")
    elif g == "D":
        c = group_d(rest)
    elif g == "E":
        c = group_e(rest)
    elif rest.startswith("dense"):
        c = group_g_dense(int(rest.split("-")[1]))
    else:
        c = group_g(2 if "2pass" in rest else 1)
    _CASES[name] = c
    return c


def state_at(case, e, t):
    """`state` of table_counts for env `e` of `case` at compared state `t` (0: the reset)."""
    recs, H = case["trace"][e], max(l.history for l in case["cfg"].lasers)
    return dict(fpos=recs[t]["fpos"], static=case["scen"][e]["static_rects"], corr=recs[t]["corr"], snaps=snapshots(recs, t, H))


def reset_counts(cfg, scen):
    """table_counts of scenario `scen` right after the reset, from a fresh oracle env."""
    recs = trace(cfg, scen, np.zeros((0, 2)))
    return table_counts(cfg, dict(fpos=recs[0]["fpos"], static=scen["static_rects"], corr=recs[0]["corr"], snaps=snapshots(recs, 0, 1)))
