"""Crafted scenes for the render kernels (tests/test_gpu_render_edges.py, tests/test_render_numpy_host.py).

A ``Spec`` holds, as host arrays, every word the render spec of include/ftl.h reads for one env: robot poses and hitboxes, the trajectory
with the green-zone words, the tracker's ring buffers with the corridor window, the env's own pool entry (route, static rects, start
position) and its row of ``lasers``.  ``Spec.scene()`` gives the dict ``render_numpy.scene_prims`` / ``render_scene`` take, without a
device; ``apply(env, e, spec)`` writes the same words into env ``e`` of a reset batch through ``state_field`` / ``pool.t`` / ``lasers``.
The GPU tests rebuild their reference from the device words (``render_numpy.env_scene``), the host tests from ``Spec.scene()``.

Dyadic scenes: every coordinate, size and radius is a multiple of 1/4 world px, robots head along +x (cos = 1, sin = 0 exactly), polylines
are axis-aligned and the scale is 1/2, 1, 2 or 4, so the float32 primitives and the float32 coverage arithmetic are exact and the
reference's 1e-3 band is empty: images are compared bit for bit."""
import numpy as np

from continiousenvironment_follower_leader_amd import abi, make_config
from fuzz_configs import draw_config
from golden_util import config_for, load_episode, load_fuzz, scenario_arrays

EPISODES = {"B": "B_s1_chase", "D": "D_s2_chase", "F": "F_s1_chase", "L": "L_s2_chase", "T": "T_s3_chase"}
TILE, CHUNK, STAGE = 32, 512, 256          # ftl_render_tile_kernel: tile edge, primitives per LDS chunk, lanes per staging round
NO_RAYS = abi.RENDER_PATH | abi.RENDER_BOX | abi.RENDER_SENSORS | abi.RENDER_TARGET


# ---- configs -----------------------------------------------------------------------------------------------------------------------
def golden_config(name, **over):
    """(cfg, scenario arrays, record) of golden episode ``EPISODES[name]`` with config overrides."""
    z, meta = load_episode(EPISODES[name])
    cfg = config_for(meta, scen_route_len=over.pop("scen_route_len", len(z["scen:route"])), **over)
    return cfg, scenario_arrays(z), z


def tracker_only_config(**over):
    """Config B with the v2 tracker as its only sensor (no ray primitives between the list's sections), small green discs and a small
    ring so that a whole list fits around one tile, and room for 256 corridor points and 2048 way-points."""
    z, meta = load_episode(EPISODES["B"])
    trk = meta["kwargs"]["follower_sensors"]["LeaderPositionsTracker_v2"]
    kw = dict(follower_sensors={"LeaderPositionsTracker_v2": trk}, corr_cap=256, max_dev=0.12, min_distance=0.24)      # 6 px and 12 px
    kw.update(over)
    cfg = config_for(meta, scen_route_len=kw.pop("scen_route_len", 2048), **kw)
    return cfg, scenario_arrays(z), z


def fuzz_config(seed):
    """(cfg, scenario arrays) of ``fuzz_configs.draw_config(seed)`` with the world its record was played on."""
    z, _ = load_fuzz(seed)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = make_config(**dict(draw_config(seed), route_cap=max(128, len(z["scen:route"]))))
    return cfg, scenario_arrays(z)


def sensor_properties(cfg):
    """Per ray sensor of ``cfg``: dict(kind 'compas' / 'explicit' / 'lenient' / 'prev', count, history, pad, after)."""
    out = []
    for k in range(cfg.c.n_lasers):
        l = cfg.c.lasers[k]
        kind = "compas" if l.compas else ("explicit" if l.explicit_angles else ("lenient" if l.lenient else "prev"))
        out.append(dict(kind=kind, count=int(l.count), history=int(l.history), pad=bool(l.pad_sectors), after=bool(l.after_tracker),
                        length=float(l.length), offset=int(l.out_offset),
                        width=int(l.count) * (5 if l.compas else (4 if l.pad_sectors else 1))))
    return out


def list_cap(cfg):
    """The capacity include/ftl.h's workspace gives one env's list: route + 2, trajectory + 1, body + outline per object, per ray sensor a
    line per ray and a disc per ray and row, 3 per corridor point + 2, the target ring."""
    c = cfg.c
    rays = sum(c.lasers[k].count * (1 + c.lasers[k].history) for k in range(c.n_lasers))
    return (c.route_cap + 2) + (c.traj_cap + 1) + 2 * (cfg.n_robots + c.n_static) + rays + 3 * c.corr_cap + 2 + 1


# ---- one env's words ------------------------------------------------------------------------------------------------------------------
class Spec:
    def __init__(self, cfg, scen):
        c, R = cfg.c, cfg.n_robots
        self.cfg = cfg
        self.pos = np.asarray(scen["robot_pos"], np.float32).reshape(R, 2).copy()
        self.dir = np.asarray(scen["robot_dir"], np.float64).reshape(R).copy()
        self.rect = np.asarray(scen["robot_rect"], np.int32).reshape(R, 4).copy()
        self.static = np.asarray(scen["static_rects"], np.int32).reshape(-1, 4)[:c.n_static].copy()
        self.start = self.pos.copy()                                   # the pool entry's robot_pos
        self.route = np.zeros((c.route_cap, 2), np.float64)
        r = np.asarray(scen["route"], np.float64).reshape(-1, 2)[:c.route_cap]
        self.route[:len(r)] = r
        self.route_len = len(r)
        self.traj = np.zeros((c.traj_cap, 2), np.float32)
        self.hist = np.zeros((c.corr_cap, 2), np.float64)
        self.corr = np.zeros((c.corr_cap, 2, 2), np.float64)
        self.words = {abi.EI_GREEN_LEN: 0, abi.EI_GREEN_COUNT: 0, abi.EI_CORR_LO: 0, abi.EI_CORR_HI: 0, abi.EI_TOO_CLOSE: 0,
                      abi.EI_TARGET_ID: 0}
        self.scen = None                                               # EI_SCEN (None: the env's own pool entry)
        self.lasers = np.zeros(cfg.lasers_len, np.float32)

    # -- helpers
    def set_route(self, pts, route_len=None, target=0):
        pts = np.asarray(pts, np.float64).reshape(-1, 2)
        self.route[:] = 0.0
        self.route[:len(pts)] = pts
        self.route_len = len(pts) if route_len is None else int(route_len)
        self.words[abi.EI_TARGET_ID] = int(target)
        return self

    def set_corridor(self, hist, right, left, lo=0, hi=None):
        """Window [lo, hi) of the ring buffers: point i of ``hist`` / ``right`` / ``left`` goes to slot (lo + i) & (corr_cap - 1)."""
        hist = np.asarray(hist, np.float64).reshape(-1, 2)
        n, m = len(hist), self.cfg.c.corr_cap - 1
        q = (lo + np.arange(n)) & m
        self.hist[q] = hist
        self.corr[q, 0] = np.asarray(right, np.float64).reshape(-1, 2)
        self.corr[q, 1] = np.asarray(left, np.float64).reshape(-1, 2)
        self.words[abi.EI_CORR_LO], self.words[abi.EI_CORR_HI] = int(lo), int(lo + n if hi is None else hi)
        return self

    def set_green(self, pts, green_len=None, green_count=None):
        """Trajectory points [0, len(pts)); by default the green zone is all of them but the first: green_len = len + 1."""
        pts = np.asarray(pts, np.float32).reshape(-1, 2)
        self.traj[:len(pts)] = pts
        self.words[abi.EI_GREEN_LEN] = len(pts) + 1 if green_len is None else int(green_len)
        self.words[abi.EI_GREEN_COUNT] = (len(pts) - 1 if green_count is None else int(green_count))
        return self

    def set_robot(self, r, x, y, direction=0.0, rect=None):
        self.pos[r] = (x, y)
        self.dir[r] = direction
        if rect is not None:
            self.rect[r] = rect
        return self

    def set_static(self, rects):
        """The first len(rects) static rects; the others are parked far outside every test window."""
        rects = np.asarray(rects, np.int32).reshape(-1, 4)
        self.static[:] = (-100000, -100000, 1, 1)
        self.static[:len(rects)] = rects
        return self

    def park(self):
        """Everything far outside every test window (integers: exact), no route, no green zone, no corridor."""
        for r in range(self.cfg.n_robots):
            self.set_robot(r, -50000.0, -50000.0 - 1000.0 * r, 0.0, (-50010, -50010 - 1000 * r, 20, 20))
        self.start = self.pos.copy()
        self.set_static([])
        self.set_route(np.zeros((0, 2)))
        self.words.update({abi.EI_GREEN_LEN: 0, abi.EI_GREEN_COUNT: 0, abi.EI_CORR_LO: 0, abi.EI_CORR_HI: 0})
        return self

    def scene(self, e=0, n_pool=None):
        """The dict of ``render_numpy.env_scene`` from the host arrays."""
        cfg, R = self.cfg, self.cfg.n_robots
        ei = np.zeros(abi.EI_COUNT, np.int32)
        for k, v in self.words.items():
            ei[k] = v
        s = e if self.scen is None else self.scen
        ei[abi.EI_SCEN] = s
        rd = np.zeros((R, abi.RD_COUNT), np.float64)
        rd[:, abi.RD_DIRECTION] = self.dir
        ri = np.zeros((R, abi.RI_COUNT), np.int32)
        ri[:, :4] = self.rect
        pool = dict(route=self.route, route_len=np.int32(self.route_len), static_rects=self.static, robot_pos=self.start)
        if self.scen is not None and not (n_pool is not None and 0 <= s < n_pool):
            pool = None
        return dict(env_int=ei, rb_pos=self.pos, rb_dbl=rd, rb_int=ri, traj=self.traj, hist=self.hist, corr=self.corr,
                    lasers=self.lasers, pool=pool)


# ---- device side --------------------------------------------------------------------------------------------------------------------
def make_batch(cfg, scen, n):
    """A reset VecGame of ``n`` <= 8 envs, env e on its own pool entry e (n copies of one world, so a test may write into each)."""
    import torch
    from continiousenvironment_follower_leader_amd.vec_game import ScenarioPool, VecGame
    assert 1 <= n <= 8
    env = VecGame(n, device="cuda:0", config=cfg)
    rep = lambda a: np.repeat(np.asarray(a)[None], n, 0)
    env.load_scenarios(ScenarioPool(cfg, rep(scen["static_rects"]), rep(scen["robot_pos"]), rep(scen["robot_dir"]), rep(scen["robot_rect"]),
                                    [scen["route"][:cfg.c.route_cap]] * n, [scen["init_traj"]] * n, "cuda:0"))
    env.reset(torch.arange(n, dtype=torch.int32))
    torch.cuda.synchronize()
    return env


def apply(env, e, spec):
    """Write ``spec`` into env ``e`` and pool entry ``e`` of a batch of ``make_batch``."""
    import torch
    cfg, R = env.cfg, env.cfg.n_robots
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    ei = env.state_field("env_int")
    for k, v in spec.words.items():
        ei[e, k] = int(v)
    ei[e, abi.EI_SCEN] = e if spec.scen is None else int(spec.scen)
    env.state_field("rb_pos")[e] = dev(spec.pos.reshape(-1))
    env.state_field("rb_dbl")[e].view(R, abi.RD_COUNT)[:, abi.RD_DIRECTION] = dev(spec.dir)
    env.state_field("rb_int")[e].view(R, abi.RI_COUNT)[:, :4] = dev(spec.rect)
    env.state_field("traj")[e] = dev(spec.traj.reshape(-1))
    env.state_field("hist")[e] = dev(spec.hist.reshape(-1))
    env.state_field("corr")[e] = dev(spec.corr.reshape(-1))
    t = env.pool.t
    t["route"][e] = dev(spec.route)
    t["route_len"][e] = int(spec.route_len)
    if cfg.c.n_static > 0:
        t["static_rects"][e] = dev(spec.static)
    t["robot_pos"][e] = dev(spec.start)
    if spec.lasers.size:
        env.lasers[e, :spec.lasers.size] = dev(spec.lasers)
    torch.cuda.synchronize()


def read_counts(env, k):
    """(counts int32[k], cap) of the last ``render`` of ``k`` envs: the list lengths the list kernel left in the workspace, and the
    per-env capacity derived from the workspace size ``ftl_render_workspace(k)`` = align_up(4 k, 256) + 32 k cap."""
    import torch
    torch.cuda.synchronize()
    kk, buf = env._render_ws
    assert kk == k
    head = (4 * k + 255) // 256 * 256
    cap, rem = divmod(buf.numel() - head, 32 * k)
    assert rem == 0
    return buf[:4 * k].view(torch.int32).cpu().numpy().copy(), cap


# ---- geometry helpers -----------------------------------------------------------------------------------------------------------------
def tile_box(tx, ty, width, height):
    """Pixel-centre extent [x0, x1] x [y0, y1] of tile (tx, ty) of a width x height image."""
    return (tx * TILE + 0.5, ty * TILE + 0.5, min((tx + 1) * TILE, width) - 0.5, min((ty + 1) * TILE, height) - 0.5)


def boxes_meet(*boxes):
    """True when the common intersection of (x0, y0, x1, y1) boxes is not empty."""
    return max(b[0] for b in boxes) <= min(b[2] for b in boxes) and max(b[1] for b in boxes) <= min(b[3] for b in boxes)


# ---- chunk scenes (group B) -----------------------------------------------------------------------------------------------------------
# Everything of a chunk scene lies around tile (1, 1) = pixels [32, 64) x [32, 64) of a 96 x 96 image at scale 1.  List order without
# OBJECTS: A route segments (A = route_len - 1 when route_len > 2) | bridge disc | finish disc | gc green discs | ring | cnt history discs |
# 2 (cnt - 1) + 2 corridor segments | target ring; n = [A + 2] + [gc + 1] + [3 cnt] + [1] over the chosen layers.
CHUNK_W = CHUNK_H = 96
CHUNK_TILE = (1, 1)
GREEN_COLS, HIST_COLS = 24, 15
FINISH = (37.25, 34.25)


def chunk_spec(cfg, scen, A, gc, cnt):
    """The chunk scene with A route segments, gc green discs (r 6) and a corridor window of cnt points.
    The route zigzags in from the right along the top of the tile to the finish point (37.25, 34.25), where the target ring is too; the
    bridge disc sits at (42, 32) on its last segment.  Green disc i (list order) is centred at (27.5 + i % 24, 44.5 + i // 24): the pixel
    on top of it stays visible under the later ones.  The ring (r 12) is centred at (44.5, 50.5).  History disc i is at
    (52.5 + i % 15, 40.5 + i // 15); the corridor's right border starts beside the last one and runs right in steps of 1/8 px, its left
    border ends beside the finish point, so the last cap crosses the tile."""
    c = cfg.c
    sp = Spec(cfg, scen).park()
    assert A == 0 or 2 <= A < c.route_cap
    assert gc == 0 or 5 < gc <= min(c.traj_cap - 1, GREEN_COLS * 26)
    assert 0 <= cnt <= min(c.corr_cap, HIST_COLS * 27)
    m = A + 1 if A else 2                                       # way-points (two when A == 0: no polyline, but a finish disc)
    k = m - 1 - np.arange(m)                                    # steps before the finish point
    sp.set_route(np.stack([FINISH[0] + k * min(3.0, 56.0 / m), FINISH[1] - 9.0 * (k % 2)], 1), target=m - 1)
    sp.set_static([(36, 28, 8, 8), (42, 30, 4, 4)])             # centres (40, 32) and (44, 32): bridge point (42, 32)
    if gc:
        i = np.arange(gc)
        traj = np.zeros((gc + 1, 2), np.float32)
        traj[gc - i] = np.stack([27.5 + i % GREEN_COLS, 44.5 + i // GREEN_COLS], 1)   # list position i is point green_len - 2 - i = gc - i
        sp.set_green(traj, green_len=gc + 2, green_count=gc)
    sp.set_robot(0, 44.5, 50.5)
    if cnt:
        i = np.arange(cnt)
        hist = np.stack([52.5 + i % HIST_COLS, 40.5 + i // HIST_COLS], 1)
        right = np.stack([hist[-1, 0] + 1.0 + i / 8.0, np.full(cnt, hist[-1, 1] - 1.0)], 1)
        left = np.stack([FINISH[0] + 5.0 - (cnt - 1 - i) / 8.0, np.full(cnt, FINISH[1] + 3.0)], 1)
        sp.set_corridor(hist, right, left, lo=c.corr_cap - 3)   # (the window wraps round the ring buffer)
    return sp


def chunk_length(layers, A, gc, cnt):
    n = 0
    if layers & abi.RENDER_PATH: n += A + 2
    if layers & abi.RENDER_BOX: n += gc + 1
    if layers & abi.RENDER_SENSORS: n += 3 * cnt
    if layers & abi.RENDER_TARGET: n += 1
    return n


def chunk_edges(n):
    """List positions p >= 1 whose pair (p - 1 | p) straddles the chunk edge n - 512 or the staging edge n - 256 of the last chunk."""
    return [n - q for q in (CHUNK, STAGE) if n - q >= 1]


def chunk_pair_problems(prims, width, height, tile, render_prims, prim_bbox):
    """Why the list fails the precondition of a chunk test (empty: it holds): at every edge position p the primitives p - 1 and p have
    different colours, their boxes and the tile have a common point, and leaving either out changes the reference image inside the
    tile.  Also: more than 256 primitives of the last chunk meet the tile."""
    n = len(prims)
    tb = tile_box(tile[0], tile[1], width, height)
    ys, xs = slice(tile[1] * TILE, (tile[1] + 1) * TILE), slice(tile[0] * TILE, (tile[0] + 1) * TILE)
    full = render_prims(prims, width, height)[0][ys, xs]
    bad = []
    for p in chunk_edges(n):
        a, b = prims[p - 1], prims[p]
        if a["rgb"] == b["rgb"]:
            bad.append((p, "same colour", a["section"], b["section"]))
        if not boxes_meet(prim_bbox(a), prim_bbox(b), tb):
            bad.append((p, "no common point in the tile", a["section"], b["section"]))
        for q in (p - 1, p):
            if np.array_equal(render_prims(prims[:q] + prims[q + 1:], width, height)[0][ys, xs], full):
                bad.append((p, "primitive %d (%s) is invisible in the tile" % (q, prims[q]["section"])))
    if n > STAGE and sum(boxes_meet(prim_bbox(q), tb) for q in prims[max(n - CHUNK, 0):]) <= STAGE:
        bad.append("at most 256 primitives of the last chunk meet the tile")
    return bad


# n -> (layers, A, gc, cnt): solutions of chunk_length(...) = n with colour changes at the edge positions, found by search
_ALL4 = NO_RAYS
CHUNK_CASES = {1: (abi.RENDER_TARGET, 0, 0, 0), 2: (abi.RENDER_BOX | abi.RENDER_TARGET, 0, 0, 0),
               255: (_ALL4, 251, 0, 0), 256: (_ALL4, 252, 0, 0), 257: (_ALL4, 0, 253, 0), 511: (_ALL4, 254, 253, 0), 512: (_ALL4, 255, 253, 0),
               513: (_ALL4, 0, 254, 85), 768: (_ALL4, 255, 254, 85), 1023: (_ALL4, 510, 254, 85), 1024: (_ALL4, 511, 254, 85),
               1025: (_ALL4, 512, 254, 85), 1537: (_ALL4, 1024, 254, 85)}


# ---- dyadic scenes (groups C and D) ---------------------------------------------------------------------------------------------------
DYADIC_SCALES = (0.5, 1.0, 2.0, 4.0)


def dyadic_spec(cfg, scen, shift=(0, 0), too_close=1):
    """A small scene of every primitive kind around the world's origin, on the 1/4-px lattice (``shift``: whole pixels).  For a config
    without ray sensors (ray directions are not dyadic): ``tracker_only_config``.  Pixel centres lie on the 1/2-px lattice at scale 1,
    so many of them sit exactly on a boundary (route and corridor strokes, disc rims, hitbox outlines): ties that both sides must
    decide by the same <= / < rule."""
    assert cfg.c.n_lasers == 0 and cfg.n_robots == 3 and cfg.c.n_static >= 3
    sx, sy = int(shift[0]), int(shift[1])
    sh = np.array([sx, sy], np.float64)
    sp = Spec(cfg, scen).park()
    sp.set_robot(0, 20.25 + sx, 14.25 + sy, 0.0, (11 + sx, 1 + sy, 19, 26))
    sp.set_robot(1, 6.75 + sx, 8.25 + sy, 0.0, (-2 + sx, -4 + sy, 17, 25))
    sp.set_robot(2, 33.25 + sx, 35.75 + sy, 0.0, (21 + sx, 23 + sy, 25, 25))
    sp.start = sp.pos.copy()
    sp.set_static([(0 + sx, 0 + sy, 1, 1), (28 + sx, 2 + sy, 6, 9), (2 + sx, 30 + sy, 12, 5)])     # (a 1 x 1 outline in the corner pixel)
    sp.set_route(np.array([(3, 3), (3, 20), (18, 20), (18, 34), (35, 34)], np.float64) + sh, target=2)
    k = np.arange(8)
    sp.set_green(np.stack([24.5 + 2 * k, np.full(8, 30.25)], 1) + sh)                                # 7 green discs
    t = np.arange(4)
    sp.set_corridor(np.stack([5.0 + 4 * t, np.full(4, 25.0)], 1) + sh, np.stack([5.0 + 4 * t, np.full(4, 28.0)], 1) + sh,
                    np.stack([5.0 + 4 * t, np.full(4, 22.0)], 1) + sh, lo=cfg.c.corr_cap - 2)
    sp.words[abi.EI_TOO_CLOSE] = int(too_close)
    return sp


# ---- ray sensors (group E) ------------------------------------------------------------------------------------------------------------
def laser_ramp(cfg, phase=0.0):
    """A ``lasers`` row in which every (sensor, row, ray) that the spec draws has its own reading in (0.12, 0.92) x laser_length, and
    every other column (the padding of pad_sectors sensors, compas blocks) holds 0.05 x laser_length: a disc drawn from one of those
    would sit next to the follower.  ``phase`` shifts every ray's ladder.  Returns (row, [(offset of the reading, sensor index)] of the readings that are drawn)."""
    row = np.zeros(cfg.lasers_len, np.float32)
    used = []
    for k, p in enumerate(sensor_properties(cfg)):
        N, H, W = p["count"], p["history"], p["width"]
        blk = np.full((H, W), 0.05 * p["length"], np.float32)
        if p["kind"] != "compas":
            rows = [H - 1] if p["kind"] in ("explicit", "lenient") else list(range(H))
            for a, j in enumerate(rows):
                for i in range(N):
                    col = i
                    if p["pad"]:
                        col = min(int(i // (N / 4)), 3) * N + i
                    # along a ray the rows' discs are 0.8 L / rows apart; every ray shifts the ladder by its own fraction of a rung
                    blk[j, col] = p["length"] * (0.12 + 0.8 * (a + 0.6 * ((i * 0.37 + k * 0.11 + phase) % 1.0)) / len(rows))
                    used.append((p["offset"] + j * W + col, k))
        row[p["offset"]:p["offset"] + H * W] = blk.reshape(-1)
    return row, used
