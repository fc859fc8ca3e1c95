"""An independent yardstick for the scenario generators' route planner (csrc/ftl_scenario.cpp plan_route, csrc/ftl_scenario_dev.hpp
plan_route_wave): numpy and the standard library only, nothing of the package.

Two parts.  `inflated_grid` rebuilds the planner's obstacle grid from a generated scenario's static_rects and the ftl_scen_params
(generate_trajectory_dstar, ENV:1499-1508: every wall / rock blocks the cells [pm - half, pm + half) per axis around its centre cell, half =
floor(side / 2 / step_grid) + floor(leader_margin * max(leader_w, leader_h) / step_grid), clipped to the grid).  `dijkstra_cost` is a plain
heapq Dijkstra in float64 over the 8-connected free cells, moves cost 1.0 or sqrt(2.0).

The goal cell is not among a generator's outputs, and the check needs none: a route is the parent chain from the leader's cell up to, but
excluding, the goal cell, and every prefix of a shortest path is a shortest path itself.  So for a found route r
    r[0] is the leader's cell, consecutive cells are 8-neighbours, no cell is blocked          (check_route_cells)
    cost(r) == dijkstra_cost(r[0], r[-1]) within COST_TOL                                       (check_route_optimal)
A planner that takes a detour fails the second, one that cuts a corner through a blocked cell the first.

COST_TOL = 1e-9 is derived, not measured: both sides add at most ~400 terms of 1 and sqrt 2, in different orders; every partial sum is
below 1024, so each addition rounds by at most 2^-43 (half an ulp of a double below 1024), and 2 x 400 x 2^-43 = 9.1e-11.  Two different
sums a + b sqrt 2 with a, b <= 400 are never that close unless equal (|a + b sqrt 2| >= 1 / (|a| + |b| sqrt 2 + 1) > 1e-3 for integers)."""
import heapq
import math

import numpy as np

COST_TOL = 1e-9
SQ2 = math.sqrt(2.0)


def grid_shape(sp):
    return sp.width // sp.step_grid, sp.height // sp.step_grid


def inflated_grid(static_rects, sp):
    """bool [rows, cols], True = blocked.  Rows of static_rects without an object (w == h == 0: fewer rocks placed than the capacity) block
    nothing.  A rect is (x, y, w, h) with x = int(cx) - (w >> 1): the centre cell is (x + (w >> 1)) // step_grid."""
    sg = sp.step_grid
    rows, cols = grid_shape(sp)
    margin = int(math.floor(sp.leader_margin * max(sp.leader_w, sp.leader_h) / sg))
    blocked = np.zeros((rows, cols), bool)
    for (x, y, w, h) in np.asarray(static_rects).tolist():
        if w == 0 and h == 0:
            continue
        pmx, pmy = (x + (w >> 1)) // sg, (y + (h >> 1)) // sg
        hw, hh = int(math.floor((w / 2.0) / sg)) + margin, int(math.floor((h / 2.0) / sg)) + margin
        blocked[max(pmx - hw, 0):max(pmx + hw, 0), max(pmy - hh, 0):max(pmy + hh, 0)] = True
    return blocked


def dijkstra_cost(blocked, a, b):
    """Cost of a cheapest 8-connected path from cell a to cell b over free cells, or None when there is none (or an end is blocked)."""
    rows, cols = blocked.shape
    W2 = cols + 2
    wall = np.ones((rows + 2, W2), bool)                     # one-cell border: the neighbour loop needs no bounds test
    wall[1:-1, 1:-1] = blocked
    done = wall.reshape(-1).tolist()                        # blocked | closed
    src, dst = (int(a[0]) + 1) * W2 + int(a[1]) + 1, (int(b[0]) + 1) * W2 + int(b[1]) + 1
    if done[src] or done[dst]:
        return None
    dist = [math.inf] * len(done)
    dist[src] = 0.0
    moves = [(-W2 - 1, SQ2), (-W2, 1.0), (-W2 + 1, SQ2), (-1, 1.0), (1, 1.0), (W2 - 1, SQ2), (W2, 1.0), (W2 + 1, SQ2)]
    heap = [(0.0, src)]
    while heap:
        k, u = heapq.heappop(heap)
        if done[u]:
            continue
        if u == dst:
            return k
        done[u] = True
        for off, c in moves:
            v = u + off
            if not done[v] and k + c < dist[v]:
                dist[v] = k + c
                heapq.heappush(heap, (k + c, v))
    return None


def route_cells(route, route_len, sg):
    """The first route_len points of a generated route (pixels, multiples of step_grid) as an int array of cells [n, 2]."""
    r = np.asarray(route[:route_len], np.float64) / sg
    c = np.rint(r).astype(np.int64)
    assert np.array_equal(c, r), "route point off the grid"
    return c


def route_cost(cells):
    """Sum over the moves of a route: 1.0 for a straight move, sqrt(2.0) for a diagonal one (float64, in route order)."""
    d = np.abs(np.diff(cells, axis=0))
    assert (d.max(1) == 1).all(), "not an 8-connected move"
    return math.fsum(SQ2 if (m[0] and m[1]) else 1.0 for m in d.tolist())


def leader_cell(leader_pos, sg):
    """(int)(x / (float)sg) of the float32 leader position, as both generators compute it."""
    p = np.asarray(leader_pos, np.float32) / np.float32(sg)
    return int(p[0]), int(p[1])


def check_route_cells(cells, blocked, leader_pos, sg):
    """The cheap checks: starts in the leader's cell, every move is to one of the 8 neighbours, no cell is blocked or off the grid."""
    assert len(cells) >= 1
    assert tuple(cells[0]) == leader_cell(leader_pos, sg), ("start", tuple(cells[0]), leader_cell(leader_pos, sg))
    if len(cells) > 1:
        d = np.abs(np.diff(cells, axis=0))
        assert d.max() <= 1 and (d.sum(1) > 0).all(), "moves"
    rows, cols = blocked.shape
    assert cells.min() >= 0 and cells[:, 0].max() < rows and cells[:, 1].max() < cols, "off the grid"
    assert not blocked[cells[:, 0], cells[:, 1]].any(), "blocked cell on the route"


def check_route_optimal(cells, blocked):
    """cost(route) equals the Dijkstra cost between its ends within COST_TOL.  Returns (route cost, Dijkstra cost)."""
    got, best = route_cost(cells), dijkstra_cost(blocked, cells[0], cells[-1])
    assert best is not None, "the route's own ends are not connected"
    assert abs(got - best) <= COST_TOL, ("route cost", got, "optimum", best)
    return got, best
