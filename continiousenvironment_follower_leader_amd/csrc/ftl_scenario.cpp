// ftl_generate_scenarios -- the scenario part of the reference's Game.reset(), host side.
//
// The `random`-driven sequential program (robots, walls, rocks, finish points; then the leader's direction, the follower's second draw, the
// outputs) is ftl_scenario_core.hpp, shared with the device generator and instantiated here with HostPolicy: glibc's atan / cos / sin as the
// reference calls them through CPython, and no cap on the rejection samplers.  This file keeps the planners between its two halves,
//   generate_trajectory_dstar     ENV:1493-1612   utils/dstar.py:84-210 -- a first D* run is Dijkstra from the goal
//   generate_trajectory_astar     ENV:1632-1711   utils/astar.py:50-166
// and the thread pool.
// Not reproducible: which of several equal-cost routes dstar.py returns (min() over a set of objects hashed by id).
//
// FTL_SCEN_DEVICE_POLICY (diagnostic build only, tests/host/scenario_policy_main.cpp): the shared program with the DEVICE's policy --
// ftl_crmath.hpp and the cap of FTL_SG_MAX_ATTEMPTS draws -- around the planners of this file, so that what lane 0 of the device generator
// computes can be compared with the product on a CPU.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "ftl_scenario_core.hpp"

namespace {

using namespace ftl_sc;
#ifdef FTL_SCEN_DEVICE_POLICY
using Policy = DevicePolicy;
#else
using Policy = HostPolicy;
#endif


// ---- utils/dstar.py: the first run() on a fresh map is Dijkstra from the goal; the route is the parent chain from start.
// Costs accumulate exactly as there (h_new = x.h + cost, cost = 1.0 or sqrt(2.0) as a double).  Returns false when the walk
// along the parents cannot reach the goal the way the reference's cannot (goal inside an inflated obstacle).
struct Grid {
    int rows, cols;
    std::vector<uint8_t> obst;
    bool in(int x, int y) const { return x >= 0 && x < rows && y >= 0 && y < cols; }
};

bool plan_route(const Grid& g, int sx, int sy, int gx, int gy, int max_iterat, std::vector<int>& rx, std::vector<int>& ry) {
    rx.clear(); ry.clear();
    if (!g.in(sx, sy) || !g.in(gx, gy)) return false;
    if (sx == gx && sy == gy) return true;                   // `while tmp != end` never runs: empty route
    // An obstacle goal or start makes every first move cost sys.maxsize: the reference then wanders through modify()
    // until max_iterat and reports found_target_point = False (pinned against the seeds the golden pool dropped).
    if (g.obst[(size_t)gx * g.cols + gy] || g.obst[(size_t)sx * g.cols + sy]) return false;
    // The open list in the reference's order -- smallest key first, insertion order among equal keys -- without a heap: every move
    // costs at least 1, so a state popped with key k only inserts keys >= k + 1, i.e. into LATER unit-wide buckets than its own.  When
    // bucket i comes up it is therefore complete; a stable sort by key (insertion order = sequence order already) puts it into pop
    // order.  Same pops, same relaxations, same parents as the binary heap this replaces, at a third of the time (the planner is
    // nine tenths of a scenario).  The grid carries a one-cell border of blocked cells, so the neighbour loop needs no bounds test.
    const int W2 = g.cols + 2, N2 = (g.rows + 2) * W2;
    const double INF = 1e300;
    struct Item { double k; int id; };
    static thread_local std::vector<double> h;               // per-thread scratch (thousands of scenarios per thread)
    static thread_local std::vector<int> parent;
    static thread_local std::vector<uint8_t> blocked;        // obstacle | closed | border
    static thread_local std::vector<std::vector<Item>> bucket;
    h.assign((size_t)N2, INF); parent.assign((size_t)N2, -1); blocked.assign((size_t)N2, 1);
    for (int x = 0; x < g.rows; x++) {
        const uint8_t* src = &g.obst[(size_t)x * g.cols];
        uint8_t* dst = &blocked[(size_t)(x + 1) * W2 + 1];
        for (int y = 0; y < g.cols; y++) dst[y] = src[y];
    }
    // Keys have no useful bound: around a dense field of rocks a shortest route is far longer than rows + cols moves (100 rocks on
    // 150 x 100 cells: costs up to 370 on 0.5 % of the seeds), so the bucket array grows with the keys.  Bucket bi only ever pushes into
    // buckets <= bi + 2 (key < bi + 1, move <= sqrt 2): the array is sized BEFORE the reference to bucket bi is taken and no push can
    // move it.  `dirty` = buckets written by the previous call of this thread -- the only ones that need clearing.
    static thread_local int dirty = 0;
    for (int i = 0; i < dirty; i++) bucket[(size_t)i].clear();
    if (bucket.size() < 3) bucket.resize(3);
    int top = 0;                                             // the last bucket that holds an entry (a local: the loop below is hot)
    const int goal = (gx + 1) * W2 + gy + 1, start = (sx + 1) * W2 + sy + 1;
    const double SQ2 = sqrt(2.0);
    // neighbour order of Map.get_neighbors (dstar.py:62-74): i = -1..1 outer, j = -1..1 inner
    const int doff[8] = {-W2 - 1, -W2, -W2 + 1, -1, 1, W2 - 1, W2, W2 + 1};
    const double dcost[8] = {SQ2, 1.0, SQ2, 1.0, 1.0, SQ2, 1.0, SQ2};
    h[(size_t)goal] = 0.0;
    bucket[0].push_back(Item{0.0, goal});
    bool reached = false;
    for (int bi = 0; bi <= top && !reached; bi++) {
        if (bucket.size() < (size_t)bi + 3) bucket.resize(std::max((size_t)bi + 3, 2 * bucket.size()));
        std::vector<Item>& B = bucket[(size_t)bi];
        if (B.empty()) continue;
        std::stable_sort(B.begin(), B.end(), [](const Item& a, const Item& b) { return a.k < b.k; });
        for (size_t t = 0; t < B.size(); t++) {
            const Item it = B[t];
            if (blocked[(size_t)it.id] || it.k != h[(size_t)it.id]) continue;      // closed meanwhile / superseded entry
            blocked[(size_t)it.id] = 1;
            if (it.id == start) { reached = true; break; }
            for (int d = 0; d < 8; d++) {
                const int nid = it.id + doff[d];
                if (blocked[(size_t)nid]) continue;
                const double hn = it.k + dcost[d];
                if (hn < h[(size_t)nid]) {
                    h[(size_t)nid] = hn; parent[(size_t)nid] = it.id;
                    const int to = (int)hn;                  // bi + 1 or bi + 2
                    top = to > top ? to : top;
                    bucket[(size_t)to].push_back(Item{hn, nid});
                }
            }
        }
    }
    dirty = top + 1;
    if (!reached) return false;                               // unreachable goal: the reference would never return
    int cur = start, iter = 0;
    while (cur != goal) {
        if (++iter > max_iterat) return false;
        rx.push_back(cur / W2 - 1); ry.push_back(cur % W2 - 1);
        cur = parent[(size_t)cur];
        if (cur < 0) return false;
    }
    return true;
}

// ---- utils/astar.py:50-166, literally: nodes ordered by f = g + h with h = SQUARED distance to the goal, CPython heapq (ties keep the
// heap's own order), a closed LIST, duplicates in the open list unless an open node at the same cell has a smaller g, and a cap of
// 1000 expansions after which the path to the LAST expanded node is returned (return_none_on_max_iter=False, ENV:1681-1695).
// Returns false when the open list runs dry (the reference returns None).  Path cells are appended to px / py in grid units.
struct ANode { int x, y, g, f, parent; };
bool astar_route(const std::vector<uint8_t>& maze, int gw, int gh, int sx, int sy, int ex, int ey, int max_iterations,
                 std::vector<int>& px, std::vector<int>& py) {
    std::vector<ANode> nodes;                       // every node ever created (parent = index)
    std::vector<int> heap;                          // open_list as CPython's heapq keeps it (indices into nodes)
    std::vector<int> closed;                        // closed_list (indices), membership by position
    std::vector<uint8_t> in_closed((size_t)gw * gh, 0);
    auto lt = [&](int a, int b) { return nodes[(size_t)a].f < nodes[(size_t)b].f; };
    auto siftdown = [&](int startpos, int pos) {
        const int item = heap[(size_t)pos];
        while (pos > startpos) {
            const int pp = (pos - 1) >> 1;
            if (lt(item, heap[(size_t)pp])) { heap[(size_t)pos] = heap[(size_t)pp]; pos = pp; continue; }
            break;
        }
        heap[(size_t)pos] = item;
    };
    auto siftup = [&](int pos) {
        const int endpos = (int)heap.size(), startpos = pos, item = heap[(size_t)pos];
        int child = 2 * pos + 1;
        while (child < endpos) {
            const int right = child + 1;
            if (right < endpos && !lt(heap[(size_t)child], heap[(size_t)right])) child = right;
            heap[(size_t)pos] = heap[(size_t)child]; pos = child; child = 2 * pos + 1;
        }
        heap[(size_t)pos] = item;
        siftdown(startpos, pos);
    };
    auto push = [&](int n) { heap.push_back(n); siftdown(0, (int)heap.size() - 1); };
    auto pop = [&]() { const int last = heap.back(); heap.pop_back(); if (heap.empty()) return last; const int ret = heap[0]; heap[0] = last; siftup(0); return ret; };
    auto emit = [&](int n) {                       // return_path: goal-to-start chain, reversed
        std::vector<int> chain;
        for (int c = n; c >= 0; c = nodes[(size_t)c].parent) chain.push_back(c);
        for (size_t i = chain.size(); i-- > 0;) { px.push_back(nodes[(size_t)chain[i]].x); py.push_back(nodes[(size_t)chain[i]].y); }
    };
    nodes.push_back(ANode{sx, sy, 0, 0, -1});
    push(0);
    static const int dx8[8] = {0, 0, -1, 1, -1, -1, 1, 1}, dy8[8] = {-1, 1, 0, 0, -1, 1, -1, 1};
    int outer = 0, current = -1;
    while (!heap.empty()) {
        outer++;
        if (outer > max_iterations) { emit(current); return true; }       // "giving up on pathfinding too many iterations"
        current = pop();
        closed.push_back(current);
        const ANode cur = nodes[(size_t)current];
        if (cur.x >= 0 && cur.x < gw && cur.y >= 0 && cur.y < gh) in_closed[(size_t)cur.x * gh + cur.y] = 1;
        if (cur.x == ex && cur.y == ey) { emit(current); return true; }
        for (int d = 0; d < 8; d++) {
            const int nx = cur.x + dx8[d], ny = cur.y + dy8[d];
            if (nx > gw - 1 || nx < 0 || ny > gh - 1 || ny < 0) continue;
            if (maze[(size_t)nx * gh + ny] != 0) continue;
            if (in_closed[(size_t)nx * gh + ny]) continue;                  // child is on the closed list
            const int g = cur.g + 1, h = (nx - ex) * (nx - ex) + (ny - ey) * (ny - ey);
            bool worse = false;                                          // an open node at this cell with a smaller g
            for (int o : heap) if (nodes[(size_t)o].x == nx && nodes[(size_t)o].y == ny && g > nodes[(size_t)o].g) { worse = true; break; }
            if (worse) continue;
            nodes.push_back(ANode{nx, ny, g, g + h, current});
            push((int)nodes.size() - 1);
        }
    }
    return false;                                                        // "Couldn't get a path to destination"
}

void generate_one(const Params& p, int64_t seed, int idx, const ftl_scenarios& out, uint8_t* status) {
    const ftl_scen_params& sp = p.sp;
    uint32_t mt[624];
    std::vector<Obj> objs((size_t)p.n_static);           // statics only, in game_object_list order
    Start S;
    before_planner<Policy>(p, seed, mt, objs.data(), S);
    objs.resize((size_t)S.nobjs);
    const bool ok = S.ok && !S.limit;
    const int W = sp.width, H = sp.height, sg = sp.step_grid;
    const float lpx = S.lpx, lpy = S.lpy;
    std::vector<double> route_x, route_y;
    bool found = true;
    if (ok && sp.planner == 2)
        for (int i = 0; i < sp.fixed_route_len; i++) { route_x.push_back(sp.fixed_route[2 * i]); route_y.push_back(sp.fixed_route[2 * i + 1]); }
    if (ok && sp.planner == 1) {
        // ---- generate_trajectory_astar (ENV:1632-1711): a 20 px grid, obstacles inflated by 2 x the leader's larger side, the bridge row
        // cleared, one leg to the near end of the bridge and one from its far end to the finish point
        const int a_sg = 20;
        const int sx = (int)(lpx / (float)a_sg), sy = (int)(lpy / (float)a_sg);
        const int ex = (int)((double)S.fx[0] / a_sg), ey = (int)((double)S.fy[0] / a_sg);
        const int gw = (int)((double)W / a_sg), gh = (int)((double)H / a_sg);
        std::vector<uint8_t> maze((size_t)gw * gh, 0);
        const int lsf = (int)(fmax(sp.leader_w, sp.leader_h) * 2);
        for (const Obj& o : objs) {
            const int x0 = std::max((int)((double)(o.r.x - lsf) / a_sg), 0), x1 = std::min((int)((double)(o.r.right() + lsf) / a_sg), gw - 1);
            const int y0 = std::max((int)((double)(o.r.y - lsf) / a_sg), 0), y1 = std::min((int)((double)(o.r.bottom() + lsf) / a_sg), gh - 1);
            for (int x = x0; x < x1; x++) for (int y = y0; y < y1; y++) maze[(size_t)x * gh + y] = 1;
        }
        std::vector<int> px, py;
        bool got = true;
        if (sp.add_obstacles && objs.size() >= 2) {
            const Obj& w1 = objs[0]; const Obj& w2 = objs[1];
            // self.bridge_point: float32 mean of the two wall centres (ENV:636-637), / 20 in float32, truncated
            const float bpx = (float)(((double)w1.px + (double)w2.px) / 2), bpy = (float)(((double)w1.py + (double)w2.py) / 2);
            const int bx = (int)(bpx / (float)a_sg), by = (int)(bpy / (float)a_sg);
            auto clear = [&](int x, int y) {              // numpy indexing: a negative index wraps around
                if (x < 0) x += gw; if (y < 0) y += gh;
                if (x >= 0 && x < gw && y >= 0 && y < gh) maze[(size_t)x * gh + y] = 0;
            };
            clear(bx, by);
            for (int i = (int)(((double)w1.r.x / a_sg) - ((double)lsf / a_sg)); i < (int)(((double)w1.r.right() / a_sg) + ((double)lsf / a_sg)); i++) clear(i, by);
            const int fbx = (int)(((double)w1.r.right() + sp.leader_pos_epsilon) / a_sg), sbx = (int)(((double)w1.r.x - sp.leader_pos_epsilon) / a_sg);
            got = astar_route(maze, gw, gh, sx, sy, fbx, by, 1000, px, py);
            if (got) {
                for (size_t i = 0; i < px.size(); i++) { route_x.push_back((long)px[i] * a_sg); route_y.push_back((long)py[i] * a_sg); }
                // `if path[-1] != first_bridge_point` compares a pixel pair with a grid pair (ENV:1684): they only coincide at the origin
                if (!(route_x.back() == fbx && route_y.back() == by)) { route_x.push_back((long)((double)w1.r.right() + sp.leader_pos_epsilon)); route_y.push_back((long)a_sg * by); }
                px.clear(); py.clear();
                if (astar_route(maze, gw, gh, sbx, by, ex, ey, 1000, px, py))
                    for (size_t i = 0; i < px.size(); i++) { route_x.push_back((long)px[i] * a_sg); route_y.push_back((long)py[i] * a_sg); }
            }
        } else {
            got = astar_route(maze, gw, gh, sx, sy, ex, ey, 1000, px, py);
            if (got) for (size_t i = 0; i < px.size(); i++) { route_x.push_back((long)px[i] * a_sg); route_y.push_back((long)py[i] * a_sg); }
        }
        found = route_x.size() >= 2;                  // the reference leaves found_target_point False (ENV:1537 is D*-only): "usable" = it can be stepped
    }
    // ---- generate_trajectory_dstar (ENV:1493-1612)
    if (ok && sp.planner == 0) {
        Grid g; g.rows = W / sg; g.cols = H / sg; g.obst.assign((size_t)g.rows * g.cols, 0);
        const int margin = (int)floor(sp.leader_margin * fmax(sp.leader_w, sp.leader_h) / sg);
        // order of the reference: rocks, then the two walls (irrelevant for a set of cells)
        for (const Obj& o : objs) {
            const int pmx = (int)floorf(o.px / (float)sg), pmy = (int)floorf(o.py / (float)sg);
            const int hh = (int)floor((o.h / 2.0) / sg) + margin, hw = (int)floor((o.w / 2.0) / sg) + margin;
            for (int i = pmx - hw; i < pmx + hw; i++)
                for (int j = pmy - hh; j < pmy + hh; j++)
                    if (g.in(i, j)) g.obst[(size_t)i * g.cols + j] = 1;
        }
        std::vector<int> rx, ry;
        int sx = (int)(lpx / (float)sg), sy = (int)(lpy / (float)sg);
        const int runs = sp.multiple_end_points ? 3 : 1;
        for (int k = 0; k < runs; k++) {
            const int gx = (int)((double)S.fx[k] / sg), gy = (int)((double)S.fy[k] / sg);
            // the 2nd and 3rd planner of the reference use the default max_iterat (Dstar(m2), dstar.py:85)
            const bool f = plan_route(g, sx, sy, gx, gy, k == 0 ? sp.path_finding_iterations : 15000, rx, ry);
            found = found && f;
            for (size_t i = 0; i < rx.size(); i++) { route_x.push_back((long)rx[i] * sg); route_y.push_back((long)ry[i] * sg); }
            sx = gx; sy = gy;
        }
    }
    const int rl = (int)route_x.size();
    Linspace traj;
    after_planner<Policy>(p, S, mt, found, rl, rl >= 2 ? route_x[1] : 0.0, rl >= 2 ? route_y[1] : 0.0, out, status, idx, traj);
    // ---- the arrays
    int32_t* srect = const_cast<int32_t*>(out.static_rects) + (size_t)idx * p.n_static * 4;
    for (int s = 0; s < p.n_static; s++) static_rect_row(objs.data(), S.nobjs, srect, s);
    double* ro = const_cast<double*>(out.route) + (size_t)idx * p.route_cap * 2;
    const int rn = rl < p.route_cap ? rl : p.route_cap;
    for (int i = 0; i < rn; i++) { ro[2 * i] = route_x[(size_t)i]; ro[2 * i + 1] = route_y[(size_t)i]; }
    for (int i = rn; i < p.route_cap; i++) route_pad(ro, i);
    float* it = const_cast<float*>(out.init_traj) + (size_t)idx * p.init_traj_cap * 2;
    for (int i = 0; i < p.init_traj_cap; i++) traj_point(traj, it, i);
}

}  // namespace

extern "C" int ftl_generate_scenarios(const ftl_config* cfg, const ftl_scen_params* sp, const int64_t* seeds, int32_t n,
                                      int32_t n_threads, const ftl_scenarios* out, uint8_t* status) {
    if (check_args(cfg, sp, n) || !seeds || !out || !status || !has_every_array(*out)) return FTL_E_INVALID;
    const Params p = make_params(*cfg, *sp);
    int T = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    if (T < 1) T = 1;
    if (T > n) T = n > 0 ? n : 1;
    std::atomic<int> next(0);
    auto work = [&]() { for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) generate_one(p, seeds[i], i, *out, status); };
    if (T == 1) work();
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < T; t++) th.emplace_back(work);
        for (auto& t : th) t.join();
    }
    return FTL_OK;
}
