// ftl_scenario_core.hpp -- the sequential program of the scenario generator, once: the `random`-driven part of the reference's Game.reset()
//  as ftl_generate_scenarios (ftl_scenario.cpp, a host thread per scenario) and ftl_generate_scenarios_device
// (ftl_scenario_dev.hpp, lane 0 of a wavefront per scenario) both run it, draw for draw.  Each of the two keeps only its planner and its way
// of spreading the work.
//
// Follows, in the reference's order of `random` draws (so that python seed s reproduces `game.seed(s); game.reset()`):
//   _create_robots                ENV:545-595     leader start by randrange, follower placed behind it (first draw)
//   _create_obstacles             ENV:613-677     two bridge walls, obstacle_number 50x50 rocks by rejection sampling
//   generate_finish_point         ENV:1614-1630   rejection sampling against every game object
//     -- the planner (not here) --
//   _create_dyn_obs/_reset_pose_bear  ENV:687-720, 761-770
//   _pos_follower_behind_leader   ENV:598-611     second follower draw, relative to the leader's new direction
//   initial leader_factual_trajectory  ENV:533-539  np.linspace(float32, float32) -> float32
// Third-party semantics restated here: CPython 3.10 `random` (MT19937 init_by_array, getrandbits, _randbelow_with_getrandbits,
// randrange), pygame.Rect integer truncation (tests/golden/gen/standins, parity unpinned at that boundary as in DESIGN.md 3),
// numpy float32 linspace, scipy euclidean on float32 operands.
//
// What differs between the two callers is a compile-time policy: which atan / cos / sin is called and whether the rejection samplers are
// capped.  HostPolicy is the reference's own: glibc through CPython, no cap (include/ftl.h: the host never sets FTL_SCEN_GEN_LIMIT).
// DevicePolicy is the correctly rounded ftl_crmath.hpp (the device math library differs from glibc by an ulp too often) and
// FTL_SG_MAX_ATTEMPTS draws, after which the scenario is marked FTL_SCEN_GEN_LIMIT.  Everything else is the same operation sequence in
// double / float on both sides (-ffp-contract=off).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/ftl.h"
#include "ftl_crmath.hpp"

#if defined(__HIPCC__)
#define FTL_SC_FN __host__ __device__ inline
#else
#define FTL_SC_FN inline
#endif

#define FTL_SG_MAX_ATTEMPTS (1 << 20)

namespace ftl_sc {

struct HostPolicy {
    static constexpr int max_draws = 0;                       // no cap
    static FTL_SC_FN double atan(double x) { return ::atan(x); }
    static FTL_SC_FN double cos(double x) { return ::cos(x); }
    static FTL_SC_FN double sin(double x) { return ::sin(x); }
};
struct DevicePolicy {
    static constexpr int max_draws = FTL_SG_MAX_ATTEMPTS;
    static FTL_SC_FN double atan(double x) { return ftl_cr::atan(x); }
    static FTL_SC_FN double cos(double x) { return ftl_cr::cos(x); }
    static FTL_SC_FN double sin(double x) { return ftl_cr::sin(x); }
};
// attempt `a` of a rejection loop: true once the policy's cap is used up (never without a cap)
template <class P> FTL_SC_FN bool out_of_draws(int& a) { return P::max_draws && a++ >= P::max_draws; }

// ---- the parameters both sides read: ftl_scen_params as it is, and what the generator needs of ftl_config
struct Params {
    ftl_scen_params sp;                // fixed_route: where the caller's side can read it (the device entry point points it at its copy)
    int32_t n_static, n_bears, route_cap, init_traj_cap;
    int32_t leader_img_w, leader_img_h, follower_img_w, follower_img_h, bear_img_w, bear_img_h;
};
inline Params make_params(const ftl_config& c, const ftl_scen_params& sp) {
    Params p{sp, c.n_static, c.n_bears, c.route_cap, c.init_traj_cap,
             c.leader.img_w, c.leader.img_h, c.follower.img_w, c.follower.img_h, c.bear.img_w, c.bear.img_h};
    if (sp.planner != 2) p.sp.fixed_route_len = 0;
    return p;
}

// The argument check of the three entry points: null, or why the call is invalid.
inline const char* check_args(const ftl_config* cfg, const ftl_scen_params* sp, int32_t n) {
    if (!cfg || !sp) return "null argument";
    if (n < 0) return "n < 0";
    if (sp->step_grid <= 0 || sp->width <= 0 || sp->height <= 0 || sp->trajectory_saving_period <= 0 || !(sp->leader_max_speed > 0))
        return "scenario parameters out of range";
    if (cfg->n_static != (sp->add_obstacles ? sp->obstacle_number + 2 : 0)) return "n_static does not match the obstacles";
    if (cfg->n_bears != (sp->add_bear ? sp->bear_number : 0)) return "n_bears does not match the bears";
    if (sp->planner < 0 || sp->planner > 2 || (sp->planner == 2 && (sp->fixed_route_len < 0 || (sp->fixed_route_len > 0 && !sp->fixed_route))))
        return "bad planner / fixed route";
    return nullptr;
}
inline bool has_every_array(const ftl_scenarios& o) {
    return o.static_rects && o.robot_pos && o.robot_dir && o.robot_rect && o.route && o.route_len && o.init_traj && o.init_traj_len;
}

// ---- CPython random.Random (Modules/_randommodule.c, Lib/random.py) on the caller's 624 words of state
template <class P> struct PyRandom {
    uint32_t* mt; int idx; bool limit;             // limit: a capped loop ran out (the scenario becomes FTL_SCEN_GEN_LIMIT)
    FTL_SC_FN void init_genrand(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    FTL_SC_FN void init_by_array(const uint32_t* key, int len) {
        init_genrand(19650218u);
        int i = 1, j = 0;
        for (int k = (624 > len ? 624 : len); k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            i++; j++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
            if (j >= len) j = 0;
        }
        for (int k = 623; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            i++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
    }
    FTL_SC_FN void seed(int64_t a) {                 // random.seed(int): key = 32-bit little-endian digits of abs(a)
        uint64_t u = a < 0 ? (uint64_t)(-(a + 1)) + 1u : (uint64_t)a;
        uint32_t key[2] = {(uint32_t)u, (uint32_t)(u >> 32)};
        init_by_array(key, key[1] ? 2 : 1);
        limit = false;
    }
    FTL_SC_FN uint32_t next() {
        if (idx >= 624) {
            int kk;
            for (kk = 0; kk < 624 - 397; kk++) { uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu); mt[kk] = mt[kk + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u); }
            for (; kk < 623; kk++) { uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu); mt[kk] = mt[kk + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u); }
            uint32_t y = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
            mt[623] = mt[396] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    }
    FTL_SC_FN uint32_t randbelow(uint32_t n) {       // _randbelow_with_getrandbits, n < 2^32
        int k = 0; for (uint32_t v = n; v; v >>= 1) k++;
        uint32_t r = next() >> (32 - k);
        for (int a = 0; r >= n;) {
            if (out_of_draws<P>(a)) { limit = true; return 0; }
            r = next() >> (32 - k);
        }
        return r;
    }
    // randrange(start, stop, step) with positive step; ok=false where CPython raises ValueError (empty range)
    FTL_SC_FN int64_t randrange(int64_t start, int64_t stop, int64_t step, bool& ok) {
        int64_t width = stop - start;
        int64_t n = step == 1 ? width : (width + step - 1) / step;
        if (n <= 0) { ok = false; return start; }
        return start + step * (int64_t)randbelow((uint32_t)n);
    }
};

struct Rect {
    int x, y, w, h;
    FTL_SC_FN int right() const { return x + w; }
    FTL_SC_FN int bottom() const { return y + h; }
};
struct Obj { Rect r; float px, py; int w, h; };             // GameObject: rectangle, float32 start_position, height/width

// image.get_rect(center=position, width=w, height=h) on an image already scaled to (w, h): CLS:42-50
FTL_SC_FN Rect rect_at(float cx, float cy, int w, int h) { return Rect{(int)cx - (w >> 1), (int)cy - (h >> 1), w, h}; }
FTL_SC_FN bool collidepoint(const Rect& r, double px, double py) { return r.x <= px && px < r.x + r.w && r.y <= py && py < r.y + r.h; }
FTL_SC_FN double angle_correction(double a) { return a >= 360 ? a - 360 : (a < 0 ? 360 + a : a); }   // MISC:6-13
template <class P> FTL_SC_FN double angle_to_point(double cx, double cy, double tx, double ty) {      // MISC:16-26
    const double rx = tx - cx, ry = ty - cy;
    double res;
    if (rx > 0) res = P::atan(ry / rx) * (180.0 / M_PI);
    else if (rx < 0) res = P::atan(ry / rx) * (180.0 / M_PI) + 180;
    else res = 0;
    return angle_correction(res);
}
FTL_SC_FN double radians(double d) { return d * (M_PI / 180.0); }
// scipy.spatial.distance.euclidean on two float32 vectors (oracle/ftl_oracle.c euclid_f32)
FTL_SC_FN double euclid_f32(float ax, float ay, float bx, float by) {
    float dx = ax - bx, dy = ay - by;
    return (double)(float)sqrt((double)dx * (double)dx + (double)dy * (double)dy);
}

// ---- the program before the planner, and what it hands on
struct Start {
    int64_t fx[3], fy[3];              // finish points (the 2nd and 3rd with multiple_end_points only; none with a fixed route)
    float lpx, lpy;                    // the leader
    double ldir0;
    Rect lrect, frect0;                // the follower as first placed
    int nobjs;                         // statics in objs, in game_object_list order: wall1, wall2, rocks...
    int ok, limit;                     // !ok: an empty randrange (CPython raises ValueError); limit: the policy's cap ran out
    int mt_idx;                        // PyRandom::idx, to resume the stream after the planner
};

// generate_finish_point (ENV:1614-1630) against [leader, follower (as first placed), statics]
template <class P> FTL_SC_FN void finish_point(const Params& p, PyRandom<P>& rnd, const Rect& lrect, const Rect& frect0, const Obj* objs, int nobjs,
                                               bool& ok, int64_t x0, int64_t y0, int64_t x1, int64_t y1, int64_t& fx, int64_t& fy) {
    for (int a = 0;;) {
        if (out_of_draws<P>(a)) { rnd.limit = true; return; }
        fx = rnd.randrange(x0, x1, 10, ok); fy = rnd.randrange(y0, y1, 10, ok);
        if (!ok || rnd.limit) return;
        bool good = true;
        for (int o = -2; o < nobjs; o++) {
            const Rect r = o == -2 ? lrect : (o == -1 ? frect0 : objs[o].r);
            if (collidepoint(r, (double)fx, (double)fy)) { good = false; continue; }
            // distance_to_rect (MISC:29-44): corners and edge mid-points, integer coordinates
            const int qx[8] = {r.x, r.x, r.x + r.w, r.x + r.w, r.x + (r.w >> 1), r.x, r.x + (r.w >> 1), r.x + r.w};
            const int qy[8] = {r.y, r.y + r.h, r.y, r.y + r.h, r.y, r.y + (r.h >> 1), r.y + r.h, r.y + (r.h >> 1)};
            double md = INFINITY;
            for (int k = 0; k < 8; k++) { double dx = (double)(fx - qx[k]), dy = (double)(fy - qy[k]); md = fmin(md, sqrt(dx * dx + dy * dy)); }
            if (md < p.sp.leader_pos_epsilon) good = false;
        }
        if (good) return;
    }
}

// Robots, walls, rocks, finish points.  mt: 624 words, objs: p.n_static entries, both the caller's.
template <class P> FTL_SC_FN void before_planner(const Params& p, int64_t seed, uint32_t* mt, Obj* objs, Start& S) {
    const ftl_scen_params& sp = p.sp;
    PyRandom<P> rnd; rnd.mt = mt; rnd.seed(seed);
    bool ok = true;
    const int W = sp.width, H = sp.height, sg = sp.step_grid;
    // ---- _create_robots (ENV:545-595)
    const int64_t lx = rnd.randrange((int64_t)(W / 2.0 + sp.max_distance), (int64_t)(W - sp.max_distance), 10, ok);
    const int64_t ly = rnd.randrange((int64_t)sp.max_distance, (int64_t)(H - sp.max_distance), 10, ok);
    const double ldir0 = angle_to_point<P>((double)lx, (double)ly, (double)(int64_t)(W / 2.0), (double)(int64_t)(H / 2.0));   // np.array(..., dtype=int)
    const float lpx = (float)lx, lpy = (float)ly;
    const Rect lrect = rect_at(lpx, lpy, p.leader_img_w, p.leader_img_h);
    Rect frect0;
    {
        const int64_t d = rnd.randrange((int64_t)(sp.min_distance * 1.1), (int64_t)(sp.max_distance * 0.9), 1, ok);
        const double th = radians(angle_correction(ldir0 + 180));
        const double fx = (double)d * P::cos(th) + (double)lx, fy = (double)d * P::sin(th) + (double)ly;
        frect0 = rect_at((float)fx, (float)fy, p.follower_img_w, p.follower_img_h);
    }
    // ---- _create_obstacles (ENV:613-677); game_object_list = [leader, follower, wall1, wall2, rocks...]
    int nobjs = 0;
    if (sp.add_obstacles) {
        const int boh = (H - sp.bridge_gap) / 2;                              // bridge_obstacle_height
        const float m1x = (float)(W / 2.0), m1y = (float)(boh / 2);
        const float m2y = (float)((H / 2) + (boh / 2) + (sp.bridge_gap / 2));
        const Obj w1{rect_at(m1x, m1y, sp.bridge_width, boh), m1x, m1y, sp.bridge_width, boh};
        const Obj w2{rect_at(m1x, m2y, sp.bridge_width, boh), m1x, m2y, sp.bridge_width, boh};
        const int wall_start_x = w1.r.x, wall_end_x = w1.r.right();
        // pygame.Rect(...) truncates each float argument toward zero
        const Rect bridge{(int)(wall_start_x - sp.leader_w * 4), (int)(w1.r.bottom() - sp.leader_h * sp.leader_margin),
                          (int)(w1.r.w + 8 * sp.leader_w), (int)(w2.r.y - w1.r.bottom() + 3 * sp.leader_h)};
        const int osz = 50;
        objs[0] = w1; objs[1] = w2; nobjs = 2;
        for (int i = 0; i < sp.obstacle_number && ok && !rnd.limit; i++) {
            int64_t gx2 = 0, gy2 = 0;
            for (int a = 0;;) {
                if (out_of_draws<P>(a)) { rnd.limit = true; break; }
                gx2 = rnd.randrange(130, W - 120, sg, ok); gy2 = rnd.randrange(20, H - 20, sg, ok);
                if (!ok || rnd.limit) break;
                const double ddx = (double)lpx - (double)gx2, ddy = (double)lpy - (double)gy2;
                const bool busy = collidepoint(lrect, (double)gx2, (double)gy2) || collidepoint(frect0, (double)gx2, (double)gy2) ||
                                  (gx2 >= wall_start_x && gx2 <= wall_end_x) || collidepoint(bridge, (double)gx2, (double)gy2) ||
                                  sqrt(ddx * ddx + ddy * ddy) <= sp.max_distance + osz / 2.0;
                if (!busy) break;
            }
            objs[nobjs++] = Obj{rect_at((float)gx2, (float)gy2, osz, osz), (float)gx2, (float)gy2, osz, osz};
        }
    }
    int64_t f1x = 0, f1y = 0, f2x = 0, f2y = 0, f3x = 0, f3y = 0;
    const bool fixed = sp.planner == 2;                                        // trajectory= of the constructor: ENV:470 skips all of this
    const int64_t xm = (int64_t)(W / 2.0), ym = (int64_t)(H / 2.0);
    if (!fixed && !rnd.limit) finish_point(p, rnd, lrect, frect0, objs, nobjs, ok, 20, 20, xm, H - 20, f1x, f1y);
    if (!fixed && sp.multiple_end_points && ok && !rnd.limit) {                // ENV:470-481: each next one in the other half of the field
        if (f1y >= H / 2.0) finish_point(p, rnd, lrect, frect0, objs, nobjs, ok, 20, 20, W - 20, ym, f2x, f2y);
        else finish_point(p, rnd, lrect, frect0, objs, nobjs, ok, 20, ym, W - 20, H - 20, f2x, f2y);
        if (ok && !rnd.limit) {
            if (f2y >= H / 2.0) finish_point(p, rnd, lrect, frect0, objs, nobjs, ok, 20, 20, W - 20, ym, f3x, f3y);
            else finish_point(p, rnd, lrect, frect0, objs, nobjs, ok, 20, ym, W - 20, H - 20, f3x, f3y);
        }
    }
    S.fx[0] = f1x; S.fy[0] = f1y; S.fx[1] = f2x; S.fy[1] = f2y; S.fx[2] = f3x; S.fy[2] = f3y;
    S.lpx = lpx; S.lpy = lpy; S.ldir0 = ldir0; S.lrect = lrect; S.frect0 = frect0;
    S.nobjs = nobjs; S.ok = ok; S.limit = rnd.limit; S.mt_idx = rnd.idx;
}

// ---- the program after the planner: the leader's direction from route[1] = (r1x, r1y) (read when rl >= 2), the follower's second draw,
// robots, status, route_len, init_traj_len.  rl counts every route point, found is the planner's (true where none ran).
struct Linspace { int n; float fpx, fpy, lpx, lpy, div, dxx, dyy, stepx, stepy; };   // initial trajectory: n points follower -> leader

template <class P> FTL_SC_FN void after_planner(const Params& p, const Start& S, uint32_t* mt, bool found, int rl, double r1x, double r1y,
                                                const ftl_scenarios& out, uint8_t* status, int idx, Linspace& L) {
    const ftl_scen_params& sp = p.sp;
    const int R = 2 + p.n_bears;
    const float lpx = S.lpx, lpy = S.lpy;
    PyRandom<P> rnd; rnd.mt = mt; rnd.idx = S.mt_idx; rnd.limit = false;
    bool ok = S.ok;
    unsigned st = 0;
    if (found && ok && !S.limit) st |= FTL_SCEN_FOUND;
    if (rl == 0) st |= FTL_SCEN_DONE_AT_RESET;
    if (rl == 1) st |= FTL_SCEN_REF_RAISES;
    // ---- leader direction, follower behind the leader (ENV:506-525, 598-611)
    double ldir = S.ldir0;
    float fpx = lpx, fpy = lpy; double fdir = 0;
    if (ok && !S.limit) {
        double tx = (double)lpx, ty = (double)lpy;              // len(trajectory) == 0: cur_target_point = leader.start_position
        if (rl >= 2) { tx = r1x; ty = r1y; }
        ldir = angle_to_point<P>((double)lpx, (double)lpy, tx, ty);
        const int64_t d = rnd.randrange((int64_t)(sp.min_distance * 1.1), (int64_t)(sp.max_distance * 0.9), 1, ok);
        const double th = angle_correction(ldir + 180);
        const double fx = (double)d * P::cos(radians(th)) + (double)lpx, fy = (double)d * P::sin(radians(th)) + (double)lpy;
        fdir = angle_to_point<P>(fx, fy, (double)lpx, (double)lpy);
        fpx = (float)fx; fpy = (float)fy;
    }
    float* rp = const_cast<float*>(out.robot_pos) + (size_t)idx * R * 2;
    double* rd = const_cast<double*>(out.robot_dir) + (size_t)idx * R;
    int32_t* rr = const_cast<int32_t*>(out.robot_rect) + (size_t)idx * R * 4;
    auto put = [&](int r, float x, float y, double dir, Rect q) {
        rp[2 * r] = x; rp[2 * r + 1] = y; rd[r] = dir; rr[4 * r] = q.x; rr[4 * r + 1] = q.y; rr[4 * r + 2] = q.w; rr[4 * r + 3] = q.h;
    };
    put(0, lpx, lpy, ldir, S.lrect);
    put(1, fpx, fpy, fdir, rect_at(fpx, fpy, p.follower_img_w, p.follower_img_h));
    for (int b = 0; b < p.n_bears; b++) {                     // _reset_pose_bear (ENV:761-770); float32 arithmetic on leader.position
        const float bx = (b % 2 == 0) ? lpx + 150.0f : lpx - 150.0f, by = (b % 2 == 0) ? lpy - 150.0f : lpy + 150.0f;
        put(2 + b, bx, by, 0.0, rect_at(bx, by, p.bear_img_w, p.bear_img_h));
    }
    if (rl > p.route_cap) st |= FTL_SCEN_ROUTE_OVERFLOW;
    // ---- initial leader_factual_trajectory (ENV:533-539): float32 linspace follower -> leader
    int n = (int)(euclid_f32(fpx, fpy, lpx, lpy) / (sp.trajectory_saving_period * sp.leader_max_speed));
    if (n < 0) n = 0;
    if (n > p.init_traj_cap) { st |= FTL_SCEN_TRAJ_OVERFLOW; n = p.init_traj_cap; }
    if (!ok) st = FTL_SCEN_REF_RAISES;                          // an empty randrange: CPython raises ValueError
    if (S.limit || rnd.limit) st = FTL_SCEN_GEN_LIMIT;
    status[idx] = (uint8_t)st;
    const_cast<int32_t*>(out.route_len)[idx] = rl < p.route_cap ? rl : p.route_cap;
    const_cast<int32_t*>(out.init_traj_len)[idx] = n;
    L = Linspace{n, fpx, fpy, lpx, lpy, 0, 0, 0, 0, 0};
    if (n > 1) {
        L.div = (float)(n - 1); L.dxx = lpx - fpx; L.dyy = lpy - fpy;
        L.stepx = L.dxx / L.div; L.stepy = L.dyy / L.div;
    }
}

// ---- element by element (the host loops over i, the device strides it over the lanes)
// row i of the scenario's init_traj: point i of the linspace, the last one exact, zero from n on
FTL_SC_FN void traj_point(const Linspace& L, float* it, int i) {
    float x = 0, y = 0;
    if (i < L.n) {
        if (L.n == 1) { x = L.fpx; y = L.fpy; }
        else if (i == L.n - 1) { x = L.lpx; y = L.lpy; }
        else {
            x = (L.stepx == 0) ? ((float)i / L.div) * L.dxx + L.fpx : (float)i * L.stepx + L.fpx;
            y = (L.stepy == 0) ? ((float)i / L.div) * L.dyy + L.fpy : (float)i * L.stepy + L.fpy;
        }
    }
    it[2 * i] = x; it[2 * i + 1] = y;
}
// row s of the scenario's static_rects
FTL_SC_FN void static_rect_row(const Obj* objs, int nobjs, int32_t* srect, int s) {
    const Rect r = s < nobjs ? objs[s].r : Rect{0, 0, 0, 0};
    srect[4 * s] = r.x; srect[4 * s + 1] = r.y; srect[4 * s + 2] = r.w; srect[4 * s + 3] = r.h;
}
// row i of the scenario's route, past its last point
FTL_SC_FN void route_pad(double* ro, int i) { ro[2 * i] = 0; ro[2 * i + 1] = 0; }

}  // namespace ftl_sc
