// ftl_scenario_dev.hpp -- ftl_generate_scenarios_device: the host generator of ftl_scenario.cpp (generate_one) as a gfx950 kernel that
// writes scenarios straight into device memory (include/ftl.h).  Included at the end of ftl_abi.hip (same translation
// unit: it shares fail() / ftl_last_error()).
//
// One wavefront per scenario, persistent: a fixed number of wavefronts loop over the seeds, each with its own slice of the caller's
// workspace (so the scratch does not grow with n).  The `random`-driven parts (MT19937 seeding, robots, bridge walls, rocks, finish points,
// the follower's second draw) are a short sequential program: lane 0 runs it on an LDS copy of the MT state, exactly as generate_one does,
// draw for draw.  The planner (nine tenths of a scenario on the host) is wave-parallel:
//
//   plan_route pops the open list bucket by unit-wide bucket; every move costs >= 1, so a relaxation from bucket i lands in a LATER bucket,
//   bucket i is complete when it comes up, and within it the host's stable sort pops in the order (h, global pop index of the node that
//   set h, neighbour index d).  Here a bucket is every open node with h < floor(min h) + 1, popped all at once: each gets its rank in that
//   order (pop index = pops so far + rank), then its neighbours are relaxed in two phases -- a 64-bit atomic minimum over the bit pattern
//   of h (all h >= 0, so the bits order like the doubles), then, among the relaxations that reached the final h of a node lowered in this
//   bucket, an atomic minimum over the tag pop_index * 8 + d.  The winner of the tag is the host's parent (nid - doff[d]).  Nodes popped
//   after the start in its own bucket do not relax (the host stops at the start).  A bucket close enough to the end of the host's bucket
//   array that a relaxation could overflow it (the `to >= nb` quirk, ftl_scenario.cpp plan_route) is run by lane 0 in pop order, with
//   the host's own early return -- never on a real grid, but the outputs stay the host's.
//
// Every loop is bounded: the rejection samplers (rocks, finish points) and randbelow stop after FTL_SG_MAX_ATTEMPTS draws and mark the
// scenario FTL_SCEN_GEN_LIMIT (unusable; the host never gets there on a real seed), a bucket closes at least one node, the parent walk
// stops at max_iterat or after every cell.
// Numerics: the same double / float operation sequence as the host (-ffp-contract=off); atan (leader / follower directions) and cos / sin
// (the follower's placement) are the correctly rounded ones of ftl_crmath.hpp, not the device math library's (which differs from glibc
// by an ulp often enough to change the start direction of 2-12 % of the worlds).
#pragma once
#include "../../include/ftl.h"
#include "ftl_crmath.hpp"

#define FTL_SG_MAX_ATTEMPTS (1 << 20)
#define FTL_SG_MAX_WAVES 2048           // persistent wavefronts (8 per CU on 256 CUs): the workspace holds one slice per wavefront
#define FTL_SG_MAX_CELLS 65536          // (rows + 2) * (cols + 2) of the D* grid: node ids and pop indices fit the 32-bit tag

struct FtlSgArgs {
    // ftl_scen_params
    int32_t width, height, step_grid, obstacle_number, add_obstacles, multiple_end_points, path_finding_iterations;
    int32_t bridge_gap, bridge_width, trajectory_saving_period, planner, fixed_route_len;
    double min_distance, max_distance, leader_pos_epsilon, leader_margin, leader_w, leader_h, leader_max_speed;
    const double* fixed_route;         // device copy (workspace)
    // ftl_config
    int32_t n_static, n_bears, route_cap, init_traj_cap;
    int32_t leader_w_img, leader_h_img, follower_w_img, follower_h_img, bear_w_img, bear_h_img;
    // grid
    int32_t rows, cols, W2, N2, nwords;
    // launch
    const int64_t* seeds; int32_t n;
    ftl_scenarios out; uint8_t* status;
    char* ws; size_t ws_per_wave;
};

namespace ftl_sg {

struct Rect { int x, y, w, h; };
struct Obj { Rect r; float px, py; int w, h; };

__device__ inline Rect rect_at(float cx, float cy, int w, int h) { return Rect{(int)cx - (w >> 1), (int)cy - (h >> 1), w, h}; }
__device__ inline bool collidepoint(const Rect& r, double px, double py) { return r.x <= px && px < r.x + r.w && r.y <= py && py < r.y + r.h; }
__device__ inline double angle_correction(double a) { return a >= 360 ? a - 360 : (a < 0 ? 360 + a : a); }
__device__ inline double angle_to_point(double cx, double cy, double tx, double ty) {
    const double rx = tx - cx, ry = ty - cy;
    double res;
    if (rx > 0) res = ftl_cr::atan(ry / rx) * (180.0 / M_PI);
    else if (rx < 0) res = ftl_cr::atan(ry / rx) * (180.0 / M_PI) + 180;
    else res = 0;
    return angle_correction(res);
}
__device__ inline double radians(double d) { return d * (M_PI / 180.0); }
__device__ inline double euclid_f32(float ax, float ay, float bx, float by) {
    float dx = ax - bx, dy = ay - by;
    return (double)(float)sqrt((double)dx * (double)dx + (double)dy * (double)dy);
}

// CPython random.Random on an LDS copy of the state (ftl_scenario.cpp PyRandom); one lane at a time
struct PyRandom {
    uint32_t* mt; int idx; bool limit;
    __device__ void init_genrand(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    __device__ void init_by_array(const uint32_t* key, int len) {
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
    __device__ void seed(int64_t a) {
        uint64_t u = a < 0 ? (uint64_t)(-(a + 1)) + 1u : (uint64_t)a;
        uint32_t key[2] = {(uint32_t)u, (uint32_t)(u >> 32)};
        init_by_array(key, key[1] ? 2 : 1);
        limit = false;
    }
    __device__ uint32_t next() {
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
    __device__ uint32_t randbelow(uint32_t n) {
        int k = 0; for (uint32_t v = n; v; v >>= 1) k++;
        uint32_t r = next() >> (32 - k);
        for (int a = 0; r >= n; a++) {
            if (a >= FTL_SG_MAX_ATTEMPTS) { limit = true; return 0; }
            r = next() >> (32 - k);
        }
        return r;
    }
    __device__ int64_t randrange(int64_t start, int64_t stop, int64_t step, bool& ok) {
        int64_t width = stop - start;
        int64_t n = step == 1 ? width : (width + step - 1) / step;
        if (n <= 0) { ok = false; return start; }
        return start + step * (int64_t)randbelow((uint32_t)n);
    }
};

// what lane 0 hands to the wave between the sequential parts
struct Shared {
    int64_t f1x, f1y, f2x, f2y, f3x, f3y;
    float lpx, lpy;
    double ldir0;
    Rect lrect;
    int nobjs, ok, limit, found, rl, fail;
    double r1x, r1y;                  // route[1] (the leader's first target point)
    // D*
    int m_open, start_rank, mt_idx, n_traj;
    float fpx, fpy;
};

// cross-lane traffic through the workspace (global atomics are performed in L2): a device-scope fence before the barrier, so that no
// lane reads a stale vector-L1 line of what another lane wrote or updated
__device__ inline void wave_sync() { __threadfence(); __syncthreads(); }

__device__ inline bool bit(const uint32_t* b, int i) { return (b[i >> 5] >> (i & 31)) & 1u; }

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// plan_route (ftl_scenario.cpp) for one leg; appends the route cells * sg to the output route (first route_cap points), counting all.
// Returns the host's bool.  Whole wave; obst = inflated obstacles + one-cell border (bit array), closed = bit array (cleared here).
__device__ bool plan_route_wave(const FtlSgArgs& A, Shared& S, const uint32_t* obst, uint32_t* closed, int sx, int sy, int gx, int gy,
                                int max_iterat, double* hh, uint32_t* tag, int* open, int* front, double* route_out) {
    const int lane = threadIdx.x;
    const int rows = A.rows, cols = A.cols, W2 = A.W2, N2 = A.N2;
    auto in = [&](int x, int y) { return x >= 0 && x < rows && y >= 0 && y < cols; };
    if (!in(sx, sy) || !in(gx, gy)) return false;
    if (sx == gx && sy == gy) return true;
    const int goal = (gx + 1) * W2 + gy + 1, start = (sx + 1) * W2 + sy + 1;
    if (bit(obst, goal) || bit(obst, start)) return false;
    const int nb = rows + cols + 8;
    const double INF = 1e300;
    const unsigned long long INFB = (unsigned long long)__double_as_longlong(INF);
    const double SQ2 = sqrt(2.0);
    const int doff[8] = {-W2 - 1, -W2, -W2 + 1, -1, 1, W2 - 1, W2, W2 + 1};
    const double dcost[8] = {SQ2, 1.0, SQ2, 1.0, 1.0, SQ2, 1.0, SQ2};
    for (int i = lane; i < N2; i += 64) hh[i] = INF;
    for (int i = lane; i < A.nwords; i += 64) closed[i] = 0u;
    wave_sync();
    if (lane == 0) { hh[goal] = 0.0; tag[goal] = 0u; open[0] = goal; S.m_open = 1; S.fail = 0; }
    wave_sync();
    unsigned base = 0;                                          // pops so far
    bool reached = false;
    for (int iter = 0; iter <= N2 && !reached; iter++) {       // every bucket closes at least one node
        const int m = S.m_open;
        if (m == 0) break;                                      // open list ran dry: unreachable goal
        // the bucket: open nodes with h < floor(min h) + 1
        unsigned long long mn = INFB;
        for (int i = lane; i < m; i += 64) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(hh[open[i]]);
            mn = b < mn ? b : mn;
        }
        mn = wave_min_u64(mn);
        const int bi = (int)__longlong_as_double((long long)mn);
        const double lim = (double)bi + 1.0;
        int nf = 0, no = 0;
        for (int c0 = 0; c0 < m; c0 += 64) {                    // in-place compaction: chunk read before any write at or after it
            const int i = c0 + lane;
            const int id = i < m ? open[i] : -1;
            const bool isf = i < m && hh[id] < lim;
            const unsigned long long bf = __ballot(isf), bo = __ballot(i < m && !isf);
            const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
            __syncthreads();
            if (isf) front[nf + __popcll(bf & below)] = id;
            else if (i < m) open[no + __popcll(bo & below)] = id;
            nf += __popcll(bf); no += __popcll(bo);
        }
        wave_sync();
        for (int i = lane; i < nf; i += 64) { const int id = front[i]; atomicOr(&closed[id >> 5], 1u << (id & 31)); }
        if (lane == 0) { S.m_open = no; S.start_rank = 0x7fffffff; }
        __syncthreads();
        // rank of every popped node in the host's order (h, tag); keys are distinct
        bool has_start = false;
        for (int c0 = 0; c0 < nf; c0 += 64) {
            const int i = c0 + lane;
            if (i < nf) {
                const int id = front[i];
                const double h0 = hh[id]; const uint32_t t0 = tag[id];
                int r = 0;
                for (int j = 0; j < nf; j++) {
                    const int jd = front[j];
                    const double h1 = hh[jd];
                    r += (h1 < h0 || (h1 == h0 && tag[jd] < t0)) ? 1 : 0;
                }
                open[N2 + i] = r;                               // (the second half of the open-list slice holds the ranks)
                if (id == start) { S.start_rank = r; }
            }
        }
        wave_sync();
        has_start = S.start_rank != 0x7fffffff;
        const int srank = S.start_rank;
        const int* rank = open + N2;
        if (bi + 2 >= nb) {
            // near the end of the host's bucket array: lane 0 pops in order with the host's early return on an overflowing push
            if (lane == 0) {
                for (int r = 0; r < nf && r < srank; r++) {
                    int id = -1;
                    for (int j = 0; j < nf; j++) if (rank[j] == r) { id = front[j]; break; }
                    const double k = hh[id];
                    for (int d = 0; d < 8; d++) {
                        const int nid = id + doff[d];
                        if (bit(obst, nid) || bit(closed, nid)) continue;
                        const double hn = k + dcost[d];
                        if (hn < hh[nid]) {
                            const bool fresh = hh[nid] == INF;
                            hh[nid] = hn; tag[nid] = (base + (unsigned)r) * 8u + (unsigned)d;
                            if ((int)hn >= nb) { S.fail = 1; break; }
                            if (fresh) open[S.m_open++] = nid;
                        }
                    }
                    if (S.fail) break;
                }
            }
            wave_sync();
            if (S.fail) return false;
        } else {
            // phase A: h = min over the relaxations (64-bit minimum on the bit pattern); a lowered node's tag is reset, a new one opened
            for (int c0 = 0; c0 < nf; c0 += 64) {
                const int i = c0 + lane;
                if (i < nf && rank[i] < srank) {
                    const int id = front[i];
                    const double k = hh[id];
                    for (int d = 0; d < 8; d++) {
                        const int nid = id + doff[d];
                        if (bit(obst, nid) || bit(closed, nid)) continue;
                        const double hn = k + dcost[d];
                        const unsigned long long hb = (unsigned long long)__double_as_longlong(hn);
                        const unsigned long long old = atomicMin((unsigned long long*)&hh[nid], hb);
                        if (hb < old) {
                            tag[nid] = 0xffffffffu;
                            if (old == INFB) open[atomicAdd(&S.m_open, 1)] = nid;
                        }
                    }
                }
            }
            wave_sync();
            // phase B: the first setter of the final h, in pop order, among nodes lowered in this bucket (their tag is >= base * 8)
            for (int c0 = 0; c0 < nf; c0 += 64) {
                const int i = c0 + lane;
                if (i < nf && rank[i] < srank) {
                    const int id = front[i];
                    const double k = hh[id];
                    const unsigned pk = (base + (unsigned)rank[i]) * 8u;
                    for (int d = 0; d < 8; d++) {
                        const int nid = id + doff[d];
                        if (bit(obst, nid) || bit(closed, nid)) continue;
                        const double hn = k + dcost[d];
                        if (hn == hh[nid] && tag[nid] >= base * 8u)
                            atomicMin(&tag[nid], pk + (unsigned)d);
                    }
                }
            }
            wave_sync();
        }
        base += (unsigned)nf;
        reached = has_start;
    }
    if (!reached) return false;
    // the parent walk (lane 0), written straight into the output route
    bool ok = true;
    if (lane == 0) {
        int cur = start, it = 0;
        while (cur != goal) {
            if (++it > max_iterat || it > N2) { ok = false; break; }
            const int k = S.rl;
            const double x = (double)((int64_t)(cur / W2 - 1) * A.step_grid), y = (double)((int64_t)(cur % W2 - 1) * A.step_grid);
            if (k < A.route_cap) { route_out[2 * k] = x; route_out[2 * k + 1] = y; }
            if (k == 1) { S.r1x = x; S.r1y = y; }
            S.rl = k + 1;
            cur = cur - doff[tag[cur] & 7u];
            if (cur < 0 || cur >= N2) { ok = false; break; }          // (cannot happen: a closed node's tag names a neighbour)
        }
        S.fail = ok ? 0 : 1;
    }
    __syncthreads();
    return S.fail == 0;
}

__global__ void __launch_bounds__(64) ftl_scenario_gen_kernel(const FtlSgArgs A) {
    extern __shared__ uint32_t lds[];
    __shared__ Shared S;
    const int lane = threadIdx.x;
    uint32_t* mt = lds;                                          // [624]
    uint32_t* obst = lds + 624;                                  // [nwords]
    uint32_t* closed = obst + A.nwords;                          // [nwords]
    Obj* objs = (Obj*)(closed + A.nwords);                       // [n_static]
    char* ws = A.ws + (size_t)blockIdx.x * A.ws_per_wave;
    double* hh = (double*)ws;
    uint32_t* tag = (uint32_t*)(hh + A.N2);
    int* open = (int*)(tag + A.N2);                              // [2 * N2]: open list, ranks of the bucket
    int* front = open + 2 * A.N2;                                // [N2]
    const int R = 2 + A.n_bears;
    const int W = A.width, H = A.height, sg = A.step_grid;
    const bool fixed = A.planner == 2;
    for (int idx = blockIdx.x; idx < A.n; idx += gridDim.x) {
        double* ro = const_cast<double*>(A.out.route) + (size_t)idx * A.route_cap * 2;
        // ---- the sequential part up to the planner (generate_one: _create_robots, _create_obstacles, generate_finish_point)
        if (lane == 0) {
            PyRandom rnd; rnd.mt = mt; rnd.seed(A.seeds[idx]);
            bool ok = true;
            const int64_t lx = rnd.randrange((int64_t)(W / 2.0 + A.max_distance), (int64_t)(W - A.max_distance), 10, ok);
            const int64_t ly = rnd.randrange((int64_t)A.max_distance, (int64_t)(H - A.max_distance), 10, ok);
            const double ldir0 = angle_to_point((double)lx, (double)ly, (double)(int64_t)(W / 2.0), (double)(int64_t)(H / 2.0));
            const float lpx = (float)lx, lpy = (float)ly;
            const Rect lrect = rect_at(lpx, lpy, A.leader_w_img, A.leader_h_img);
            Rect frect0;
            {
                const int64_t d = rnd.randrange((int64_t)(A.min_distance * 1.1), (int64_t)(A.max_distance * 0.9), 1, ok);
                const double th = radians(angle_correction(ldir0 + 180));
                const double fx = (double)d * ftl_cr::cos(th) + (double)lx, fy = (double)d * ftl_cr::sin(th) + (double)ly;
                frect0 = rect_at((float)fx, (float)fy, A.follower_w_img, A.follower_h_img);
            }
            int nobjs = 0;
            bool limit = false;
            if (A.add_obstacles) {
                const int boh = (H - A.bridge_gap) / 2;
                const float m1x = (float)(W / 2.0), m1y = (float)(boh / 2);
                const float m2y = (float)((H / 2) + (boh / 2) + (A.bridge_gap / 2));
                const Obj w1{rect_at(m1x, m1y, A.bridge_width, boh), m1x, m1y, A.bridge_width, boh};
                const Obj w2{rect_at(m1x, m2y, A.bridge_width, boh), m1x, m2y, A.bridge_width, boh};
                const int wall_start_x = w1.r.x, wall_end_x = w1.r.x + w1.r.w;
                const Rect bridge{(int)(wall_start_x - A.leader_w * 4), (int)(w1.r.y + w1.r.h - A.leader_h * A.leader_margin),
                                  (int)(w1.r.w + 8 * A.leader_w), (int)(w2.r.y - (w1.r.y + w1.r.h) + 3 * A.leader_h)};
                const int osz = 50;
                objs[0] = w1; objs[1] = w2; nobjs = 2;
                for (int i = 0; i < A.obstacle_number && ok && !limit; i++) {
                    int64_t gx2 = 0, gy2 = 0;
                    for (int a = 0;; a++) {
                        if (a >= FTL_SG_MAX_ATTEMPTS) { limit = true; break; }
                        gx2 = rnd.randrange(130, W - 120, sg, ok); gy2 = rnd.randrange(20, H - 20, sg, ok);
                        if (!ok || rnd.limit) break;
                        const double ddx = (double)lpx - (double)gx2, ddy = (double)lpy - (double)gy2;
                        const bool busy = collidepoint(lrect, (double)gx2, (double)gy2) || collidepoint(frect0, (double)gx2, (double)gy2) ||
                                          (gx2 >= wall_start_x && gx2 <= wall_end_x) || collidepoint(bridge, (double)gx2, (double)gy2) ||
                                          sqrt(ddx * ddx + ddy * ddy) <= A.max_distance + osz / 2.0;
                        if (!busy) break;
                    }
                    objs[nobjs++] = Obj{rect_at((float)gx2, (float)gy2, osz, osz), (float)gx2, (float)gy2, osz, osz};
                }
            }
            // generate_finish_point against [leader, follower (as first placed), statics]
            auto finish_point = [&](int64_t x0, int64_t y0, int64_t x1, int64_t y1, int64_t& fx, int64_t& fy) {
                for (int a = 0;; a++) {
                    if (a >= FTL_SG_MAX_ATTEMPTS) { limit = true; return; }
                    fx = rnd.randrange(x0, x1, 10, ok); fy = rnd.randrange(y0, y1, 10, ok);
                    if (!ok || rnd.limit) return;
                    bool good = true;
                    for (int o = -2; o < nobjs; o++) {
                        const Rect r = o == -2 ? lrect : (o == -1 ? frect0 : objs[o].r);
                        if (collidepoint(r, (double)fx, (double)fy)) { good = false; continue; }
                        const int qx[8] = {r.x, r.x, r.x + r.w, r.x + r.w, r.x + (r.w >> 1), r.x, r.x + (r.w >> 1), r.x + r.w};
                        const int qy[8] = {r.y, r.y + r.h, r.y, r.y + r.h, r.y, r.y + (r.h >> 1), r.y + r.h, r.y + (r.h >> 1)};
                        double md = INFINITY;
                        for (int k = 0; k < 8; k++) { double dx = (double)(fx - qx[k]), dy = (double)(fy - qy[k]); md = fmin(md, sqrt(dx * dx + dy * dy)); }
                        if (md < A.leader_pos_epsilon) good = false;
                    }
                    if (good) return;
                }
            };
            int64_t f1x = 0, f1y = 0, f2x = 0, f2y = 0, f3x = 0, f3y = 0;
            if (!fixed && !limit) finish_point(20, 20, (int64_t)(W / 2.0), H - 20, f1x, f1y);
            if (!fixed && A.multiple_end_points && ok && !limit && !rnd.limit) {
                if (f1y >= H / 2.0) finish_point(20, 20, W - 20, (int64_t)(H / 2.0), f2x, f2y);
                else finish_point(20, (int64_t)(H / 2.0), W - 20, H - 20, f2x, f2y);
                if (ok && !limit && !rnd.limit) {
                    if (f2y >= H / 2.0) finish_point(20, 20, W - 20, (int64_t)(H / 2.0), f3x, f3y);
                    else finish_point(20, (int64_t)(H / 2.0), W - 20, H - 20, f3x, f3y);
                }
            }
            S.f1x = f1x; S.f1y = f1y; S.f2x = f2x; S.f2y = f2y; S.f3x = f3x; S.f3y = f3y;
            S.lpx = lpx; S.lpy = lpy; S.ldir0 = ldir0; S.lrect = lrect;
            S.nobjs = nobjs; S.ok = ok; S.limit = limit || rnd.limit;
            S.rl = 0; S.r1x = 0; S.r1y = 0;
            S.found = ok;
            S.mt_idx = rnd.idx;                                  // (the MT state stays in LDS for the follower's second draw)
        }
        __syncthreads();
        const bool ok0 = S.ok && !S.limit;
        if (ok0 && fixed && lane == 0) {
            for (int i = 0; i < A.fixed_route_len; i++) {
                if (i < A.route_cap) { ro[2 * i] = A.fixed_route[2 * i]; ro[2 * i + 1] = A.fixed_route[2 * i + 1]; }
            }
            if (A.fixed_route_len >= 2) { S.r1x = A.fixed_route[2]; S.r1y = A.fixed_route[3]; }
            S.rl = A.fixed_route_len;
        }
        if (ok0 && A.planner == 0) {
            // ---- generate_trajectory_dstar: obstacles inflated onto the grid (+ the border of the host's padded grid)
            const int rows = A.rows, cols = A.cols, W2 = A.W2;
            for (int w = lane; w < A.nwords; w += 64) {
                uint32_t v = 0;
                for (int b = 0; b < 32; b++) {
                    const int id = w * 32 + b;
                    const int x = id / W2, y = id % W2;
                    if (id >= A.N2 || x == 0 || x == rows + 1 || y == 0 || y == cols + 1) v |= 1u << b;
                }
                obst[w] = v;
            }
            __syncthreads();
            const int margin = (int)floor(A.leader_margin * fmax(A.leader_w, A.leader_h) / sg);
            for (int o = lane; o < S.nobjs; o += 64) {
                const Obj ob = objs[o];
                const int pmx = (int)floorf(ob.px / (float)sg), pmy = (int)floorf(ob.py / (float)sg);
                const int hh2 = (int)floor((ob.h / 2.0) / sg) + margin, hw = (int)floor((ob.w / 2.0) / sg) + margin;
                const int i0 = max(pmx - hw, 0), i1 = min(pmx + hw, rows), j0 = max(pmy - hh2, 0), j1 = min(pmy + hh2, cols);
                for (int i = i0; i < i1; i++)
                    for (int j = j0; j < j1; j++) {
                        const int id = (i + 1) * W2 + j + 1;
                        atomicOr(&obst[id >> 5], 1u << (id & 31));
                    }
            }
            __syncthreads();
            int sx = (int)(S.lpx / (float)sg), sy = (int)(S.lpy / (float)sg);
            const int64_t gxs[3] = {S.f1x, S.f2x, S.f3x}, gys[3] = {S.f1y, S.f2y, S.f3y};
            const int runs = A.multiple_end_points ? 3 : 1;
            bool found = true;
            for (int k = 0; k < runs; k++) {
                const int gx = (int)((double)gxs[k] / sg), gy = (int)((double)gys[k] / sg);
                const bool f = plan_route_wave(A, S, obst, closed, sx, sy, gx, gy, k == 0 ? A.path_finding_iterations : 15000,
                                               hh, tag, open, front, ro);
                found = found && f;
                sx = gx; sy = gy;
            }
            if (lane == 0) S.found = found;
            __syncthreads();
        }
        // ---- leader direction, the follower behind the leader, outputs
        const float lpx = S.lpx, lpy = S.lpy;
        const int rl = S.rl;
        if (lane == 0) {
            PyRandom rnd; rnd.mt = mt; rnd.idx = S.mt_idx; rnd.limit = false;
            bool ok = S.ok;
            unsigned st = 0;
            if (S.found && ok0) st |= FTL_SCEN_FOUND;
            if (rl == 0) st |= FTL_SCEN_DONE_AT_RESET;
            if (rl == 1) st |= FTL_SCEN_REF_RAISES;
            double ldir = S.ldir0;
            float fpx = lpx, fpy = lpy; double fdir = 0;
            if (ok && !S.limit) {
                double tx = (double)lpx, ty = (double)lpy;
                if (rl >= 2) { tx = S.r1x; ty = S.r1y; }
                ldir = angle_to_point((double)lpx, (double)lpy, tx, ty);
                const int64_t d = rnd.randrange((int64_t)(A.min_distance * 1.1), (int64_t)(A.max_distance * 0.9), 1, ok);
                const double th = angle_correction(ldir + 180);
                const double fx = (double)d * ftl_cr::cos(radians(th)) + (double)lpx, fy = (double)d * ftl_cr::sin(radians(th)) + (double)lpy;
                fdir = angle_to_point(fx, fy, (double)lpx, (double)lpy);
                fpx = (float)fx; fpy = (float)fy;
            }
            float* rp = const_cast<float*>(A.out.robot_pos) + (size_t)idx * R * 2;
            double* rd = const_cast<double*>(A.out.robot_dir) + (size_t)idx * R;
            int32_t* rr = const_cast<int32_t*>(A.out.robot_rect) + (size_t)idx * R * 4;
            auto put = [&](int r, float x, float y, double dir, Rect q) {
                rp[2 * r] = x; rp[2 * r + 1] = y; rd[r] = dir; rr[4 * r] = q.x; rr[4 * r + 1] = q.y; rr[4 * r + 2] = q.w; rr[4 * r + 3] = q.h;
            };
            put(0, lpx, lpy, ldir, S.lrect);
            put(1, fpx, fpy, fdir, rect_at(fpx, fpy, A.follower_w_img, A.follower_h_img));
            for (int b = 0; b < A.n_bears; b++) {
                const float bx = (b % 2 == 0) ? lpx + 150.0f : lpx - 150.0f, by = (b % 2 == 0) ? lpy - 150.0f : lpy + 150.0f;
                put(2 + b, bx, by, 0.0, rect_at(bx, by, A.bear_w_img, A.bear_h_img));
            }
            if (rl > A.route_cap) st |= FTL_SCEN_ROUTE_OVERFLOW;
            int n = (int)(euclid_f32(fpx, fpy, lpx, lpy) / (A.trajectory_saving_period * A.leader_max_speed));
            if (n < 0) n = 0;
            if (n > A.init_traj_cap) { st |= FTL_SCEN_TRAJ_OVERFLOW; n = A.init_traj_cap; }
            if (!ok) st = FTL_SCEN_REF_RAISES;
            if (S.limit || rnd.limit) st = FTL_SCEN_GEN_LIMIT;
            A.status[idx] = (uint8_t)st;
            const_cast<int32_t*>(A.out.route_len)[idx] = rl < A.route_cap ? rl : A.route_cap;
            const_cast<int32_t*>(A.out.init_traj_len)[idx] = n;
            S.fpx = fpx; S.fpy = fpy; S.n_traj = n;
        }
        __syncthreads();
        // ---- zero padding, static rects, initial leader_factual_trajectory (float32 linspace follower -> leader)
        {
            const int rn = rl < A.route_cap ? rl : A.route_cap;
            for (int i = rn + lane; i < A.route_cap; i += 64) { ro[2 * i] = 0; ro[2 * i + 1] = 0; }
            int32_t* srect = const_cast<int32_t*>(A.out.static_rects) + (size_t)idx * A.n_static * 4;
            for (int s = lane; s < A.n_static; s += 64) {
                const Rect r = s < S.nobjs ? objs[s].r : Rect{0, 0, 0, 0};
                srect[4 * s] = r.x; srect[4 * s + 1] = r.y; srect[4 * s + 2] = r.w; srect[4 * s + 3] = r.h;
            }
            float* it = const_cast<float*>(A.out.init_traj) + (size_t)idx * A.init_traj_cap * 2;
            const int n = S.n_traj;
            const float fpx = S.fpx, fpy = S.fpy;
            if (n == 1) { if (lane == 0) { it[0] = fpx; it[1] = fpy; } }
            else if (n > 1) {
                const float div = (float)(n - 1);
                const float dxx = lpx - fpx, dyy = lpy - fpy;
                const float stepx = dxx / div, stepy = dyy / div;
                for (int i = lane; i < n - 1; i += 64) {
                    it[2 * i] = (stepx == 0) ? ((float)i / div) * dxx + fpx : (float)i * stepx + fpx;
                    it[2 * i + 1] = (stepy == 0) ? ((float)i / div) * dyy + fpy : (float)i * stepy + fpy;
                }
                if (lane == 0) { it[2 * (n - 1)] = lpx; it[2 * (n - 1) + 1] = lpy; }
            }
            for (int i = n + lane; i < A.init_traj_cap; i += 64) { it[2 * i] = 0; it[2 * i + 1] = 0; }
        }
        __syncthreads();
    }
}

// the workspace: [fixed route (planner 2)] [one slice per wavefront: h f64, tag u32, open list + ranks 2 x i32, bucket i32 per cell]
inline size_t ws_per_wave(int N2) { return ((size_t)N2 * (8 + 4 + 8 + 4) + 255) & ~(size_t)255; }
inline size_t ws_head(int fixed_len) { return ((size_t)(fixed_len > 0 ? fixed_len : 0) * 16 + 255) & ~(size_t)255; }
inline int n_waves(int n) { return n < FTL_SG_MAX_WAVES ? (n > 0 ? n : 1) : FTL_SG_MAX_WAVES; }

int check_args(const ftl_config* cfg, const ftl_scen_params* sp, int32_t n, FtlSgArgs& A) {
    if (!cfg || !sp) return fail(FTL_E_INVALID, "null argument");
    if (sp->planner == 1) return fail(FTL_E_UNSUPPORTED, "the astar planner (CPython heapq order) has no device generator: use ftl_generate_scenarios");
    if (n < 0) return fail(FTL_E_INVALID, "n < 0");
    if (sp->step_grid <= 0 || sp->width <= 0 || sp->height <= 0 || sp->trajectory_saving_period <= 0 || !(sp->leader_max_speed > 0))
        return fail(FTL_E_INVALID, "scenario parameters out of range");
    if (cfg->n_static != (sp->add_obstacles ? sp->obstacle_number + 2 : 0)) return fail(FTL_E_INVALID, "n_static does not match the obstacles");
    if (cfg->n_bears != (sp->add_bear ? sp->bear_number : 0)) return fail(FTL_E_INVALID, "n_bears does not match the bears");
    if (sp->planner < 0 || sp->planner > 2 || (sp->planner == 2 && (sp->fixed_route_len < 0 || (sp->fixed_route_len > 0 && !sp->fixed_route))))
        return fail(FTL_E_INVALID, "bad planner / fixed route");
    if (cfg->route_cap <= 0 || cfg->init_traj_cap <= 0 || cfg->n_bears < 0 || cfg->n_static < 0) return fail(FTL_E_INVALID, "bad capacities");
    const int rows = sp->width / sp->step_grid, cols = sp->height / sp->step_grid;
    const long long N2 = (long long)(rows + 2) * (cols + 2);
    if (N2 > FTL_SG_MAX_CELLS) return fail(FTL_E_UNSUPPORTED, "D* grid larger than 65536 cells");
    if (cfg->n_static > 1024) return fail(FTL_E_UNSUPPORTED, "more than 1022 rocks");
    A = FtlSgArgs{};
    A.width = sp->width; A.height = sp->height; A.step_grid = sp->step_grid; A.obstacle_number = sp->obstacle_number;
    A.add_obstacles = sp->add_obstacles; A.multiple_end_points = sp->multiple_end_points; A.path_finding_iterations = sp->path_finding_iterations;
    A.bridge_gap = sp->bridge_gap; A.bridge_width = sp->bridge_width; A.trajectory_saving_period = sp->trajectory_saving_period;
    A.planner = sp->planner; A.fixed_route_len = sp->planner == 2 ? sp->fixed_route_len : 0;
    A.min_distance = sp->min_distance; A.max_distance = sp->max_distance; A.leader_pos_epsilon = sp->leader_pos_epsilon;
    A.leader_margin = sp->leader_margin; A.leader_w = sp->leader_w; A.leader_h = sp->leader_h; A.leader_max_speed = sp->leader_max_speed;
    A.n_static = cfg->n_static; A.n_bears = cfg->n_bears; A.route_cap = cfg->route_cap; A.init_traj_cap = cfg->init_traj_cap;
    A.leader_w_img = cfg->leader.img_w; A.leader_h_img = cfg->leader.img_h; A.follower_w_img = cfg->follower.img_w;
    A.follower_h_img = cfg->follower.img_h; A.bear_w_img = cfg->bear.img_w; A.bear_h_img = cfg->bear.img_h;
    A.rows = rows; A.cols = cols; A.W2 = cols + 2; A.N2 = (int)N2; A.nwords = (int)((N2 + 31) / 32);
    A.n = n;
    return FTL_OK;
}

inline size_t lds_bytes(const FtlSgArgs& A) { return (624 + 2 * (size_t)A.nwords) * 4 + (size_t)A.n_static * sizeof(Obj); }

}  // namespace ftl_sg

extern "C" {

int ftl_generate_scenarios_device_workspace(const ftl_config* cfg, const ftl_scen_params* sp, int32_t n, size_t* workspace_bytes) {
    if (!workspace_bytes) return fail(FTL_E_INVALID, "null argument");
    FtlSgArgs A;
    const int rc = ftl_sg::check_args(cfg, sp, n, A);
    if (rc) return rc;
    *workspace_bytes = ftl_sg::ws_head(A.fixed_route_len) + (size_t)ftl_sg::n_waves(n) * ftl_sg::ws_per_wave(A.N2);
    return FTL_OK;
}

int ftl_generate_scenarios_device(const ftl_config* cfg, const ftl_scen_params* sp, const int64_t* dev_seeds, int32_t n,
                                  const ftl_scenarios* dev_out, uint8_t* dev_status, void* workspace, size_t workspace_bytes, void* stream) {
    FtlSgArgs A;
    const int rc = ftl_sg::check_args(cfg, sp, n, A);
    if (rc) return rc;
    if (!dev_out || (n > 0 && (!dev_seeds || !dev_status || !workspace))) return fail(FTL_E_INVALID, "null argument");
    if (n > 0 && (!dev_out->static_rects || !dev_out->robot_pos || !dev_out->robot_dir || !dev_out->robot_rect || !dev_out->route ||
                  !dev_out->route_len || !dev_out->init_traj || !dev_out->init_traj_len))
        return fail(FTL_E_INVALID, "null output array");
    const size_t head = ftl_sg::ws_head(A.fixed_route_len), per = ftl_sg::ws_per_wave(A.N2);
    const int waves = ftl_sg::n_waves(n);
    if (workspace_bytes < head + (size_t)waves * per) return fail(FTL_E_INVALID, "workspace smaller than ftl_generate_scenarios_device_workspace");
    if (n == 0) return FTL_OK;
    hipError_t e;
    if (A.fixed_route_len > 0) {
        e = hipMemcpyAsync(workspace, sp->fixed_route, (size_t)A.fixed_route_len * 16, hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMemcpyAsync(fixed route): ") + hipGetErrorString(e));
    }
    A.fixed_route = (const double*)workspace;
    A.seeds = dev_seeds; A.out = *dev_out; A.status = dev_status;
    A.ws = (char*)workspace + head; A.ws_per_wave = per;
    hipLaunchKernelGGL(ftl_sg::ftl_scenario_gen_kernel, dim3((unsigned)waves), dim3(64), ftl_sg::lds_bytes(A), (hipStream_t)stream, A);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
    return FTL_OK;
}

}  // extern "C"
