// ftl_scenario_dev.hpp -- ftl_generate_scenarios_device: the host generator of ftl_scenario.cpp (generate_one) as a gfx950 kernel that
// writes scenarios straight into device memory (include/ftl.h).  Included at the end of ftl_abi.hip (same translation
// unit: it shares fail() / ftl_last_error()).
//
// One wavefront per scenario, persistent: a fixed number of wavefronts loop over the seeds, each with its own slice of the caller's
// workspace (so the scratch does not grow with n).  The `random`-driven parts (MT19937 seeding, robots, bridge walls, rocks, finish points,
// the follower's second draw) are a short sequential program, ftl_scenario_core.hpp, the very code generate_one runs: lane 0 runs it on an
// LDS copy of the MT state with DevicePolicy, the lanes share its element-wise output formulas.  This file holds the planner (nine tenths
// of a scenario on the host), which is wave-parallel, and the kernel skeleton around it:
//
//   plan_route pops the open list bucket by unit-wide bucket; every move costs >= 1, so a relaxation from bucket i lands in a LATER bucket,
//   bucket i is complete when it comes up, and within it the host's stable sort pops in the order (h, global pop index of the node that
//   set h, neighbour index d).  Here a bucket is every open node with h < floor(min h) + 1, popped all at once: each gets its rank in that
//   order (pop index = pops so far + rank), then its neighbours are relaxed in two phases -- a 64-bit atomic minimum over the bit pattern
//   of h (all h >= 0, so the bits order like the doubles), then, among the relaxations that reached the final h of a node lowered in this
//   bucket, an atomic minimum over the tag pop_index * 8 + d.  The winner of the tag is the host's parent (nid - doff[d]).  Nodes popped
//   after the start in its own bucket do not relax (the host stops at the start).  Keys have no bound but the grid's: the host's bucket
//   array grows with them (routes around dense rocks cost far more than rows + cols), here a bucket is a range of h whatever its
//   index, and the tag fits 32 bits as long as pops * 8 does (N2 <= FTL_SG_MAX_CELLS = 65536).
//
// Every loop is bounded: the rejection samplers (rocks, finish points) and randbelow stop after FTL_SG_MAX_ATTEMPTS draws (DevicePolicy) and
// mark the scenario FTL_SCEN_GEN_LIMIT (unusable; the host never gets there on a real seed), a bucket closes at least one node, the parent
// walk stops at max_iterat or after every cell.
// Numerics: the same double / float operation sequence as the host (-ffp-contract=off); DevicePolicy's atan (leader / follower directions)
// and cos / sin (the follower's placement) are the correctly rounded ones of ftl_crmath.hpp, not the device math library's (which differs
// from glibc by an ulp often enough to change the start direction of 2-12 % of the worlds).
#pragma once
#include "ftl_scenario_core.hpp"

#define FTL_SG_MAX_WAVES 2048           // persistent wavefronts (8 per CU on 256 CUs): the workspace holds one slice per wavefront
#define FTL_SG_MAX_CELLS 65536          // (rows + 2) * (cols + 2) of the D* grid: node ids and pop indices fit the 32-bit tag

struct FtlSgArgs {                      // the launch (the scenario parameters travel beside it as ftl_sc::Params)
    int32_t rows, cols, W2, N2, nwords; // the D* grid
    const int64_t* seeds; int32_t n;
    ftl_scenarios out; uint8_t* status;
    char* ws; size_t ws_per_wave;
};

namespace ftl_sg {

using namespace ftl_sc;

// what lane 0 hands to the wave between the sequential parts
struct Shared {
    Start start;                      // ftl_sc::before_planner
    int rl, fail;
    double r1x, r1y;                  // route[1] (the leader's first target point)
    // D*
    int m_open, start_rank;
    Linspace traj;                    // ftl_sc::after_planner
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
__device__ bool plan_route_wave(const Params& P, const FtlSgArgs& A, Shared& S, const uint32_t* obst, uint32_t* closed, int sx, int sy, int gx, int gy,
                                int max_iterat, double* hh, uint32_t* tag, int* open, int* front, double* route_out) {
    const int lane = threadIdx.x;
    const int rows = A.rows, cols = A.cols, W2 = A.W2, N2 = A.N2;
    auto in = [&](int x, int y) { return x >= 0 && x < rows && y >= 0 && y < cols; };
    if (!in(sx, sy) || !in(gx, gy)) return false;
    if (sx == gx && sy == gy) return true;
    const int goal = (gx + 1) * W2 + gy + 1, start = (sx + 1) * W2 + sy + 1;
    if (bit(obst, goal) || bit(obst, start)) return false;
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
            const double x = (double)((int64_t)(cur / W2 - 1) * P.sp.step_grid), y = (double)((int64_t)(cur % W2 - 1) * P.sp.step_grid);
            if (k < P.route_cap) { route_out[2 * k] = x; route_out[2 * k + 1] = y; }
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

__global__ void __launch_bounds__(64) ftl_scenario_gen_kernel(const Params P, const FtlSgArgs A) {
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
    const ftl_scen_params& sp = P.sp;
    const int sg = sp.step_grid;
    for (int idx = blockIdx.x; idx < A.n; idx += gridDim.x) {
        double* ro = const_cast<double*>(A.out.route) + (size_t)idx * P.route_cap * 2;
        // ---- the sequential part up to the planner (the MT state stays in LDS for the follower's second draw)
        if (lane == 0) {
            before_planner<DevicePolicy>(P, A.seeds[idx], mt, objs, S.start);
            S.rl = 0; S.r1x = 0; S.r1y = 0;
        }
        __syncthreads();
        const bool ok0 = S.start.ok && !S.start.limit;
        bool found = true;
        if (ok0 && sp.planner == 2 && lane == 0) {
            for (int i = 0; i < sp.fixed_route_len; i++) {
                if (i < P.route_cap) { ro[2 * i] = sp.fixed_route[2 * i]; ro[2 * i + 1] = sp.fixed_route[2 * i + 1]; }
            }
            if (sp.fixed_route_len >= 2) { S.r1x = sp.fixed_route[2]; S.r1y = sp.fixed_route[3]; }
            S.rl = sp.fixed_route_len;
        }
        if (ok0 && sp.planner == 0) {
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
            const int margin = (int)floor(sp.leader_margin * fmax(sp.leader_w, sp.leader_h) / sg);
            for (int o = lane; o < S.start.nobjs; o += 64) {
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
            int sx = (int)(S.start.lpx / (float)sg), sy = (int)(S.start.lpy / (float)sg);
            const int runs = sp.multiple_end_points ? 3 : 1;
            for (int k = 0; k < runs; k++) {
                const int gx = (int)((double)S.start.fx[k] / sg), gy = (int)((double)S.start.fy[k] / sg);
                const bool f = plan_route_wave(P, A, S, obst, closed, sx, sy, gx, gy, k == 0 ? sp.path_finding_iterations : 15000,
                                               hh, tag, open, front, ro);
                found = found && f;
                sx = gx; sy = gy;
            }
            __syncthreads();
        }
        // ---- leader direction, the follower behind the leader, robots, status, lengths
        const int rl = S.rl;
        if (lane == 0) after_planner<DevicePolicy>(P, S.start, mt, found, rl, S.r1x, S.r1y, A.out, A.status, idx, S.traj);
        __syncthreads();
        // ---- zero padding, static rects, initial leader_factual_trajectory
        const int rn = rl < P.route_cap ? rl : P.route_cap;
        for (int i = rn + lane; i < P.route_cap; i += 64) route_pad(ro, i);
        int32_t* srect = const_cast<int32_t*>(A.out.static_rects) + (size_t)idx * P.n_static * 4;
        for (int s = lane; s < P.n_static; s += 64) static_rect_row(objs, S.start.nobjs, srect, s);
        float* it = const_cast<float*>(A.out.init_traj) + (size_t)idx * P.init_traj_cap * 2;
        for (int i = lane; i < P.init_traj_cap; i += 64) traj_point(S.traj, it, i);
        __syncthreads();
    }
}

// the workspace: [fixed route (planner 2)] [one slice per wavefront: h f64, tag u32, open list + ranks 2 x i32, bucket i32 per cell]
inline size_t ws_per_wave(int N2) { return ((size_t)N2 * (8 + 4 + 8 + 4) + 255) & ~(size_t)255; }
inline size_t ws_head(int fixed_len) { return ((size_t)(fixed_len > 0 ? fixed_len : 0) * 16 + 255) & ~(size_t)255; }
inline int n_waves(int n) { return n < FTL_SG_MAX_WAVES ? (n > 0 ? n : 1) : FTL_SG_MAX_WAVES; }

// the shared argument check, then the device generator's own limits; fills the launch's grid sizes
int check_args(const ftl_config* cfg, const ftl_scen_params* sp, int32_t n, FtlSgArgs& A) {
    if (cfg && sp && sp->planner == 1) return fail(FTL_E_UNSUPPORTED, "the astar planner (CPython heapq order) has no device generator: use ftl_generate_scenarios");
    if (const char* why = ftl_sc::check_args(cfg, sp, n)) return fail(FTL_E_INVALID, why);
    if (cfg->route_cap <= 0 || cfg->init_traj_cap <= 0 || cfg->n_bears < 0 || cfg->n_static < 0) return fail(FTL_E_INVALID, "bad capacities");
    const int rows = sp->width / sp->step_grid, cols = sp->height / sp->step_grid;
    const long long N2 = (long long)(rows + 2) * (cols + 2);
    if (N2 > FTL_SG_MAX_CELLS) return fail(FTL_E_UNSUPPORTED, "D* grid larger than 65536 cells");
    if (cfg->n_static > 1024) return fail(FTL_E_UNSUPPORTED, "more than 1022 rocks");
    A = FtlSgArgs{};
    A.rows = rows; A.cols = cols; A.W2 = cols + 2; A.N2 = (int)N2; A.nwords = (int)((N2 + 31) / 32);
    A.n = n;
    return FTL_OK;
}

inline size_t lds_bytes(const FtlSgArgs& A, int n_static) { return (624 + 2 * (size_t)A.nwords) * 4 + (size_t)n_static * sizeof(Obj); }

}  // namespace ftl_sg

extern "C" {

int ftl_generate_scenarios_device_workspace(const ftl_config* cfg, const ftl_scen_params* sp, int32_t n, size_t* workspace_bytes) {
    if (!workspace_bytes) return fail(FTL_E_INVALID, "null argument");
    FtlSgArgs A;
    const int rc = ftl_sg::check_args(cfg, sp, n, A);
    if (rc) return rc;
    *workspace_bytes = ftl_sg::ws_head(ftl_sc::make_params(*cfg, *sp).sp.fixed_route_len) + (size_t)ftl_sg::n_waves(n) * ftl_sg::ws_per_wave(A.N2);
    return FTL_OK;
}

int ftl_generate_scenarios_device(const ftl_config* cfg, const ftl_scen_params* sp, const int64_t* dev_seeds, int32_t n,
                                  const ftl_scenarios* dev_out, uint8_t* dev_status, void* workspace, size_t workspace_bytes, void* stream) {
    FtlSgArgs A;
    const int rc = ftl_sg::check_args(cfg, sp, n, A);
    if (rc) return rc;
    if (!dev_out || (n > 0 && (!dev_seeds || !dev_status || !workspace))) return fail(FTL_E_INVALID, "null argument");
    if (n > 0 && !ftl_sc::has_every_array(*dev_out)) return fail(FTL_E_INVALID, "null output array");
    ftl_sc::Params P = ftl_sc::make_params(*cfg, *sp);
    const size_t head = ftl_sg::ws_head(P.sp.fixed_route_len), per = ftl_sg::ws_per_wave(A.N2);
    const int waves = ftl_sg::n_waves(n);
    if (workspace_bytes < head + (size_t)waves * per) return fail(FTL_E_INVALID, "workspace smaller than ftl_generate_scenarios_device_workspace");
    if (n == 0) return FTL_OK;
    if (P.sp.fixed_route_len > 0) {
        hipError_t e = hipMemcpyAsync(workspace, sp->fixed_route, (size_t)P.sp.fixed_route_len * 16, hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMemcpyAsync(fixed route): ") + hipGetErrorString(e));
    }
    P.sp.fixed_route = (const double*)workspace;                 // the kernel reads the device copy
    A.seeds = dev_seeds; A.out = *dev_out; A.status = dev_status;
    A.ws = (char*)workspace + head; A.ws_per_wave = per;
    hipLaunchKernelGGL(ftl_sg::ftl_scenario_gen_kernel, dim3((unsigned)waves), dim3(64), ftl_sg::lds_bytes(A, P.n_static), (hipStream_t)stream, P, A);
    return launched();
}

}  // extern "C"
