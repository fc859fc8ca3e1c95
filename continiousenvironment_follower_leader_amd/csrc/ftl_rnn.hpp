// ftl_rnn.hpp -- a recurrent policy, or a population of them, on the device: a trunk of dense ReLU layers, one LSTM cell and a linear
// head (include/ftl.h, the ftl_rnn_act block, is the contract).  One decision of every env with its state update (ftl_rnn_act), T
// closed-loop steps (ftl_rollout_rnn), a recorded trajectory (ftl_collect_rnn), and the net put back over a recorded sequence in one
// launch (ftl_rnn_forward, ftl_rnn_forward_kernel: further down, with its own comment).  Included by ftl_abi.hip after ftl_collect.hpp (same
// translation unit: it reads the handle, uses the head maps of ftl_mlp.hpp and the record kernel of ftl_collect.hpp, and hands its
// kernel to rollout_loop, which owns the steps; there is no second loop here).  The host side shares with ftl_mlp.hpp the tile map
// (tile_map), the width and set checks, and the closed-loop rollout of a policy (policy_rollout), with ftl_collect.hpp the one collect
// (collect_loop); RnnSeq holds what ftl_rnn_forward and ftl_rnn_backward check and fill alike.
//
// ftl_rnn_kernel keeps the plan of ftl_mlp_kernel: one workgroup of 256 threads per tile of up to FTL_MLP_ENV_TILE envs of ONE weight set,
// everything in one launch, activations in LDS between the layers, a layer's weights staged in LDS in k-chunks, the products on
// v_mfma_f32_16x16x4_f32 with the bias as the C operand (the contract's fmaf chain: tests/test_gpu_mlp.py).  The layer loop is a copy of
// mlp_body's (ftl_mlp_kernel and ftl_mlp_sample_kernel keep their code and their resource rows) with two generalisations: input and
// output are separate LDS arrays, and the staged columns of the gate layer go through a column map.
//   trunk   layers 0 .. Lt-1 as in ftl_mlp_kernel; the last one writes x into the first width[Lt] columns of u.
//   gather  u[e] = [x | a_prev | r_prev | h]: the rest of the row comes from the env's state row and out->reward (all zeros where mode
//           BEFORE reads a finished env as fresh); the same threads store h | a_prev | live to state_rec.
//   gates   a dense layer over u in passes of at most 64 cells: a pass computes the columns {q * C + j0 + jj}, q = 0 .. 3 (i, f, g, o), of
//           the torch-ordered W_g -- at most 256, what a tile's accumulators hold.  The column map (gate_col) gives the four gates of a
//           cell to the four accumulators acc[4 * gs + q] of ONE lane, so z never leaves the registers: the lane that holds z of (4 envs,
//           2 cells) reads their c from HBM, runs the cell lines (ftl_rnn_math.hpp), writes h' to an LDS array of its own -- later
//           passes still read the old h in u -- and c', h' to the state row (zeros in mode AFTER at an env that was done on entry).
//           Nothing reads h or c from HBM after the gather / its own lane, so the row is updated in place.
//   head    a dense layer h' -> y, then one thread per env: the head map of ftl_mlp_sample, a_prev' and live.
// LDS is sized from the actual widths (rnn_lds_bytes): 61.25 KiB for 180-64-64, C = 64 (two workgroups a CU), and at the limits (widths
// 256, C = 128, head 5) 125.25 KiB of the 160 KiB a workgroup may have.
#include <hip/hip_runtime.h>
#include "ftl_rnn_math.hpp"

#define FTL_RNN_PASS_CELLS 64          // cells of one gate pass: 4 * 64 = FTL_MLP_MAX_WIDTH columns

namespace ftlrnn {

using ftlmlp::f32x4;
using ftlmlp::TILE; using ftlmlp::KC; using ftlmlp::EPW; using ftlmlp::NB; using ftlmlp::GROUPS; using ftlmlp::PARITIES; using ftlmlp::BPW; using ftlmlp::XS;
static_assert(4 * FTL_RNN_PASS_CELLS == FTL_MLP_MAX_WIDTH && FTL_RNN_MAX_CELL % FTL_RNN_PASS_CELLS == 0, "a gate pass fills a tile's accumulators");

struct Args {
    ftlmlp::Args m;            // the trunk as ftl_mlp_kernel's arguments: n_layers = Lt, width[0 .. Lt]; head, bounds, action, the tile map
    int32_t cell, P, R, A;     // C; widths of a_prev and r_prev in u; the head width
    int32_t u_stride, h_stride;                // floats per env row of u and h' in LDS (each % 32 == 2)
    float* state; int64_t state_stride;
    float* state_rec;          // [n_envs][S] or null
    const double* reward; const uint8_t* out_done;
    const uint8_t* alive;      // mode AFTER inside a loop: the rollout scratch; null: the state's done word
    const int32_t* env_int; int32_t rec_stride;
    int32_t before;            // 1: mode BEFORE
};

// The staged columns of a gate pass.  A wave of parity p owns the column blocks jb = p + PARITIES * m, m < BPW = 8; in a gate pass block
// (p, m) holds gate q = m & 3 of the 16 cells of group G = 2 * (m >> 2) + p, so the lane that holds accumulator rows of cell G * 16 + li
// holds all four gates of that cell (acc[4 * (m >> 2) + q]) and the cell lines run in registers.  cn <= 64 cells of the pass are real;
// a column of a cell past cn is staged from the pass's last cell and never used.
struct Gates { int cn, C, j0; };
constexpr int NLD = 16;                  // weights of a chunk a thread has in flight from L2 at a time: a 4,096-float chunk in one go
__device__ __forceinline__ int gate_group(int par, int m) { return 2 * (m >> 2) + par; }
__device__ __forceinline__ int gate_col(const Gates& gm, int c) {
    const int jb = c >> 4, m = jb >> 1, jj = gate_group(jb & 1, m) * NB + (c & 15);
    return (m & 3) * gm.C + gm.j0 + (jj < gm.cn ? jj : gm.cn - 1);
}
static_assert(PARITIES == 2 && BPW == 8 && NB == 16 && FTL_RNN_PASS_CELLS == 4 * NB, "the gate map");

// The accumulators of one dense layer of a tile: acc of column j = chain over k of x[e][k] * W[k][col(j)] from bias[col(j)].
// GATES false: col(j) = j, j < w_out, W is [w_in][w_out].  GATES true: col = gate_col, w_out is the staged width (128 for up to 32 cells of
// the pass, else 256), W is W_g with rows of ldw floats.  obs != null: x is read from HBM (the policy_obs rows, staged in xs chunk by chunk
// and copied to obs_rec); else from xin in LDS.
template <bool GATES>
__device__ __forceinline__ void layer_acc(f32x4 (&acc)[BPW], const float* W, int ldw, const float* bias, const Gates gm, int w_in, int w_out,
                                          const float* obs, float* obs_rec, int start, int tile_n,
                                          const float* xin, int xin_stride, float* xs, float* ws) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int g = wave % GROUPS, par = wave / GROUPS;
    const int row_a = g * EPW + li, row_d = g * EPW + 4 * lk;
    const bool busy = g * EPW < tile_n;
    const int nblk = (w_out + NB - 1) / NB;
    bool on[BPW];                                               // (wave-uniform) the block holds columns somebody reads
#pragma unroll
    for (int m = 0; m < BPW; m++) {
        const int jb = par + PARITIES * m, j = jb * NB + li;
        on[m] = GATES ? gate_group(par, m) * NB < gm.cn : jb < nblk;
        const float b = !on[m] ? 0.0f : GATES ? bias[gate_col(gm, j)] : j < w_out ? bias[j] : 0.0f;
        acc[m] = f32x4{b, b, b, b};
    }
    const int kc = ftlmlp::chunk_rows(w_out);
    const int xstride = obs ? XS : xin_stride;
    for (int k0 = 0; k0 < w_in; k0 += kc) {
        const int kn = w_in - k0 < kc ? w_in - k0 : kc;
        __syncthreads();                                        // the chunk before this one has been read (and, k0 == 0, the input written)
        // (NLD loads are issued before the first is stored, so a thread waits for L2 once per NLD floats, not once per float)
        const int sh = w_out == 128 ? 7 : 8;
        for (int base = t; base < kn * w_out; base += NLD * FTL_MLP_THREADS) {
            float v[NLD];
#pragma unroll
            for (int i = 0; i < NLD; i++) {
                const int idx = base + i * FTL_MLP_THREADS, ok = idx < kn * w_out, at = ok ? idx : base;
                v[i] = GATES ? W[(size_t)(k0 + (at >> sh)) * ldw + gate_col(gm, at & (w_out - 1))] : W[(size_t)k0 * w_out + at];
            }
#pragma unroll
            for (int i = 0; i < NLD; i++) {
                const int idx = base + i * FTL_MLP_THREADS;
                if (idx < kn * w_out) ws[idx] = v[i];
            }
        }
        if (obs) {
            const int e = t >> 3;                               // 8 threads per env of the tile
            if (e < tile_n) {
                const size_t row = (size_t)(start + e) * w_in + k0;
                if (obs_rec)
                    for (int kk = t & 7; kk < kn; kk += 8) { const float v = obs[row + kk]; xs[e * XS + kk] = v; obs_rec[row + kk] = v; }
                else
                    for (int kk = t & 7; kk < kn; kk += 8) xs[e * XS + kk] = obs[row + kk];
            }
        }
        __syncthreads();
        if (!busy) continue;
        const float* x = obs ? xs : xin + k0;
        const float* xa = x + row_a * xstride + lk;
        const float* xd = x + row_d * xstride;
        int kk = 0;
        for (; kk + 4 <= kn; kk += 4) {
            const float av = xa[kk];
            const float* wrow = ws + (kk + lk) * w_out + li;    // columns past w_out read on into the stage
#pragma unroll
            for (int m = 0; m < BPW; m++)
                if (on[m]) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wrow[(par + PARITIES * m) * NB], acc[m], 0, 0, 0);
        }
        for (; kk < kn; kk++) {                                  // w_in % 4 rows at the layer's end
#pragma unroll
            for (int m = 0; m < BPW; m++) {
                if (!on[m]) continue;
                const float w = ws[kk * w_out + (par + PARITIES * m) * NB + li];
#pragma unroll
                for (int r = 0; r < 4; r++) acc[m][r] = __builtin_fmaf(xd[r * xstride + kk], w, acc[m][r]);
            }
        }
    }
}

// One dense layer of a tile into LDS: y[e][j], j < w_out; relu as in ftl_mlp_kernel.  yout may be xin.
__device__ __forceinline__ void dense(const float* W, const float* bias, int w_in, int w_out, const float* obs, float* obs_rec, int start, int tile_n,
                                      const float* xin, int xin_stride, float* yout, int y_stride, bool relu, float* xs, float* ws) {
    f32x4 acc[BPW];
    layer_acc<false>(acc, W, w_out, bias, Gates{0, 0, 0}, w_in, w_out, obs, obs_rec, start, tile_n, xin, xin_stride, xs, ws);
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int row_d = (wave % GROUPS) * EPW + 4 * lk, par = wave / GROUPS;
    __syncthreads();                                            // every wave has read this layer's input
#pragma unroll
    for (int m = 0; m < BPW; m++) {
        const int j = (par + PARITIES * m) * NB + li;
        if (j >= w_out) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float v = acc[m][r];
            yout[(row_d + r) * y_stride + j] = relu ? (v > 0.0f ? v : 0.0f) : v;
        }
    }
}

__global__ __launch_bounds__(FTL_MLP_THREADS) void ftl_rnn_kernel(const Args a, const ftlmlp::Sample sm) {
    extern __shared__ float4 rnn_lds[];
    const ftlmlp::Args& m = a.m;
    float* act = reinterpret_cast<float*>(rnn_lds);             // [TILE][act_stride]: the trunk between its layers, then y
    float* u = act + TILE * m.act_stride;                       // [TILE][u_stride]
    float* hn = u + TILE * a.u_stride;                          // [TILE][h_stride]: h'
    float* xs = hn + TILE * a.h_stride;                         // [TILE][XS]
    float* ws = xs + TILE * XS;                                 // the weight stage (+ 64 floats never used)
    const int t = (int)threadIdx.x;
    // the tile's set and envs (as in mlp_body)
    int set = m.env_first / m.envs_per_set, start, end;
    if ((int)blockIdx.x < m.tiles0) { start = (int)blockIdx.x * TILE; end = m.len0; }
    else {
        const int b = (int)blockIdx.x - m.tiles0, q = b / m.tiles_per_set;
        const int64_t seg = (int64_t)m.len0 + (int64_t)q * m.envs_per_set, seg_end = seg + m.envs_per_set;
        set += 1 + q;
        start = (int)seg + (b % m.tiles_per_set) * TILE;
        end = seg_end < (int64_t)m.n_envs ? (int)seg_end : m.n_envs;
    }
    const int tile_n = end - start < TILE ? end - start : TILE;
    const float* P = m.params + (int64_t)set * m.set_stride;
    const int Lt = m.n_layers, C = a.cell, wx = m.width[Lt], U = wx + a.P + a.R + C, S = 2 * C + a.P + 1;
    for (int l = 0; l < Lt; l++) {
        const int w_in = m.width[l], w_out = m.width[l + 1];
        const bool last = l + 1 == Lt;
        dense(P, P + (size_t)w_in * w_out, w_in, w_out, l == 0 ? m.obs : nullptr, sm.obs_rec, start, tile_n,
              act, m.act_stride, last ? u : act, last ? a.u_stride : m.act_stride, true, xs, ws);
        P += ((size_t)w_in + 1) * w_out;
    }
    // gather the rest of u; the env's "read as fresh" and "write zeros" predicates
    const int tail = a.P + a.R + C;
    for (int idx = t; idx < tile_n * tail; idx += FTL_MLP_THREADS) {
        const int e = idx / tail, k = idx - e * tail;
        const size_t env = (size_t)start + e;
        const bool fresh = a.before && a.out_done[env] != 0;
        const float* row = a.state + env * a.state_stride;
        float* rec = a.state_rec ? a.state_rec + env * S : nullptr;
        float v;
        if (k < a.P) {
            v = fresh ? 0.0f : row[2 * C + k];
            if (rec) rec[2 * C + k] = v;
        } else if (k < a.P + a.R) {
            const float live = fresh ? 0.0f : row[2 * C + a.P];
            v = live != 0.0f ? (float)a.reward[env] : 0.0f;
        } else {
            const int j = k - a.P - a.R;
            v = fresh ? 0.0f : row[j];
            if (rec) rec[j] = v;
        }
        u[e * a.u_stride + wx + k] = v;
    }
    if (a.state_rec && t < tile_n) {
        const size_t env = (size_t)start + t;
        const bool fresh = a.before && a.out_done[env] != 0;
        a.state_rec[env * S + 2 * C + a.P] = fresh ? 0.0f : a.state[env * a.state_stride + 2 * C + a.P];
    }
    // (layer_acc() begins with a barrier: u is complete before any wave reads it)
    const float* Wg = P;
    const float* bg = Wg + (size_t)U * 4 * C;
    const int lane = t & 63, wave = t >> 6, li = lane & 15, row_d = (wave % GROUPS) * EPW + 4 * (lane >> 4), par = wave / GROUPS;
    for (int j0 = 0; j0 < C; j0 += FTL_RNN_PASS_CELLS) {
        const int cn = C - j0 < FTL_RNN_PASS_CELLS ? C - j0 : FTL_RNN_PASS_CELLS;
        f32x4 z[BPW];
        layer_acc<true>(z, Wg, 4 * C, bg, Gates{cn, C, j0}, U, cn <= 2 * NB ? 128 : 256, nullptr, nullptr, start, tile_n, u, a.u_stride, xs, ws);
#pragma unroll
        for (int gs = 0; gs < 2; gs++) {                            // the lane's two cells of the pass, four envs each
            const int jj = gate_group(par, 4 * gs) * NB + li, j = j0 + jj;
            if (jj >= cn) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int e = row_d + r;
                if (e >= tile_n) continue;
                const size_t env = (size_t)start + e;
                const bool done_in = a.alive ? a.alive[env] == 0
                                   : reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(a.env_int) + env * (size_t)a.rec_stride)[FTL_EI_DONE] != 0;
                const bool fresh = a.before && a.out_done[env] != 0, wipe = !a.before && done_in;
                float* row = a.state + env * a.state_stride;
                const float c = fresh ? 0.0f : row[C + j];
                if (a.state_rec) a.state_rec[env * S + C + j] = c;
                const float gi = ftlrnnmath::sig32(z[4 * gs][r]);
                const float gf = ftlrnnmath::sig32(z[4 * gs + 1][r]);
                const float gg = ftlrnnmath::tanh32(z[4 * gs + 2][r]);
                const float go = ftlrnnmath::sig32(z[4 * gs + 3][r]);
                const float tt = gi * gg;
                const float cn1 = __builtin_fmaf(gf, c, tt);
                const float th = ftlrnnmath::tanh32(cn1);
                const float hn1 = go * th;
                hn[e * a.h_stride + j] = hn1;                       // (an array of its own: later passes still read the old h in u)
                row[j] = wipe ? 0.0f : hn1;
                row[C + j] = wipe ? 0.0f : cn1;
            }
        }
    }
    const float* Wy = bg + 4 * C;
    dense(Wy, Wy + (size_t)C * a.A, C, a.A, nullptr, nullptr, start, tile_n, hn, a.h_stride, act, m.act_stride, false, xs, ws);
    __syncthreads();
    if (t >= tile_n) return;
    const float* y = act + t * m.act_stride;
    const size_t e = (size_t)start + t;
    const int wl = a.A;
    if (sm.head_rec)
        for (int j = 0; j < wl; j++) sm.head_rec[e * wl + j] = y[j];
    float ap[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (m.head == FTL_ACTION_DISCRETE) {
        int k = 0;
        if (sm.noise) {                                         // s_j = y_j + noise_j in float64; the first maximum, a NaN never beats anything
            const float* nz = sm.noise + e * wl;
            double best = (double)y[0] + (double)nz[0];
            for (int j = 1; j < 5; j++) {
                const double sj = (double)y[j] + (double)nz[j];
                if (sj > best) { best = sj; k = j; }
            }
        } else {
            for (int j = 1; j < 5; j++) if (y[j] > y[k]) k = j;
        }
        static_cast<int32_t*>(m.action)[e] = k;
#pragma unroll
        for (int j = 0; j < 5; j++) ap[j] = j == k ? 1.0f : 0.0f;
    } else {
        const float* nz = sm.noise ? sm.noise + e * wl : nullptr;
        const float* sg = sm.noise ? sm.sigma + (size_t)set * wl : nullptr;
        if (m.head == FTL_ACTION_BOX2) {
            const double a0 = nz ? ftlmlp::box_sample(y[0], sg[0], nz[0], m.lo0, m.hi0) : ftlmlp::box_head(y[0], m.lo0, m.hi0);
            const double a1 = nz ? ftlmlp::box_sample(y[1], sg[1], nz[1], m.lo1, m.hi1) : ftlmlp::box_head(y[1], m.lo1, m.hi1);
            static_cast<double*>(m.action)[2 * e] = a0;
            static_cast<double*>(m.action)[2 * e + 1] = a1;
            ap[0] = (float)a0; ap[1] = (float)a1;
        } else {
            const double a1 = nz ? ftlmlp::box_sample(y[0], sg[0], nz[0], m.lo1, m.hi1) : ftlmlp::box_head(y[0], m.lo1, m.hi1);
            static_cast<double*>(m.action)[e] = a1;
            ap[0] = (float)a1;
        }
    }
    const bool done_in = a.alive ? a.alive[e] == 0
                       : reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(a.env_int) + e * (size_t)a.rec_stride)[FTL_EI_DONE] != 0;
    const bool wipe = !a.before && done_in;
    float* row = a.state + e * a.state_stride + 2 * C;
#pragma unroll
    for (int j = 0; j < 5; j++)
        if (j < a.P) row[j] = wipe ? 0.0f : ap[j];
    row[a.P] = wipe ? 0.0f : 1.0f;
}

// ---- ftl_rnn_forward: the net on a recorded sequence (include/ftl.h: ftl_rnn_forward) ----
// ONE launch for all B blocks: the tile map, the LDS plan and the layers (dense, layer_acc, gate_col) of ftl_rnn_kernel, with the block
// loop inside the kernel and the state in the workgroup.  c lives in the registers of the lane that owns the cell -- the gate map gives a
// lane the same (4 rows, 2 cells) in every pass of every block, so C = 128 is two passes x two cells x four rows = 16 floats a lane -- and
// h' goes from its LDS array into the h columns of u after the head layer has read it (behind a barrier; later gate passes of the same
// block still read the old h, as in ftl_rnn_kernel).  The zero rule is applied there from kind[b].  HBM state traffic is the state before
// block 0 (read once) and state_out (written once); head[b] and h[b] leave as contiguous runs from LDS.  The trunk does not depend on the
// state; it runs inside the block loop, so act holds one block's activations as in ftl_rnn_kernel and the LDS plan is unchanged.
struct Seq {
    ftlmlp::Args m;            // the trunk and the tile map over the n rows of a block (n_envs = n); m.obs is block 0 of obs
    int32_t cell, P, R, A;
    int32_t u_stride, h_stride;
    int32_t n_blocks, state_at;
    const float* state; int64_t state_stride;                   // the rows before block 0: read only
    int64_t obs_bb, action_bb, reward_bb, kind_bb, head_bb, h_bb;               // bytes between two blocks
    const void* action; const double* reward; const uint8_t* kind; const double* reward0;
    float* head; float* h; float* state_out;
};

__global__ __launch_bounds__(FTL_MLP_THREADS, 2) void ftl_rnn_forward_kernel(const Seq a) {
    extern __shared__ float4 rnn_fwd_lds[];
    const ftlmlp::Args& m = a.m;
    float* act = reinterpret_cast<float*>(rnn_fwd_lds);         // [TILE][act_stride]: the trunk between its layers, then y
    float* u = act + TILE * m.act_stride;                       // [TILE][u_stride]
    float* hn = u + TILE * a.u_stride;                          // [TILE][h_stride]: h'
    float* xs = hn + TILE * a.h_stride;                         // [TILE][XS]
    float* ws = xs + TILE * XS;                                 // the weight stage (+ 64 floats never used)
    const int t = (int)threadIdx.x;
    // the tile's set and rows (as in ftl_rnn_kernel)
    int set = m.env_first / m.envs_per_set, start, end;
    if ((int)blockIdx.x < m.tiles0) { start = (int)blockIdx.x * TILE; end = m.len0; }
    else {
        const int b = (int)blockIdx.x - m.tiles0, q = b / m.tiles_per_set;
        const int64_t seg = (int64_t)m.len0 + (int64_t)q * m.envs_per_set, seg_end = seg + m.envs_per_set;
        set += 1 + q;
        start = (int)seg + (b % m.tiles_per_set) * TILE;
        end = seg_end < (int64_t)m.n_envs ? (int)seg_end : m.n_envs;
    }
    const int tile_n = end - start < TILE ? end - start : TILE;
    const float* P0 = m.params + (int64_t)set * m.set_stride;
    const int Lt = m.n_layers, C = a.cell, wx = m.width[Lt], U = wx + a.P + a.R + C, S = 2 * C + a.P + 1;
    const float* Wg = P0;
    for (int l = 0; l < Lt; l++) Wg += ((size_t)m.width[l] + 1) * m.width[l + 1];
    const float* bg = Wg + (size_t)U * 4 * C;
    const float* Wy = bg + 4 * C;
    const int tail = a.P + a.R + C;
    const int lane = t & 63, wave = t >> 6, li = lane & 15, row_d = (wave % GROUPS) * EPW + 4 * (lane >> 4), par = wave / GROUPS;
    constexpr int PASSES = FTL_RNN_MAX_CELL / FTL_RNN_PASS_CELLS;
    static_assert(PASSES == 2, "c of a pass is selected between two register sets");
    // the state before block 0: the rest of u, and c into the registers of the lane that owns the cell
    for (int idx = t; idx < tile_n * tail; idx += FTL_MLP_THREADS) {
        const int e = idx / tail, k = idx - e * tail;
        const size_t row_i = (size_t)start + e;
        const float* row = a.state + row_i * a.state_stride;
        float* so = a.state_out && a.state_at == 0 ? a.state_out + row_i * S : nullptr;
        float v;
        if (k < a.P) {
            v = row[2 * C + k];
            if (so) so[2 * C + k] = v;
        } else if (k < a.P + a.R) {
            const float live = row[2 * C + a.P];
            v = live != 0.0f ? (float)(a.reward0 ? a.reward0[row_i] : 0.0) : 0.0f;
        } else {
            const int j = k - a.P - a.R;
            v = row[j];
            if (so) so[j] = v;
        }
        u[e * a.u_stride + wx + k] = v;
    }
    if (a.state_out && a.state_at == 0 && t < tile_n) {
        const size_t row_i = (size_t)start + t;
        a.state_out[row_i * S + 2 * C + a.P] = a.state[row_i * a.state_stride + 2 * C + a.P];
    }
    float c[PASSES][2][4];
#pragma unroll
    for (int ps = 0; ps < PASSES; ps++)
#pragma unroll
        for (int gs = 0; gs < 2; gs++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = ps * FTL_RNN_PASS_CELLS + gate_group(par, 4 * gs) * NB + li, e = row_d + r;
                float v = 0.0f;
                if (j < C && e < tile_n) {
                    const size_t row_i = (size_t)start + e;
                    v = a.state[row_i * a.state_stride + C + j];
                    if (a.state_out && a.state_at == 0) a.state_out[row_i * S + C + j] = v;
                }
                c[ps][gs][r] = v;
            }
    for (int b = 0; b < a.n_blocks; b++) {
        const bool more = b + 1 < a.n_blocks;                   // block b + 1 reads the row this one leaves: kind[b], action[b], reward[b]
        const bool keep = more && a.state_out && a.state_at == b + 1;
        const float* obs = reinterpret_cast<const float*>(reinterpret_cast<const char*>(m.obs) + (int64_t)b * a.obs_bb);
        const uint8_t* kind = more ? a.kind + (int64_t)b * a.kind_bb : nullptr;
        const float* P = P0;
        for (int l = 0; l < Lt; l++) {
            const int w_in = m.width[l], w_out = m.width[l + 1];
            const bool last = l + 1 == Lt;
            dense(P, P + (size_t)w_in * w_out, w_in, w_out, l == 0 ? obs : nullptr, nullptr, start, tile_n,
                  act, m.act_stride, last ? u : act, last ? a.u_stride : m.act_stride, true, xs, ws);
            P += ((size_t)w_in + 1) * w_out;
        }
        bool wipe[4];                                           // the zero rule of the lane's four rows
#pragma unroll
        for (int r = 0; r < 4; r++) wipe[r] = more && row_d + r < tile_n && kind[(size_t)start + row_d + r] == FTL_TR_VOID;
        // (layer_acc() begins with a barrier: u is complete before any wave reads it)
#pragma unroll 1
        for (int ps = 0; ps < PASSES; ps++) {                   // (one copy of the pass's code: c of the pass is selected, not indexed)
            const int j0 = ps * FTL_RNN_PASS_CELLS;
            if (j0 >= C) break;
            const int cn = C - j0 < FTL_RNN_PASS_CELLS ? C - j0 : FTL_RNN_PASS_CELLS;
            f32x4 z[BPW];
            layer_acc<true>(z, Wg, 4 * C, bg, Gates{cn, C, j0}, U, cn <= 2 * NB ? 128 : 256, nullptr, nullptr, start, tile_n, u, a.u_stride, xs, ws);
#pragma unroll
            for (int gs = 0; gs < 2; gs++) {                        // the lane's two cells of the pass, four rows each
                const int jj = gate_group(par, 4 * gs) * NB + li, j = j0 + jj;
                if (jj >= cn) continue;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int e = row_d + r;
                    if (e >= tile_n) continue;
                    const float gi = ftlrnnmath::sig32(z[4 * gs][r]);
                    const float gf = ftlrnnmath::sig32(z[4 * gs + 1][r]);
                    const float gg = ftlrnnmath::tanh32(z[4 * gs + 2][r]);
                    const float go = ftlrnnmath::sig32(z[4 * gs + 3][r]);
                    const float tt = gi * gg;
                    const float cn1 = __builtin_fmaf(gf, ps == 0 ? c[0][gs][r] : c[1][gs][r], tt);
                    const float th = ftlrnnmath::tanh32(cn1);
                    hn[e * a.h_stride + j] = go * th;               // (an array of its own: later passes still read the old h in u)
                    const float cw = wipe[r] ? 0.0f : cn1;
                    if (ps == 0) c[0][gs][r] = cw; else c[1][gs][r] = cw;
                    if (keep) a.state_out[((size_t)start + e) * S + C + j] = cw;
                }
            }
        }
        dense(Wy, Wy + (size_t)C * a.A, C, a.A, nullptr, nullptr, start, tile_n, hn, a.h_stride, act, m.act_stride, false, xs, ws);
        __syncthreads();
        // the block's outputs, contiguous runs of the tile's rows; then the rest of u for block b + 1 (every gate pass has read the old one)
        {
            float* y = reinterpret_cast<float*>(reinterpret_cast<char*>(a.head) + (int64_t)b * a.head_bb) + (size_t)start * a.A;
            for (int idx = t; idx < tile_n * a.A; idx += FTL_MLP_THREADS) {
                const int r = idx / a.A;
                y[idx] = act[r * m.act_stride + (idx - r * a.A)];
            }
        }
        if (a.h) {
            float* ho = reinterpret_cast<float*>(reinterpret_cast<char*>(a.h) + (int64_t)b * a.h_bb) + (size_t)start * C;
            for (int idx = t; idx < tile_n * C; idx += FTL_MLP_THREADS) {
                const int r = idx / C;
                ho[idx] = hn[r * a.h_stride + (idx - r * C)];
            }
        }
        if (!more) break;
        for (int idx = t; idx < tile_n * tail; idx += FTL_MLP_THREADS) {
            const int e = idx / tail, k = idx - e * tail;
            const size_t row_i = (size_t)start + e;
            const bool live = kind[row_i] != FTL_TR_VOID;
            float* so = keep ? a.state_out + row_i * S : nullptr;
            float v = 0.0f;
            if (k < a.P) {
                if (live) {
                    const char* ab = static_cast<const char*>(a.action) + (int64_t)b * a.action_bb;
                    if (m.head == FTL_ACTION_DISCRETE) v = reinterpret_cast<const int32_t*>(ab)[row_i] == k ? 1.0f : 0.0f;
                    else v = (float)reinterpret_cast<const double*>(ab)[row_i * a.P + k];
                }
                if (so) so[2 * C + k] = v;
            } else if (k < a.P + a.R) {
                if (live) v = (float)reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.reward) + (int64_t)b * a.reward_bb)[row_i];
            } else {
                const int j = k - a.P - a.R;
                if (live) v = hn[e * a.h_stride + j];
                if (so) so[j] = v;
            }
            u[e * a.u_stride + wx + k] = v;
        }
        if (keep && t < tile_n) a.state_out[((size_t)start + t) * S + 2 * C + a.P] = kind[(size_t)start + t] != FTL_TR_VOID ? 1.0f : 0.0f;
    }
}

// ---- ftl_rnn_backward: d loss / d params of the net on a recorded sequence (include/ftl.h: ftl_rnn_backward) ----
// ONE workgroup per GROUP of G = max(1, 64 / B) consecutive tiles of a set (the tile map of ftl_rnn_forward), the tiles one after the
// other, so the carry of back-propagation through time never leaves the workgroup.  Per tile: a forward sweep over the B blocks with the
// layers of ftl_rnn_forward_kernel (dense, layer_acc, gate_col: the same chains, the same bits) leaves h' and c' of every block in the
// record part of the workspace; then the blocks run DESCENDING.  A block of the reverse sweep recomputes the trunk (every hidden
// activation kept in LDS with a 1.0 in the bias's column) and u, takes dW_y and dh from dy, recomputes the gates pass by pass -- z in the
// registers of the lane that owns the cell, as in the forward, and dc_next with it --, writes the pass's dz to LDS, advances dW_g by
// u^T dz and du by dz W_g^T (both on the MFMA), and finishes with the trunk as ftl_mlp_backward does.  du of a cell with two passes
// travels between them through the group's carry rows in the workspace, every lane its own words.  The running partial of a span lives in
// the span's slice of the workspace as in ftl_mlp_backward_kernel; ftl_mlp_backward_reduce_kernel sums the spans.
// LDS: the hidden buffers, u, dh, the weight stage, and one region that is xs | h' | dy before the gate passes and dz from then on.
struct Bwd {
    ftlmlp::Args m;            // the trunk and the tile map over the n rows of a block; m.obs is block 0 of obs
    int32_t cell, P, R, A;
    int32_t u_stride, h_stride, dz_stride, stage;               // floats; stage: of the weight stage
    int32_t n_blocks, G, spg;                                   // tiles of a group, spans of a whole group
    int32_t groups0, groups_mid, spans0, spans_mid;             // of the first touched set and of a whole set
    const float* state; int64_t state_stride;
    int64_t obs_bb, action_bb, reward_bb, kind_bb, dy_bb;
    const void* action; const double* reward; const uint8_t* kind; const double* reward0;
    const float* dy; const float* dstate_in; float* dstate_out;
    float* part; int64_t count;                                 // the span partials, [spans][count]
    float* rec;                                                 // [B][n][2C]: h' | c' of every block, before any wipe
    float* carry;                                               // [groups][TILE][U]
};

// column j of a product -> word (j / cn) * C + j0 + j % cn of a matrix row: the pass's columns of W_g; cn = w_out, j0 = 0: the identity
struct ColMap { int cn, C, j0; };
__device__ __forceinline__ int map_col(const ColMap& cm, int j) { const int q = j / cm.cn; return q * cm.C + cm.j0 + (j - q * cm.cn); }

// ftlmlp::dw_blocks with the column map: G[(k0 + k) * ldg + map_col(j)] += the chain over the tile's 32 row slots of src[row][k] * delta[row][j]
__device__ __forceinline__ void dw_map(const float* src, int sstride, int k0, int kn, const float* delta, int dstride, int w_out,
                                       float* G, int ldg, const ColMap cm, bool first, int tile_n, int wave, int li, int lk) {
    constexpr int DWB = ftlmlp::DWB, WAVES = ftlmlp::WAVES;
    const int nkb = (kn + NB - 1) / NB, njb = (w_out + NB - 1) / NB, total = nkb * njb;
    for (int q0 = wave * DWB; q0 < total; q0 += WAVES * DWB) {
        f32x4 c[DWB];
        int kb[DWB], jb[DWB], gc[DWB];
#pragma unroll
        for (int v = 0; v < DWB; v++) {
            const int q = q0 + v < total ? q0 + v : total - 1;
            kb[v] = q / njb; jb[v] = q - kb[v] * njb;
            const int j = jb[v] * NB + li;
            gc[v] = map_col(cm, j < w_out ? j : w_out - 1);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int k = kb[v] * NB + 4 * lk + r;
                c[v][r] = (!first && q0 + v < total && k < kn && j < w_out) ? G[(size_t)(k0 + k) * ldg + gc[v]] : 0.0f;
            }
        }
        for (int rr = 0; rr < TILE; rr += 4) {
            const int row = rr + lk;
            const bool live = row < tile_n;
#pragma unroll
            for (int v = 0; v < DWB; v++) {
                if (q0 + v >= total) continue;                  // (wave-uniform)
                const int k = kb[v] * NB + li, j = jb[v] * NB + li;
                const float av = (live && k < kn) ? src[row * sstride + k] : 0.0f;
                const float bv = (live && j < w_out) ? delta[row * dstride + j] : 0.0f;
                c[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c[v], 0, 0, 0);
            }
        }
#pragma unroll
        for (int v = 0; v < DWB; v++) {
            if (q0 + v >= total) continue;
            const int j = jb[v] * NB + li;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int k = kb[v] * NB + 4 * lk + r;
                if (k < kn && j < w_out) G[(size_t)(k0 + k) * ldg + gc[v]] = c[v][r];
            }
        }
    }
}

__global__ __launch_bounds__(FTL_MLP_THREADS) void ftl_rnn_backward_kernel(const Bwd a) {
    extern __shared__ float4 rnn_bwd_lds[];
    const ftlmlp::Args& m = a.m;
    const int Lt = m.n_layers, C = a.cell, AS = m.act_stride, wx = m.width[Lt], tail = a.P + a.R + C, U = wx + tail, A = a.A, B = a.n_blocks;
    const int US = a.u_stride, HS = a.h_stride, ZS = a.dz_stride, DS = ftlmlp::dy_stride(A), w0 = m.width[0];
    float* hb = reinterpret_cast<float*>(rnn_bwd_lds);          // [Lt - 1][TILE][AS]: h_l of the trunk, then delta_l
    float* u = hb + (Lt - 1) * TILE * AS;                       // [TILE][US]: u and its 1.0; the x columns become delta_Lt
    float* dhb = u + TILE * US;                                 // [TILE][HS]: dh_next, then dh
    float* ws = dhb + TILE * HS;                                // the weight stage
    float* dzp = ws + a.stage;                                  // [TILE][ZS]: dz of a gate pass; before the passes:
    float* xs = dzp;                                            //   [TILE][XS]
    float* hn = xs + TILE * XS;                                 //   [TILE][HS]: h' of the block and its 1.0
    float* dyb = hn + TILE * HS;                                //   [TILE][DS]
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int g = wave % GROUPS, par = wave / GROUPS, row_a = g * EPW + li, row_d = g * EPW + 4 * lk;
    // the group's set, its rows of a block and its tiles
    int ms, gi;
    if ((int)blockIdx.x < a.groups0) { ms = 0; gi = (int)blockIdx.x; }
    else { const int q = (int)blockIdx.x - a.groups0; ms = 1 + q / a.groups_mid; gi = q % a.groups_mid; }
    const int set = m.env_first / m.envs_per_set + ms;
    int seg, seg_end;
    if (ms == 0) { seg = 0; seg_end = m.len0; }
    else {
        const int64_t s0 = (int64_t)m.len0 + (int64_t)(ms - 1) * m.envs_per_set, s1 = s0 + m.envs_per_set;
        seg = (int)s0; seg_end = s1 < (int64_t)m.n_envs ? (int)s1 : m.n_envs;
    }
    const int set_tiles = (seg_end - seg + TILE - 1) / TILE, tile_lo = gi * a.G;
    const int n_tiles = set_tiles - tile_lo < a.G ? set_tiles - tile_lo : a.G;
    const int64_t span_base = (ms == 0 ? 0 : (int64_t)a.spans0 + (int64_t)(ms - 1) * a.spans_mid) + (int64_t)gi * a.spg;
    float* carry = a.carry + (size_t)blockIdx.x * TILE * U;
    const float* P0 = m.params + (int64_t)set * m.set_stride;
    int off[FTL_MLP_MAX_LAYERS + 1];
    off[0] = 0;
#pragma unroll
    for (int l = 0; l < FTL_MLP_MAX_LAYERS; l++) off[l + 1] = off[l] + (l < Lt ? (m.width[l] + 1) * m.width[l + 1] : 0);
    const int o_g = off[Lt], o_y = o_g + (U + 1) * 4 * C;
    const float* Wg = P0 + o_g;
    const float* bg = Wg + (size_t)U * 4 * C;
    const float* Wy = P0 + o_y;
    const size_t rec_bb = (size_t)m.n_envs * 2 * C;             // floats between two blocks of the record
    constexpr int PASSES = FTL_RNN_MAX_CELL / FTL_RNN_PASS_CELLS;
    static_assert(PASSES == 2, "dc_next of a pass is selected between two register sets");

    for (int ti = 0; ti < n_tiles; ti++) {
        const int start = seg + (tile_lo + ti) * TILE;
        const int tile_n = seg_end - start < TILE ? seg_end - start : TILE;
        const bool busy = g * EPW < tile_n;
        // the trunk of block b: h_l into hb (with the bias's 1.0), x into u
        auto trunk = [&](int b) {
            const float* obs = reinterpret_cast<const float*>(reinterpret_cast<const char*>(m.obs) + (int64_t)b * a.obs_bb);
            const float* P = P0;
            for (int l = 0; l < Lt; l++) {
                const int w_in = m.width[l], w_out = m.width[l + 1];
                const bool last = l + 1 == Lt;
                dense(P, P + (size_t)w_in * w_out, w_in, w_out, l == 0 ? obs : nullptr, nullptr, start, tile_n,
                      l == 0 ? nullptr : hb + (l - 1) * TILE * AS, AS, last ? u : hb + l * TILE * AS, last ? US : AS, true, xs, ws);
                if (!last && t < TILE) hb[l * TILE * AS + t * AS + w_out] = 1.0f;
                P += ((size_t)w_in + 1) * w_out;
            }
        };
        // the rest of u for block b: a_prev | r_prev | h of the row it reads (the zero rule of ftl_rnn_forward), and the bias's 1.0
        auto fill_tail = [&](int b) {
            const uint8_t* kind = b ? a.kind + (int64_t)(b - 1) * a.kind_bb : nullptr;
            for (int idx = t; idx < tile_n * tail; idx += FTL_MLP_THREADS) {
                const int e = idx / tail, k = idx - e * tail;
                const size_t row_i = (size_t)start + e;
                float v = 0.0f;
                if (b == 0) {
                    const float* row = a.state + row_i * a.state_stride;
                    if (k < a.P) v = row[2 * C + k];
                    else if (k < a.P + a.R) v = row[2 * C + a.P] != 0.0f ? (float)(a.reward0 ? a.reward0[row_i] : 0.0) : 0.0f;
                    else v = row[k - a.P - a.R];
                } else if (kind[row_i] != FTL_TR_VOID) {
                    if (k < a.P) {
                        const char* ab = static_cast<const char*>(a.action) + (int64_t)(b - 1) * a.action_bb;
                        if (m.head == FTL_ACTION_DISCRETE) v = reinterpret_cast<const int32_t*>(ab)[row_i] == k ? 1.0f : 0.0f;
                        else v = (float)reinterpret_cast<const double*>(ab)[row_i * a.P + k];
                    } else if (k < a.P + a.R)
                        v = (float)reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.reward) + (int64_t)(b - 1) * a.reward_bb)[row_i];
                    else v = a.rec[(size_t)(b - 1) * rec_bb + row_i * 2 * C + (k - a.P - a.R)];
                }
                u[e * US + wx + k] = v;
            }
            if (t < TILE) u[t * US + U] = 1.0f;
        };
        // c of the row block b reads
        auto c_prev = [&](int b, size_t row_i, int j) -> float {
            if (b == 0) return a.state[row_i * a.state_stride + C + j];
            if (a.kind[(int64_t)(b - 1) * a.kind_bb + row_i] == FTL_TR_VOID) return 0.0f;
            return a.rec[(size_t)(b - 1) * rec_bb + row_i * 2 * C + C + j];
        };

        // ---- forward sweep: h' and c' of every block into the record
        for (int b = 0; b < B; b++) {
            trunk(b);
            fill_tail(b);
#pragma unroll 1
            for (int ps = 0; ps < PASSES; ps++) {
                const int j0 = ps * FTL_RNN_PASS_CELLS;
                if (j0 >= C) break;
                const int cn = C - j0 < FTL_RNN_PASS_CELLS ? C - j0 : FTL_RNN_PASS_CELLS;
                f32x4 z[BPW];
                layer_acc<true>(z, Wg, 4 * C, bg, Gates{cn, C, j0}, U, cn <= 2 * NB ? 128 : 256, nullptr, nullptr, start, tile_n, u, US, xs, ws);
#pragma unroll
                for (int gs = 0; gs < 2; gs++) {
                    const int jj = gate_group(par, 4 * gs) * NB + li, j = j0 + jj;
                    if (jj >= cn) continue;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int e = row_d + r;
                        if (e >= tile_n) continue;
                        const size_t row_i = (size_t)start + e;
                        const float gi_ = ftlrnnmath::sig32(z[4 * gs][r]);
                        const float gf = ftlrnnmath::sig32(z[4 * gs + 1][r]);
                        const float gg = ftlrnnmath::tanh32(z[4 * gs + 2][r]);
                        const float go = ftlrnnmath::sig32(z[4 * gs + 3][r]);
                        const float tt = gi_ * gg;
                        const float cn1 = __builtin_fmaf(gf, c_prev(b, row_i, j), tt);
                        const float th = ftlrnnmath::tanh32(cn1);
                        float* rc = a.rec + (size_t)b * rec_bb + row_i * 2 * C;
                        rc[j] = go * th;
                        rc[C + j] = cn1;
                    }
                }
            }
        }

        // ---- reverse sweep
        float dcn[PASSES][2][4];
#pragma unroll
        for (int ps = 0; ps < PASSES; ps++)
#pragma unroll
            for (int gs = 0; gs < 2; gs++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int j = ps * FTL_RNN_PASS_CELLS + gate_group(par, 4 * gs) * NB + li, e = row_d + r;
                    dcn[ps][gs][r] = (a.dstate_in && j < C && e < tile_n) ? a.dstate_in[((size_t)start + e) * 2 * C + C + j] : 0.0f;
                }
        for (int b = B - 1; b >= 0; b--) {
            const int pair = ti * B + (B - 1 - b);
            const bool first = pair % FTL_RNN_BWD_SPAN == 0;
            float* Gs = a.part + (span_base + pair / FTL_RNN_BWD_SPAN) * a.count;
            const uint8_t* kind = b + 1 < B ? a.kind + (int64_t)b * a.kind_bb : nullptr;        // the row block b + 1 read was zeros where VOID
            trunk(b);
            fill_tail(b);
            {
                const float* dy = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.dy) + (int64_t)b * a.dy_bb) + (size_t)start * A;
                for (int idx = t; idx < TILE * A; idx += FTL_MLP_THREADS) {
                    const int r = idx / A;
                    dyb[r * DS + (idx - r * A)] = r < tile_n ? dy[idx] : 0.0f;
                }
                const float* hr = a.rec + (size_t)b * rec_bb + (size_t)start * 2 * C;
                for (int idx = t; idx < tile_n * C; idx += FTL_MLP_THREADS) {
                    const int r = idx / C, k = idx - r * C;
                    hn[r * HS + k] = hr[(size_t)r * 2 * C + k];
                }
                if (t < TILE) hn[t * HS + C] = 1.0f;
            }
            __syncthreads();
            dw_map(hn, HS, 0, C + 1, dyb, DS, A, Gs + o_y, A, ColMap{A, A, 0}, first, tile_n, wave, li, lk);
            // dh = the chain of W_y over dy, plus dh_next
            for (int idx = t; idx < tile_n * C; idx += FTL_MLP_THREADS) {
                const int e = idx / C, k = idx - e * C;
                const size_t row_i = (size_t)start + e;
                float acc = 0.0f;
                for (int j = 0; j < A; j++) acc = __builtin_fmaf(Wy[k * A + j], dyb[e * DS + j], acc);
                float nx;
                if (b + 1 == B) nx = a.dstate_in ? a.dstate_in[row_i * 2 * C + k] : 0.0f;
                else nx = kind[row_i] == FTL_TR_VOID ? 0.0f : dhb[e * HS + k];
                dhb[e * HS + k] = acc + nx;
            }
            bool wipe[4];
#pragma unroll
            for (int r = 0; r < 4; r++) wipe[r] = kind && row_d + r < tile_n && kind[(size_t)start + row_d + r] == FTL_TR_VOID;
#pragma unroll 1
            for (int ps = 0; ps < PASSES; ps++) {
                const int j0 = ps * FTL_RNN_PASS_CELLS;
                if (j0 >= C) break;
                const int cn = C - j0 < FTL_RNN_PASS_CELLS ? C - j0 : FTL_RNN_PASS_CELLS, w = 4 * cn;
                const bool firstp = ps == 0, lastp = j0 + cn >= C;
                {
                    f32x4 z[BPW];
                    // (layer_acc() begins with a barrier: u, dh are complete, and nobody reads h', dy or the last pass's dz any more)
                    layer_acc<true>(z, Wg, 4 * C, bg, Gates{cn, C, j0}, U, cn <= 2 * NB ? 128 : 256, nullptr, nullptr, start, tile_n, u, US, xs, ws);
#pragma unroll
                    for (int gs = 0; gs < 2; gs++) {
                        const int jj = gate_group(par, 4 * gs) * NB + li, j = j0 + jj;
                        if (jj >= cn) continue;
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int e = row_d + r;
                            if (e >= tile_n) continue;
                            const size_t row_i = (size_t)start + e;
                            const float gi_ = ftlrnnmath::sig32(z[4 * gs][r]);
                            const float gf = ftlrnnmath::sig32(z[4 * gs + 1][r]);
                            const float gg = ftlrnnmath::tanh32(z[4 * gs + 2][r]);
                            const float go = ftlrnnmath::sig32(z[4 * gs + 3][r]);
                            const float cp = c_prev(b, row_i, j);
                            const float tt = gi_ * gg;
                            const float cn1 = __builtin_fmaf(gf, cp, tt);
                            const float tc = ftlrnnmath::tanh32(cn1);
                            const float dh = dhb[e * HS + j];
                            const float dcx = wipe[r] ? 0.0f : (ps == 0 ? dcn[0][gs][r] : dcn[1][gs][r]);
                            const float q = dh * go;
                            const float d = __builtin_fmaf(-tc, tc, 1.0f);
                            const float dc = __builtin_fmaf(q, d, dcx);
                            const float d_o = dh * tc;
                            const float di = dc * gg, dg = dc * gi_, df = dc * cp, dnx = dc * gf;
                            if (ps == 0) dcn[0][gs][r] = dnx; else dcn[1][gs][r] = dnx;
                            float* zr = dzp + e * ZS + jj;
                            zr[0] = di * __builtin_fmaf(-gi_, gi_, gi_);
                            zr[cn] = df * __builtin_fmaf(-gf, gf, gf);
                            zr[2 * cn] = dg * __builtin_fmaf(-gg, gg, 1.0f);
                            zr[3 * cn] = d_o * __builtin_fmaf(-go, go, go);
                        }
                    }
                }
                __syncthreads();
                dw_map(u, US, 0, U + 1, dzp, ZS, w, Gs + o_g, 4 * C, ColMap{cn, C, j0}, first, tile_n, wave, li, lk);
                // du[r][k] = the chain over the pass's columns of W_g[k][col] * dz[r][col], from +0 or the pass before
                const int kc = ftlmlp::chunk_rows(w), wst = ftlmlp::bwd_stride(w);
                for (int k0 = 0; k0 < U; k0 += kc) {
                    const int kn = U - k0 < kc ? U - k0 : kc, nkb = (kn + NB - 1) / NB;
                    __syncthreads();
                    for (int idx = t; idx < kn * w; idx += FTL_MLP_THREADS) {
                        const int kk = idx / w, dd = idx - kk * w;
                        ws[kk * wst + dd] = Wg[(size_t)(k0 + kk) * 4 * C + map_col(ColMap{cn, C, j0}, dd)];
                    }
                    __syncthreads();
                    if (!busy) continue;
                    f32x4 acc[2];
                    const float* wr[2];
#pragma unroll
                    for (int mm = 0; mm < 2; mm++) {
                        const int k = (par + PARITIES * mm) * NB + li;
                        wr[mm] = ws + (k < kn ? k : kn - 1) * wst;
#pragma unroll
                        for (int r = 0; r < 4; r++) acc[mm][r] = (firstp || k >= kn) ? 0.0f : carry[(row_d + r) * U + k0 + k];
                    }
                    for (int j = 0; j < w; j += 4) {
                        const float av = dzp[row_a * ZS + j + lk];
#pragma unroll
                        for (int mm = 0; mm < 2; mm++)
                            if (par + PARITIES * mm < nkb) acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[mm][j + lk], acc[mm], 0, 0, 0);
                    }
#pragma unroll
                    for (int mm = 0; mm < 2; mm++) {
                        const int k = (par + PARITIES * mm) * NB + li, kk = k0 + k;
                        if (k >= kn) continue;
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int e = row_d + r;
                            const float v = acc[mm][r];
                            if (!lastp) carry[e * U + kk] = v;
                            else if (kk < wx) { float* p = u + e * US + kk; *p = *p > 0.0f ? v : 0.0f; }
                            else if (kk >= wx + a.P + a.R) dhb[e * HS + (kk - wx - a.P - a.R)] = v;
                        }
                    }
                }
            }
            // the trunk, as ftl_mlp_backward_kernel: delta_Lt lies in the x columns of u
            for (int l = Lt; l >= 1; l--) {
                const int w_in = m.width[l - 1], w_out = m.width[l];
                const float* delta = l == Lt ? u : hb + (l - 1) * TILE * AS;
                const int dst = l == Lt ? US : AS;
                float* Gl = Gs + off[l - 1];
                if (l == 1) {
                    const float* obs = reinterpret_cast<const float*>(reinterpret_cast<const char*>(m.obs) + (int64_t)b * a.obs_bb);
                    for (int k0 = 0; k0 < w0 + 1; k0 += KC) {
                        const int kn = w0 + 1 - k0 < KC ? w0 + 1 - k0 : KC;
                        __syncthreads();
                        const int e = t >> 3;
                        if (e < tile_n) {
                            const size_t row = (size_t)(start + e) * w0;
                            for (int kk = t & 7; kk < kn; kk += 8) xs[e * XS + kk] = k0 + kk < w0 ? obs[row + k0 + kk] : 1.0f;
                        }
                        __syncthreads();
                        dw_map(xs, XS, k0, kn, delta, dst, w_out, Gl, w_out, ColMap{w_out, w_out, 0}, first, tile_n, wave, li, lk);
                    }
                    break;
                }
                float* hprev = hb + (l - 2) * TILE * AS;
                __syncthreads();
                dw_map(hprev, AS, 0, w_in + 1, delta, dst, w_out, Gl, w_out, ColMap{w_out, w_out, 0}, first, tile_n, wave, li, lk);
                const float* W = P0 + off[l - 1];
                const int kc = ftlmlp::chunk_rows(w_out), wst = ftlmlp::bwd_stride(w_out);
                for (int k0 = 0; k0 < w_in; k0 += kc) {
                    const int kn = w_in - k0 < kc ? w_in - k0 : kc, nkb = (kn + NB - 1) / NB;
                    __syncthreads();
                    ftlmlp::stage_rows(ws, wst, W + (size_t)k0 * w_out, kn, w_out, t);
                    __syncthreads();
                    if (!busy) continue;
                    f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
                    const float* wr[2];
#pragma unroll
                    for (int mm = 0; mm < 2; mm++) {
                        const int k = (par + PARITIES * mm) * NB + li;
                        wr[mm] = ws + (k < kn ? k : kn - 1) * wst;
                    }
                    int j = 0;
                    for (; j + 4 <= w_out; j += 4) {
                        const float av = delta[row_a * dst + j + lk];
#pragma unroll
                        for (int mm = 0; mm < 2; mm++)
                            if (par + PARITIES * mm < nkb) acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[mm][j + lk], acc[mm], 0, 0, 0);
                    }
                    for (; j < w_out; j++) {
#pragma unroll
                        for (int mm = 0; mm < 2; mm++) {
                            if (par + PARITIES * mm >= nkb) continue;
                            const float wv = wr[mm][j];
#pragma unroll
                            for (int r = 0; r < 4; r++) acc[mm][r] = __builtin_fmaf(wv, delta[(row_d + r) * dst + j], acc[mm][r]);
                        }
                    }
#pragma unroll
                    for (int mm = 0; mm < 2; mm++) {
                        const int k = (par + PARITIES * mm) * NB + li;
                        if (k >= kn) continue;
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            float* p = hprev + (row_d + r) * AS + k0 + k;
                            *p = *p > 0.0f ? acc[mm][r] : 0.0f;
                        }
                    }
                }
            }
        }
        // d loss / d (h, c) of the rows block 0 read
        __syncthreads();
        if (a.dstate_out) {
            for (int idx = t; idx < tile_n * C; idx += FTL_MLP_THREADS) {
                const int e = idx / C, k = idx - e * C;
                a.dstate_out[((size_t)start + e) * 2 * C + k] = dhb[e * HS + k];
            }
#pragma unroll
            for (int ps = 0; ps < PASSES; ps++)
#pragma unroll
                for (int gs = 0; gs < 2; gs++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int j = ps * FTL_RNN_PASS_CELLS + gate_group(par, 4 * gs) * NB + li, e = row_d + r;
                        if (j < C && e < tile_n) a.dstate_out[((size_t)start + e) * 2 * C + C + j] = dcn[ps][gs][r];
                    }
        }
        __syncthreads();
    }
}

}  // namespace ftlrnn

static int32_t rnn_prev_width(int32_t head_width, uint32_t flags) { return (flags & FTL_RNN_PREV_ACTION) ? head_width : 0; }

// floats of one weight set; -1 outside the limits of include/ftl.h
static int64_t rnn_param_count(const int32_t* w, int32_t Lt, int32_t C, uint32_t flags) {
    if (!w || Lt < 1 || Lt > FTL_MLP_MAX_LAYERS - 1 || C < 1 || C > FTL_RNN_MAX_CELL || (flags & ~3u)) return -1;
    const int64_t trunk = mlp_param_count(w, Lt);
    const int32_t A = w[Lt + 1];
    if (trunk < 0 || (A != 1 && A != 2 && A != 5)) return -1;
    const int64_t U = (int64_t)w[Lt] + rnn_prev_width(A, flags) + ((flags & FTL_RNN_PREV_REWARD) ? 1 : 0) + C;
    return trunk + (U + 1) * 4 * C + ((int64_t)C + 1) * A;
}

static size_t rnn_lds_bytes(int32_t act_stride, int32_t u_stride, int32_t h_stride) {
    return ((size_t)FTL_MLP_ENV_TILE * ((size_t)act_stride + u_stride + h_stride + ftlmlp::XS) + FTL_MLP_W_STAGE + 64) * sizeof(float);
}

// the checks of the net itself, for `n` rows (the handle's envs, or the rows of a block of ftl_rnn_forward: `rows` names them in the last
// message): those of mlp_net_check, in its order, then the cell
static int rnn_net_check(const ftl_rnn* net, int64_t n, const char* rows) {
    const int32_t Lt = net->n_layers;
    if (Lt < 1) return fail(FTL_E_INVALID, "rnn: n_layers must be at least 1");
    if (Lt > FTL_MLP_MAX_LAYERS - 1) return fail(FTL_E_UNSUPPORTED, "rnn: more than FTL_MLP_MAX_LAYERS - 1 trunk layers");
    if (int rc = net_widths_check("rnn: ", net->width, Lt + 1)) return rc;
    if (net->cell < 1) return fail(FTL_E_INVALID, "rnn: cell must be at least 1");
    if (net->cell > FTL_RNN_MAX_CELL) return fail(FTL_E_UNSUPPORTED, "rnn: cell beyond FTL_RNN_MAX_CELL");
    if (net->flags & ~(uint32_t)(FTL_RNN_PREV_ACTION | FTL_RNN_PREV_REWARD)) return fail(FTL_E_INVALID, "rnn: unknown bit in ftl_rnn.flags");
    if (net->activation != FTL_MLP_ACT_RELU) return fail(FTL_E_UNSUPPORTED, "rnn: the trunk is ReLU: ftl_rnn.activation must be FTL_MLP_ACT_RELU (0)");
    const int32_t wl = net->width[Lt + 1], C = net->cell;
    if (wl != 1 && wl != 2 && wl != 5) return fail(FTL_E_INVALID, "rnn: the head width must be 2 (Box(2)), 1 (Box(1) turn) or 5 (Discrete(5))");
    return net_sets_check("rnn: ", net, rnn_param_count(net->width, Lt, C, net->flags), "ftl_rnn_param_count", n, rows);
}

// ... and of its state block
static int rnn_state_check(const ftl_rnn* net) {
    const int32_t S = 2 * net->cell + rnn_prev_width(net->width[net->n_layers + 1], net->flags) + 1;
    if (!net->state) return fail(FTL_E_INVALID, "rnn: state is NULL");
    if (((uintptr_t)net->state) & 3) return fail(FTL_E_INVALID, "rnn: state must be 4-byte aligned");
    if (net->state_stride < S) return fail(FTL_E_INVALID, "rnn: state_stride below S = 2 * cell + P + 1");
    return FTL_OK;
}

// what follows from a checked net and its `n` rows: the trunk's arguments but for obs, the bounds and `action`, the tile map and the grid's
// tiles, the LDS strides of u and h'
static void rnn_fill(const ftl_rnn* net, int64_t n, ftlmlp::Args& m, int32_t& u_stride, int32_t& h_stride, unsigned& grid) {
    const int32_t Lt = net->n_layers, wl = net->width[Lt + 1], C = net->cell;
    m.params = net->params; m.set_stride = net->set_stride;
    m.n_envs = (int32_t)n; m.n_layers = Lt; m.env_first = net->env_first; m.envs_per_set = net->envs_per_set;
    int wmax = wl;                                              // act holds the trunk's inner layers and y
    for (int l = 0; l <= FTL_MLP_MAX_LAYERS; l++) {
        m.width[l] = l <= Lt ? net->width[l] : 0;
        if (l >= 1 && l < Lt && m.width[l] > wmax) wmax = m.width[l];
    }
    m.act_stride = ((wmax + 31) & ~31) + 2;
    grid = tile_map_fill(tile_map(net->env_first, net->envs_per_set, n), m);
    m.head = wl == 2 ? FTL_ACTION_BOX2 : wl == 1 ? FTL_ACTION_TURN : FTL_ACTION_DISCRETE;
    m.action = nullptr;
    const int U = net->width[Lt] + rnn_prev_width(wl, net->flags) + ((net->flags & FTL_RNN_PREV_REWARD) ? 1 : 0) + C;
    u_stride = ((U + 31) & ~31) + 2; h_stride = ((C + 31) & ~31) + 2;
}

// the checks of the net and its state that every entry on a handle's policy_obs shares (those of mlp_args, in its order, then the cell and
// the state); fills the kernel's arguments but for action / state_rec / alive / before, its grid and its LDS bytes
static int rnn_args(ftl_handle* h, const ftl_outputs* out, const ftl_rnn* net, ftlrnn::Args& a, unsigned& grid, size_t& lds) {
    if (!h || !out || !net || !net->params) return fail(FTL_E_INVALID, "null argument");
    if (int rc = rnn_net_check(net, h->P.n_envs, "the handle's last env")) return rc;
    if (!out->policy_obs || h->P.pol_h <= 0 || h->P.pol_width <= 0) return fail(FTL_E_INVALID, "rnn: the policy reads policy_obs (ftl_outputs.policy_obs, a config with a sensor for it)");
    if ((int64_t)net->width[0] != (int64_t)h->P.pol_h * h->P.pol_width) return fail(FTL_E_INVALID, "rnn: width[0] must be H * W of policy_obs");
    if (int rc = rnn_state_check(net)) return rc;
    if (!out->reward || !out->done) return fail(FTL_E_INVALID, "rnn: the policy reads out->reward and out->done");
    const int32_t Lt = net->n_layers, wl = net->width[Lt + 1], C = net->cell;
    ftlmlp::Args& m = a.m;
    rnn_fill(net, h->P.n_envs, m, a.u_stride, a.h_stride, grid);
    m.obs = out->policy_obs;
    const ftl_robot_params& f = h->P.cfg.follower;
    m.lo0 = f.min_speed; m.hi0 = f.max_speed; m.lo1 = -f.max_rotation_speed; m.hi1 = f.max_rotation_speed;
    a.cell = C; a.P = rnn_prev_width(wl, net->flags); a.R = (net->flags & FTL_RNN_PREV_REWARD) ? 1 : 0; a.A = wl;
    a.state = net->state; a.state_stride = net->state_stride; a.state_rec = nullptr;
    a.reward = out->reward; a.out_done = out->done; a.alive = nullptr;
    a.env_int = h->P.env_int; a.rec_stride = h->P.rec_stride; a.before = 0;
    lds = rnn_lds_bytes(m.act_stride, a.u_stride, a.h_stride);
    return FTL_OK;
}

// dynamic LDS above 64 KiB is asked for on the current device before the launch (harmless where the runtime needs no asking; a launch that
// is refused all the same is reported by launched())
static int rnn_kernel_ready(size_t lds, const void* kernel = (const void*)ftlrnn::ftl_rnn_kernel) {
    if (lds > 160 * 1024) return fail(FTL_E_UNSUPPORTED, "rnn: the net needs more than 160 KiB of LDS per workgroup");
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return FTL_OK;
}

// the groups and spans of ftl_rnn_backward for a checked net and its rows (include/ftl.h): per touched set -- the first, a whole one, the
// last (0 when the first is the only one) -- and in all
struct RnnBwdPlan { int64_t G, spg, groups0, groups_mid, groups, spans0, spans_mid, spans_last, n_touched, spans; };
static RnnBwdPlan rnn_bwd_plan(const ftl_rnn* net, int64_t B, int64_t n) {
    const TileMap m = tile_map(net->env_first, net->envs_per_set, n);
    const int64_t span = FTL_RNN_BWD_SPAN;
    RnnBwdPlan p;
    p.G = std::max<int64_t>(1, span / B);
    p.spg = (p.G * B + span - 1) / span;
    auto groups_of = [&](int64_t tiles) { return (tiles + p.G - 1) / p.G; };
    auto spans_of = [&](int64_t tiles) {
        const int64_t cut = tiles % p.G;
        return (tiles / p.G) * p.spg + (cut ? (cut * B + span - 1) / span : 0);
    };
    p.groups0 = groups_of(m.tiles0); p.groups_mid = m.rem ? groups_of(m.tiles_per_set) : 1;
    p.groups = p.groups0 + m.full * p.groups_mid + (m.last ? groups_of(m.tiles_last) : 0);
    p.spans0 = spans_of(m.tiles0); p.spans_mid = m.rem ? spans_of(m.tiles_per_set) : 1;
    p.spans_last = !m.rem ? 0 : m.last ? spans_of(m.tiles_last) : p.spans_mid;
    p.n_touched = 1 + m.full + (m.last ? 1 : 0);
    p.spans = p.spans0 + m.full * p.spans_mid + (m.last ? p.spans_last : 0);
    return p;
}

// the workspace of ftl_rnn_backward in floats: the span partials, the record h' | c' of every block, the groups' carry rows
static int64_t rnn_bwd_workspace_floats(const ftl_rnn* net, const RnnBwdPlan& p, int64_t B, int64_t n, int64_t count) {
    const int32_t Lt = net->n_layers, A = net->width[Lt + 1], C = net->cell;
    const int64_t U = (int64_t)net->width[Lt] + rnn_prev_width(A, net->flags) + ((net->flags & FTL_RNN_PREV_REWARD) ? 1 : 0) + C;
    return p.spans * count + B * n * 2 * C + p.groups * FTL_MLP_ENV_TILE * U;
}

// What ftl_rnn_forward and ftl_rnn_backward check of their net and of an ftl_rnn_sequence alike, in their common order, between the
// checks of their own: `name` heads the messages, `limit` is the entry's text for more than 65,535 blocks
struct RnnSeq {
    const char *name, *limit;
    const ftl_handle* h; const ftl_rnn* net; int32_t n_blocks, n; const ftl_rnn_sequence* seq;
    int32_t A, C, P, R; bool more; int64_t arow, ael;           // (set by open())
    int no(int code, const std::string& what) const { return fail(code, std::string(name) + ": " + what); }
    // h, net, seq and `g_missing` (the entry's further struct, if it has one); n_blocks, n, the net and its state; seq->obs
    int open(bool g_missing) {
        if (!h) return no(FTL_E_INVALID, "null argument: h");
        if (!net) return no(FTL_E_INVALID, "null argument: net");
        if (!net->params) return no(FTL_E_INVALID, "null argument: net->params");
        if (!seq) return no(FTL_E_INVALID, "null argument: seq");
        if (g_missing) return no(FTL_E_INVALID, "null argument: g");
        if (n_blocks < 1 || n < 1) return no(FTL_E_INVALID, "n_blocks and n must be at least 1");
        if (n_blocks > 65535) return no(FTL_E_UNSUPPORTED, limit);
        if (int rc = rnn_net_check(net, n, "the last row")) return rc;
        if (int rc = rnn_state_check(net)) return rc;
        A = net->width[net->n_layers + 1]; C = net->cell;
        P = rnn_prev_width(A, net->flags); R = (net->flags & FTL_RNN_PREV_REWARD) ? 1 : 0;
        more = n_blocks > 1; arow = A == 2 ? 16 : A == 1 ? 8 : 4; ael = A == 5 ? 4 : 8;
        if (!seq->obs) return no(FTL_E_INVALID, "null argument: seq->obs");
        return FTL_OK;
    }
    // the records between the blocks are there where the net reads them; the bytes between two blocks of obs and of the records
    int blocks() const {
        if (more && !seq->kind) return no(FTL_E_INVALID, "null argument: seq->kind (read for every block but the last)");
        if (more && P && !seq->action) return no(FTL_E_INVALID, "null argument: seq->action (the net has FTL_RNN_PREV_ACTION)");
        if (more && R && !seq->reward) return no(FTL_E_INVALID, "null argument: seq->reward (the net has FTL_RNN_PREV_REWARD)");
        if (seq->obs_block_bytes < (int64_t)n * net->width[0] * 4 || (seq->obs_block_bytes & 3))
            return no(FTL_E_INVALID, "obs_block_bytes must be a multiple of 4 of at least one block, n * width[0] * 4");
        if (more && P && (seq->action_block_bytes < (int64_t)n * arow || (seq->action_block_bytes & (ael - 1))))
            return no(FTL_E_INVALID, "action_block_bytes must be a multiple of the action element of at least one block of encoded actions");
        if (more && R && (seq->reward_block_bytes < (int64_t)n * 8 || (seq->reward_block_bytes & 7)))
            return no(FTL_E_INVALID, "reward_block_bytes must be a multiple of 8 of at least one block, n * 8");
        if (more && seq->kind_block_bytes < (int64_t)n) return no(FTL_E_INVALID, "kind_block_bytes below one block, n");
        return FTL_OK;
    }
    int aligned() const {
        if (((uintptr_t)seq->obs) & 3) return no(FTL_E_INVALID, "obs must be 4-byte aligned");
        if (more && P && (((uintptr_t)seq->action) & (uintptr_t)(ael - 1))) return no(FTL_E_INVALID, "action not aligned to its element");
        if (more && R && (((uintptr_t)seq->reward) & 7)) return no(FTL_E_INVALID, "reward must be 8-byte aligned");
        if (((uintptr_t)seq->reward0) & 7) return no(FTL_E_INVALID, "reward0 must be 8-byte aligned");
        return FTL_OK;
    }
    // the fields that ftlrnn::Seq and ftlrnn::Bwd have in common, but for those rnn_fill has set
    template <typename Args> void fill(Args& a) const {
        a.m.obs = seq->obs; a.m.lo0 = a.m.hi0 = a.m.lo1 = a.m.hi1 = 0.0;
        a.cell = C; a.P = P; a.R = R; a.A = A; a.n_blocks = n_blocks;
        a.state = net->state; a.state_stride = net->state_stride;
        a.obs_bb = seq->obs_block_bytes; a.action_bb = seq->action_block_bytes; a.reward_bb = seq->reward_block_bytes;
        a.kind_bb = seq->kind_block_bytes;
        a.action = P ? seq->action : nullptr; a.reward = R ? seq->reward : nullptr; a.kind = seq->kind; a.reward0 = R ? seq->reward0 : nullptr;
    }
};

extern "C" {

size_t ftl_sizeof_rnn(void) { return sizeof(ftl_rnn); }
size_t ftl_sizeof_rnn_collect_buffers(void) { return sizeof(ftl_rnn_collect_buffers); }
size_t ftl_sizeof_rnn_sequence(void) { return sizeof(ftl_rnn_sequence); }

int64_t ftl_rnn_param_count(const int32_t* widths, int32_t n_layers, int32_t cell, uint32_t flags) { return rnn_param_count(widths, n_layers, cell, flags); }

int ftl_rnn_act(ftl_handle* h, const ftl_outputs* out, const ftl_rnn* net, const float* noise, const float* sigma, float* head_rec,
                float* obs_rec, float* state_rec, void* action, uint32_t flags, void* stream) {
    if (!action) return fail(FTL_E_INVALID, "null argument");
    ftlrnn::Args a; unsigned grid; size_t lds;
    if (int rc = rnn_args(h, out, net, a, grid, lds)) return rc;
    if (flags & ~(uint32_t)FTL_RNN_ZERO_ON_OUT_DONE) return fail(FTL_E_INVALID, "ftl_rnn_act takes no flag but FTL_RNN_ZERO_ON_OUT_DONE");
    if (((uintptr_t)action) & (a.m.head == FTL_ACTION_DISCRETE ? 3 : 7)) return fail(FTL_E_INVALID, "ftl_rnn_act: action not aligned to its element");
    if (int rc = mlp_sample_check("ftl_rnn_act", a.m.head, noise, sigma, head_rec, obs_rec)) return rc;
    if (((uintptr_t)state_rec) & 3) return fail(FTL_E_INVALID, "ftl_rnn_act: state_rec must be 4-byte aligned");
    if (int rc = check_ready(h, out)) return rc;
    if (int rc = set_device(h)) return rc;
    if (int rc = rnn_kernel_ready(lds)) return rc;
    a.m.action = action; a.state_rec = state_rec; a.before = (flags & FTL_RNN_ZERO_ON_OUT_DONE) ? 1 : 0;
    const ftlmlp::Sample sm{noise, sigma, head_rec, obs_rec};
    hipLaunchKernelGGL(ftlrnn::ftl_rnn_kernel, dim3(grid), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a, sm);
    return launched();
}

int ftl_rollout_rnn(ftl_handle* h, int32_t T, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro, const ftl_rnn* net,
                    void* actions, int64_t step_bytes, uint32_t flags, void* stream) {
    if (int rc = policy_rollout_check("ftl_rollout_rnn", h, out, net, ro, T, flags)) return rc;
    ftlrnn::Args a; unsigned grid; size_t lds;
    if (int rc = rnn_args(h, out, net, a, grid, lds)) return rc;
    const ftlmlp::Sample sm{nullptr, nullptr, nullptr, nullptr};
    return policy_rollout("ftl_rollout_rnn", h, a.m.head, T, gamma, out, ro, actions, step_bytes, stream, [&] { return rnn_kernel_ready(lds); },
                          [&](void* action) {
        a.m.action = action; a.alive = h->ro_alive;             // (the fold's first pass sets it from the state before decision 0 reads it)
        hipLaunchKernelGGL(ftlrnn::ftl_rnn_kernel, dim3(grid), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a, sm);
    });
}

int ftl_collect_rnn(ftl_handle* h, int32_t T, const ftl_outputs* out, const ftl_rnn* net, const ftl_rnn_collect_buffers* rb, uint32_t flags, void* stream) {
    if (int rc = collect_check("ftl_collect_rnn", h, out, net, rb, flags, T)) return rc;
    ftlrnn::Args a; unsigned grid; size_t lds;
    if (int rc = rnn_args(h, out, net, a, grid, lds)) return rc;
    return collect_loop("ftl_collect_rnn", h, T, out, a.m, a.A, &rb->b, flags, stream,
        [&](bool& is_short, bool& misaligned) {                 // the state blocks beside the feed-forward record
            if (!rb->state) return fail(FTL_E_INVALID, "ftl_rnn_collect_buffers: state missing (at least block 0: the rows decision 0 read)");
            if (rb->state_steps != 1 && rb->state_steps != T) return fail(FTL_E_INVALID, "ftl_rnn_collect_buffers: state_steps must be 1 or T");
            const int64_t S = 2 * (int64_t)a.cell + a.P + 1;
            is_short = rb->state_steps > 1 && rb->state_step_bytes < h->P.n_envs * S * 4;
            misaligned = (((uintptr_t)rb->state) | (uintptr_t)(rb->state_steps > 1 ? rb->state_step_bytes : 0)) & 3;
            return (int)FTL_OK;
        },
        [&] { return rnn_kernel_ready(lds); },
        [&](int32_t t, const ftlmlp::Sample& sm, void* action) {
            a.m.action = action; a.alive = h->ro_alive;
            a.state_rec = t < rb->state_steps ? (float*)((char*)rb->state + (int64_t)t * rb->state_step_bytes) : nullptr;
            hipLaunchKernelGGL(ftlrnn::ftl_rnn_kernel, dim3(grid), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a, sm);
        });
}

int ftl_rnn_forward(const ftl_handle* h, const ftl_rnn* net, int32_t n_blocks, int32_t n, const ftl_rnn_sequence* seq, void* stream) {
    RnnSeq r{"ftl_rnn_forward", "n_blocks beyond 65,535", h, net, n_blocks, n, seq};
    if (int rc = r.open(false)) return rc;
    const int32_t A = r.A, C = r.C;
    if (!seq->head) return fail(FTL_E_INVALID, "ftl_rnn_forward: null argument: seq->head");
    if (int rc = r.blocks()) return rc;
    if (seq->head_block_bytes < (int64_t)n * A * 4 || (seq->head_block_bytes & 3))
        return fail(FTL_E_INVALID, "ftl_rnn_forward: head_block_bytes must be a multiple of 4 of at least one block, n * A * 4");
    if (seq->h && (seq->h_block_bytes < (int64_t)n * C * 4 || (seq->h_block_bytes & 3)))
        return fail(FTL_E_INVALID, "ftl_rnn_forward: h_block_bytes must be a multiple of 4 of at least one block, n * cell * 4");
    if (seq->state_out && (seq->state_at < 0 || seq->state_at >= n_blocks))
        return fail(FTL_E_INVALID, "ftl_rnn_forward: state_at must name a block, 0 <= state_at < n_blocks");
    ftlrnn::Seq a; unsigned grid;
    rnn_fill(net, n, a.m, a.u_stride, a.h_stride, grid);
    if ((uint64_t)grid * FTL_MLP_THREADS > 0xFFFFFFFFull)       // (a grid dimension counts threads in 32 bits: 2^24 tiles, over 5e8 rows a block)
        return fail(FTL_E_UNSUPPORTED, "ftl_rnn_forward: n beyond the 2^24 - 1 tiles of one launch; split the rows");
    if (int rc = r.aligned()) return rc;
    if (((uintptr_t)seq->h) & 3) return fail(FTL_E_INVALID, "ftl_rnn_forward: h must be 4-byte aligned");
    if (((uintptr_t)seq->state_out) & 3) return fail(FTL_E_INVALID, "ftl_rnn_forward: state_out must be 4-byte aligned");
    if (((uintptr_t)seq->head) & 3) return fail(FTL_E_INVALID, "ftl_rnn_forward: head must be 4-byte aligned");
    const size_t lds = rnn_lds_bytes(a.m.act_stride, a.u_stride, a.h_stride);
    if (int rc = set_device(h)) return rc;
    if (int rc = rnn_kernel_ready(lds, (const void*)ftlrnn::ftl_rnn_forward_kernel)) return rc;
    r.fill(a);
    a.state_at = seq->state_out ? seq->state_at : -1; a.head_bb = seq->head_block_bytes; a.h_bb = seq->h_block_bytes;
    a.head = seq->head; a.h = seq->h; a.state_out = seq->state_out;
    hipLaunchKernelGGL(ftlrnn::ftl_rnn_forward_kernel, dim3(grid), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a);
    return launched();
}

size_t ftl_sizeof_rnn_gradient(void) { return sizeof(ftl_rnn_gradient); }

int64_t ftl_sizeof_rnn_backward_workspace(const ftl_rnn* net, int32_t n_blocks, int32_t n) {
    if (!net || n_blocks < 1 || n < 1 || net->envs_per_set < 1 || net->env_first < 0) return -1;
    const int64_t count = rnn_param_count(net->width, net->n_layers, net->cell, net->flags);
    if (count < 0) return -1;
    return rnn_bwd_workspace_floats(net, rnn_bwd_plan(net, n_blocks, n), n_blocks, n, count) * 4;
}

int ftl_rnn_backward(const ftl_handle* h, const ftl_rnn* net, int32_t n_blocks, int32_t n, const ftl_rnn_sequence* seq, const ftl_rnn_gradient* g,
                     void* stream) {
    RnnSeq r{"ftl_rnn_backward", "n_blocks beyond 65,535 (the limit of ftl_rnn_forward)", h, net, n_blocks, n, seq};
    if (int rc = r.open(!g)) return rc;
    const int32_t Lt = net->n_layers, A = r.A, C = r.C;
    if (!g->dhead) return fail(FTL_E_INVALID, "ftl_rnn_backward: null argument: g->dhead");
    if (!g->grad) return fail(FTL_E_INVALID, "ftl_rnn_backward: null argument: g->grad");
    if (!g->workspace) return fail(FTL_E_INVALID, "ftl_rnn_backward: null argument: g->workspace");
    if (int rc = r.blocks()) return rc;
    if (g->dhead_block_bytes < (int64_t)n * A * 4 || (g->dhead_block_bytes & 3))
        return fail(FTL_E_INVALID, "ftl_rnn_backward: dhead_block_bytes must be a multiple of 4 of at least one block, n * A * 4");
    ftlrnn::Bwd a; unsigned grid;
    rnn_fill(net, n, a.m, a.u_stride, a.h_stride, grid);
    // LDS (include/ftl.h): the hidden buffers, u, dh, the weight stage, and the region that is xs | h' | dy, then dz of a gate pass
    const int32_t cnmax = std::min<int32_t>(C, FTL_RNN_PASS_CELLS);
    a.dz_stride = 4 * cnmax + 2;
    size_t stage = FTL_MLP_W_STAGE + 64;
    for (int l = 1; l <= Lt + 1; l++) {
        const int w = l <= Lt ? net->width[l] : 4 * cnmax;
        stage = std::max(stage, (size_t)ftlmlp::chunk_rows(w) * ftlmlp::bwd_stride(w));
    }
    if (C > FTL_RNN_PASS_CELLS && C % FTL_RNN_PASS_CELLS) {      // (the second pass of a cell that is no multiple of the pass)
        const int w = 4 * (C - FTL_RNN_PASS_CELLS);
        stage = std::max(stage, (size_t)ftlmlp::chunk_rows(w) * ftlmlp::bwd_stride(w));
    }
    a.stage = (int32_t)stage;
    const size_t region = std::max<size_t>(a.dz_stride, ftlmlp::XS + a.h_stride + ftlmlp::dy_stride(A));
    const size_t lds = ((size_t)FTL_MLP_ENV_TILE * ((size_t)(Lt - 1) * a.m.act_stride + a.u_stride + a.h_stride + region) + stage) * sizeof(float);
    if (lds > 160 * 1024) return fail(FTL_E_UNSUPPORTED, "ftl_rnn_backward: the net needs more than the 160 KiB of LDS of a workgroup (FTL_RNN_BWD limits)");
    const RnnBwdPlan p = rnn_bwd_plan(net, n_blocks, n);
    if ((uint64_t)grid * FTL_MLP_THREADS > 0xFFFFFFFFull || (uint64_t)p.spans * FTL_MLP_THREADS > 0xFFFFFFFFull)
        return fail(FTL_E_UNSUPPORTED, "ftl_rnn_backward: n beyond the 2^24 - 1 tiles of a block, or beyond 2^24 - 1 spans in all; split the rows");
    const int64_t count = rnn_param_count(net->width, Lt, C, net->flags);
    if (g->workspace_bytes < rnn_bwd_workspace_floats(net, p, n_blocks, n, count) * 4)
        return fail(FTL_E_INVALID, "ftl_rnn_backward: workspace_bytes below ftl_sizeof_rnn_backward_workspace");
    if (int rc = r.aligned()) return rc;
    if (((uintptr_t)g->dhead) & 3) return fail(FTL_E_INVALID, "ftl_rnn_backward: dhead must be 4-byte aligned");
    if (((uintptr_t)g->dstate_in) & 3) return fail(FTL_E_INVALID, "ftl_rnn_backward: dstate_in must be 4-byte aligned");
    if (((uintptr_t)g->dstate_out) & 3) return fail(FTL_E_INVALID, "ftl_rnn_backward: dstate_out must be 4-byte aligned");
    if (((uintptr_t)g->workspace) & 3) return fail(FTL_E_INVALID, "ftl_rnn_backward: workspace must be 4-byte aligned");
    if (((uintptr_t)g->grad) & 3) return fail(FTL_E_INVALID, "ftl_rnn_backward: grad must be 4-byte aligned");
    if (int rc = set_device(h)) return rc;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)ftlrnn::ftl_rnn_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipFuncSetAttribute(ftl_rnn_backward_kernel): ") + hipGetErrorString(e));
    }
    r.fill(a);
    a.G = (int32_t)p.G; a.spg = (int32_t)p.spg;
    a.groups0 = (int32_t)p.groups0; a.groups_mid = (int32_t)p.groups_mid; a.spans0 = (int32_t)p.spans0; a.spans_mid = (int32_t)p.spans_mid;
    a.dy_bb = g->dhead_block_bytes;
    a.dy = g->dhead; a.dstate_in = g->dstate_in; a.dstate_out = g->dstate_out;
    a.part = static_cast<float*>(g->workspace); a.count = count;
    a.rec = a.part + p.spans * count;
    a.carry = a.rec + (int64_t)n_blocks * n * 2 * C;
    hipLaunchKernelGGL(ftlrnn::ftl_rnn_backward_kernel, dim3((unsigned)p.groups), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a);
    const ftlmlp::Reduce rd{a.part, g->grad, count, net->set_stride, (int32_t)(net->env_first / net->envs_per_set),
                            (int32_t)p.n_touched, (int32_t)p.spans0, (int32_t)p.spans_mid, (int32_t)p.spans_last};
    hipLaunchKernelGGL(ftlmlp::ftl_mlp_backward_reduce_kernel, dim3((unsigned)p.n_touched, (unsigned)((count + FTL_MLP_THREADS - 1) / FTL_MLP_THREADS)),
                       dim3(FTL_MLP_THREADS), 0, (hipStream_t)stream, rd);
    return launched();
}

}  // extern "C"
