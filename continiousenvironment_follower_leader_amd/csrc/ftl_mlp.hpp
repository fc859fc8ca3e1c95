// ftl_mlp.hpp -- a dense feed-forward policy, or a population of them (one weight set per block of envs), on the device: the forward
// pass from every env's policy_obs row to its encoded action (ftl_mlp_act) and T closed-loop steps with one call (ftl_rollout_mlp); the
// numerics contract is in include/ftl.h.  Included by ftl_abi.hip after ftl_baseline.hpp (same translation unit: it reads the handle,
// shares the handle's action scratch with the baseline and hands its act kernel to rollout_loop, which owns the steps and the fold).
//
// ftl_mlp_kernel: one workgroup of 256 threads per tile of up to FTL_MLP_ENV_TILE envs of ONE weight set (a tile ends at a set
// boundary), all layers in one launch.  The activations of the tile stay in LDS between the layers ([env][act_stride] floats); nothing
// but the input row and the action touches global memory per env.  A layer's weights are staged in LDS in chunks of kc input rows,
// kc = min(FTL_MLP_K_CHUNK, FTL_MLP_W_STAGE / w_out) rounded down to a multiple of 4, and with them, for the first layer, the same kc
// columns of the tile's policy_obs rows.  The products go through v_mfma_f32_16x16x4_f32: a wave owns FTL_MLP_ENVS_PER_WAVE envs (wave & 1
// picks the half of the tile) and every second block of FTL_MLP_NEURON_BLOCK neurons (wave >> 1 picks the parity), the accumulator tile of
// a block starts at the bias (the C operand), and one instruction advances all 256 chains of the block by 4 k in ascending order -- on
// this hardware bit for bit the fmaf chain of the contract: tests/test_gpu_mlp.py pins it to the twin, on random nets and on rows built so
// that a tie decided by the third operand and subnormal operands, sums and results reach the action (test_act_keeps_ties_and_subnormals).  The k left
// over when a layer's input width is no multiple of 4 are plain fmaf on the same accumulators.  Per 4 k a wave reads one x and one
// weight per lane and block from LDS.  Rows past the tile's last env and columns past w_out compute on whatever the stage holds: an MFMA
// output depends on its own row and column only, and they are never stored.
//
// ftl_mlp_tanh_kernel and ftl_mlp_sample_tanh_kernel are the same body with the other hidden activation of include/ftl.h (ftl_mlp.activation):
// mlp_body<SAMPLE, ACT> differs in the hidden layers' epilogue only, tanh32 of csrc/ftl_rnn_math.hpp on every accumulator value instead of
// the ReLU select.  ACT is a compile-time constant, so the ReLU kernels are the instantiations they were (same code, same resource rows:
// profiles/mlp_tanh_kernel_resources.txt); grid, LDS plan, tiling and MFMA path are shared.  mlp_launch picks the kernel from the net.
//
// ftl_mlp_sample_kernel is the same body (mlp_body<true, ..>) with three optional additions, each a pointer of ftlmlp::Sample: the threads that
// stage a chunk of the tile's policy_obs rows store the same floats to obs_rec (the row is read from HBM once and written once), the raw
// head outputs go to head_rec before any map, and the head map adds the caller's noise (include/ftl.h: ftl_mlp_sample).  ftl_collect_mlp
// plays T such decisions through episode boundaries and records a trajectory (ftl_collect_record_kernel); ftl_gae_kernel turns its rewards
// and kinds and the caller's values into advantages.
//
// ftl_mlp_forward_kernel and ftl_mlp_forward_tanh_kernel evaluate the net on rows the caller supplies (include/ftl.h: ftl_mlp_forward):
// mlp_body<false, ACT, true>, the same tile plan, LDS plan, weight staging and MFMA path, with three differences, each behind the
// compile-time FORWARD: blockIdx.y names a block of n rows and the first layer stages its input from obs + blockIdx.y * x_block_bytes
// (64-bit byte offsets), the tile map runs over the n rows of a block (Args.n_envs = n, set on the host), and the epilogue stores the raw
// head -- the tile's rows are one contiguous run of tile_n * width[L] floats of y, written by all 256 threads in order -- and has no
// action map.  The additions travel in ftlmlp::Forward, as the sampling ones do in Sample; Args is what it was, and so are the four
// kernels above (profiles/mlp_forward_kernel_resources.txt).
//
// Weight traffic: a tile reads its set once from L2, ftl_mlp_param_count * 4 bytes per FTL_MLP_ENV_TILE envs (about 2 KB per env for
// 180-64-64-2), against the whole set per env of a wave-per-env form.
#include <hip/hip_runtime.h>
#include "ftl_rnn_math.hpp"

#define FTL_MLP_ENV_TILE 32           // envs of one workgroup
#define FTL_MLP_K_CHUNK 64            // input rows of a layer staged at a time, at most
#define FTL_MLP_W_STAGE 4096          // floats of the weight stage: a chunk is kc rows of w_out floats, kc * w_out <= this
#define FTL_MLP_ENVS_PER_WAVE 16      // rows of an MFMA tile
#define FTL_MLP_NEURON_BLOCK 16       // columns of an MFMA tile
#define FTL_MLP_THREADS 256

namespace ftlmlp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TILE = FTL_MLP_ENV_TILE, KC = FTL_MLP_K_CHUNK, EPW = FTL_MLP_ENVS_PER_WAVE, NB = FTL_MLP_NEURON_BLOCK, WAVES = FTL_MLP_THREADS / 64;
constexpr int GROUPS = TILE / EPW, PARITIES = WAVES / GROUPS;           // env groups of a tile; waves that share a group's neuron blocks
constexpr int BPW = FTL_MLP_MAX_WIDTH / NB / PARITIES;                  // neuron blocks of a wave, at most
constexpr int XS = KC + 2;             // row stride of the staged input chunk, and act_stride % 32 == 2 too: 16 rows x 2 k hit 32 banks
static_assert(EPW == 16 && NB == 16 && GROUPS * PARITIES == WAVES && BPW * PARITIES * NB == FTL_MLP_MAX_WIDTH &&
              FTL_MLP_W_STAGE / FTL_MLP_MAX_WIDTH >= 4 && KC % 4 == 0 && TILE * 8 == FTL_MLP_THREADS, "staging sizes");

struct Args {
    const float* obs;          // policy_obs: [n_envs][width[0]]
    const float* params; int64_t set_stride;
    int32_t n_envs, n_layers, width[FTL_MLP_MAX_LAYERS + 1], env_first, envs_per_set;
    int32_t len0, tiles0, tiles_per_set;       // tile -> (set, envs): envs of the first (possibly cut) set, its tiles, the tiles of a whole set
    int32_t act_stride;        // floats per env row of the activations in LDS: the widest of width[1 ..] rounded up to 32, plus 2
    int32_t head;              // FTL_ACTION_*
    double lo0, hi0, lo1, hi1;
    void* action;
};

__host__ __device__ inline int chunk_rows(int w_out) {
    const int by_stage = FTL_MLP_W_STAGE / w_out;
    return (by_stage < KC ? by_stage : KC) & ~3;
}

struct Sample {               // what ftl_mlp_sample_kernel adds to ftl_mlp_kernel; every pointer may be null
    const float* noise;       // [n_envs][width[L]]
    const float* sigma;       // [n_sets][width[L]] (Box heads)
    float* head_rec;          // [n_envs][width[L]]: y before any map
    float* obs_rec;           // [n_envs][width[0]]: the policy_obs rows as the first layer staged them
};

struct Forward {              // what the ftl_mlp_forward kernels add: Args.obs is x, Args.n_envs the rows of a block, blockIdx.y the block
    int64_t x_block_bytes;    // block b of the input rows at (char*)obs + b * x_block_bytes
    float* y;                 // block b of the raw heads, [n][width[L]], at (char*)y + b * y_block_bytes
    int64_t y_block_bytes;
};

__device__ __forceinline__ double box_map(double z, double lo, double hi) {
    const double u = fmin(fmax(z, -1.0), 1.0);
    const double s = (u + 1.0) * 0.5;
    const double w = hi - lo;
    const double a = lo + s * w;
    return fmin(fmax(a, lo), hi);
}

__device__ __forceinline__ double box_head(float y, double lo, double hi) { return box_map((double)y, lo, hi); }

// z = y + sigma * noise: the product of two float32 is exact in float64, the sum is the one rounding
__device__ __forceinline__ double box_sample(float y, float sigma, float noise, double lo, double hi) {
    const double p = (double)sigma * (double)noise;
    return box_map((double)y + p, lo, hi);
}

template <bool SAMPLE, int ACT, bool FORWARD = false>
__device__ __forceinline__ void mlp_body(const Args& a, const Sample& sm, const Forward& fw = Forward{}) {
    extern __shared__ float4 mlp_lds[];
    float* act = reinterpret_cast<float*>(mlp_lds);            // [TILE][act_stride]
    float* xs = act + TILE * a.act_stride;                      // [TILE][XS]: a chunk of the input rows (first layer)
    float* ws = xs + TILE * XS;                                 // [kc][w_out]: a chunk of the layer's weights (+ 64 floats never used)
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int g = wave % GROUPS, par = wave / GROUPS;
    const int row_a = g * EPW + li;                             // the env whose x this lane feeds to the MFMA (A[i = lane & 15][k = lane >> 4])
    const int row_d = g * EPW + 4 * lk;                         // the first of the 4 envs whose results it holds (D[4 * (lane >> 4) + r][lane & 15])
    // the tile's set and envs
    int set = a.env_first / a.envs_per_set, start, end;
    if ((int)blockIdx.x < a.tiles0) { start = (int)blockIdx.x * TILE; end = a.len0; }
    else {
        const int b = (int)blockIdx.x - a.tiles0, m = b / a.tiles_per_set;
        const int64_t seg = (int64_t)a.len0 + (int64_t)m * a.envs_per_set, seg_end = seg + a.envs_per_set;
        set += 1 + m;
        start = (int)seg + (b % a.tiles_per_set) * TILE;
        end = seg_end < (int64_t)a.n_envs ? (int)seg_end : a.n_envs;
    }
    const int tile_n = end - start < TILE ? end - start : TILE;
    const bool busy = g * EPW < tile_n;                         // this wave has envs
    const float* P = a.params + (int64_t)set * a.set_stride;
    const int w0 = a.width[0];
    const float* obs = a.obs;
    if (FORWARD) obs = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.obs) + (int64_t)blockIdx.y * fw.x_block_bytes);
    for (int l = 0; l < a.n_layers; l++) {
        const int w_in = a.width[l], w_out = a.width[l + 1], nblk = (w_out + NB - 1) / NB;
        const float* W = P;
        const float* bias = W + (size_t)w_in * w_out;
        P = bias + w_out;
        f32x4 acc[BPW];
#pragma unroll
        for (int m = 0; m < BPW; m++) {
            const int j = (par + PARITIES * m) * NB + li;
            const float b = j < w_out ? bias[j] : 0.0f;
            acc[m] = f32x4{b, b, b, b};
        }
        const int kc = chunk_rows(w_out);
        const int xstride = l == 0 ? XS : a.act_stride;
        for (int k0 = 0; k0 < w_in; k0 += kc) {
            const int kn = w_in - k0 < kc ? w_in - k0 : kc;
            __syncthreads();                                    // the chunk before this one has been read (and, k0 == 0, the layer before written)
            for (int idx = t; idx < kn * w_out; idx += FTL_MLP_THREADS) ws[idx] = W[(size_t)k0 * w_out + idx];
            if (l == 0) {
                const int e = t >> 3;                           // 8 threads per env of the tile
                if (e < tile_n) {
                    const size_t row = (size_t)(start + e) * w0 + k0;
                    if (SAMPLE && sm.obs_rec)
                        for (int kk = t & 7; kk < kn; kk += 8) { const float v = obs[row + kk]; xs[e * XS + kk] = v; sm.obs_rec[row + kk] = v; }
                    else
                        for (int kk = t & 7; kk < kn; kk += 8) xs[e * XS + kk] = obs[row + kk];
                }
            }
            __syncthreads();
            if (!busy) continue;
            const float* x = l == 0 ? xs : act + k0;
            const float* xa = x + row_a * xstride + lk;
            const float* xd = x + row_d * xstride;
            int kk = 0;
            for (; kk + 4 <= kn; kk += 4) {
                const float av = xa[kk];
                const float* wrow = ws + (kk + lk) * w_out + li;          // B[k = lane >> 4][j = lane & 15]; columns past w_out read on into the stage
#pragma unroll
                for (int m = 0; m < BPW; m++) {
                    const int jb = par + PARITIES * m;
                    if (jb < nblk) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wrow[jb * NB], acc[m], 0, 0, 0);      // (wave-uniform)
                }
            }
            for (; kk < kn; kk++) {                              // w_in % 4 rows at the layer's end
#pragma unroll
                for (int m = 0; m < BPW; m++) {
                    const int jb = par + PARITIES * m;
                    if (jb >= nblk) continue;
                    const float w = ws[kk * w_out + jb * NB + li];
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[m][r] = __builtin_fmaf(xd[r * xstride + kk], w, acc[m][r]);
                }
            }
        }
        __syncthreads();                                        // every wave has read this layer's input
        const bool hidden = l + 1 < a.n_layers;
        if (ACT == FTL_MLP_ACT_TANH && hidden) {                // (block-uniform; the head layer takes the loop below, whose select then is v)
#pragma unroll
            for (int m = 0; m < BPW; m++) {
                const int j = (par + PARITIES * m) * NB + li;
                if (j >= w_out) continue;
#pragma unroll
                for (int r = 0; r < 4; r++) act[(row_d + r) * a.act_stride + j] = ftlrnnmath::tanh32(acc[m][r]);
            }
            continue;
        }
#pragma unroll
        for (int m = 0; m < BPW; m++) {
            const int j = (par + PARITIES * m) * NB + li;
            if (j >= w_out) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float v = acc[m][r];
                act[(row_d + r) * a.act_stride + j] = hidden ? (v > 0.0f ? v : 0.0f) : v;
            }
        }
    }
    __syncthreads();
    if (FORWARD) {                                              // the raw head rows of the tile: tile_n * width[L] consecutive floats of the block
        const int wl = a.width[a.n_layers];
        float* y = reinterpret_cast<float*>(reinterpret_cast<char*>(fw.y) + (int64_t)blockIdx.y * fw.y_block_bytes) + (size_t)start * wl;
        for (int idx = t; idx < tile_n * wl; idx += FTL_MLP_THREADS) {
            const int r = idx / wl;
            y[idx] = act[r * a.act_stride + (idx - r * wl)];
        }
        return;
    }
    if (t >= tile_n) return;
    const float* y = act + t * a.act_stride;
    const size_t e = (size_t)start + t;
    if (SAMPLE) {
        const int wl = a.width[a.n_layers];
        if (sm.head_rec)
            for (int j = 0; j < wl; j++) sm.head_rec[e * wl + j] = y[j];
        if (sm.noise) {
            const float* nz = sm.noise + e * wl;
            if (a.head == FTL_ACTION_DISCRETE) {                // s_j = y_j + noise_j in float64; the first maximum, a NaN never beats anything
                int k = 0;
                double best = (double)y[0] + (double)nz[0];
                for (int j = 1; j < 5; j++) {
                    const double sj = (double)y[j] + (double)nz[j];
                    if (sj > best) { best = sj; k = j; }
                }
                static_cast<int32_t*>(a.action)[e] = k;
            } else {
                const float* sg = sm.sigma + (size_t)set * wl;
                if (a.head == FTL_ACTION_BOX2) {
                    static_cast<double*>(a.action)[2 * e] = box_sample(y[0], sg[0], nz[0], a.lo0, a.hi0);
                    static_cast<double*>(a.action)[2 * e + 1] = box_sample(y[1], sg[1], nz[1], a.lo1, a.hi1);
                } else static_cast<double*>(a.action)[e] = box_sample(y[0], sg[0], nz[0], a.lo1, a.hi1);
            }
            return;
        }
    }
    if (a.head == FTL_ACTION_DISCRETE) {
        int k = 0;
        for (int j = 1; j < 5; j++) if (y[j] > y[k]) k = j;
        static_cast<int32_t*>(a.action)[e] = k;
    } else if (a.head == FTL_ACTION_BOX2) {
        static_cast<double*>(a.action)[2 * e] = box_head(y[0], a.lo0, a.hi0);
        static_cast<double*>(a.action)[2 * e + 1] = box_head(y[1], a.lo1, a.hi1);
    } else static_cast<double*>(a.action)[e] = box_head(y[0], a.lo1, a.hi1);
}

__global__ __launch_bounds__(FTL_MLP_THREADS) void ftl_mlp_kernel(const Args a) { mlp_body<false, FTL_MLP_ACT_RELU>(a, Sample{}); }

__global__ __launch_bounds__(FTL_MLP_THREADS) void ftl_mlp_sample_kernel(const Args a, const Sample sm) { mlp_body<true, FTL_MLP_ACT_RELU>(a, sm); }

// (four waves a SIMD asked for: left alone the allocator spreads the 32 unrolled tanh32 of the epilogue over 112 VGPRs beside the 32
// accumulator registers, three waves a SIMD where the ReLU kernels have four; bounded it needs 96 in all, without spill or scratch)
__global__ __launch_bounds__(FTL_MLP_THREADS, 4) void ftl_mlp_tanh_kernel(const Args a) { mlp_body<false, FTL_MLP_ACT_TANH>(a, Sample{}); }

__global__ __launch_bounds__(FTL_MLP_THREADS, 4) void ftl_mlp_sample_tanh_kernel(const Args a, const Sample sm) { mlp_body<true, FTL_MLP_ACT_TANH>(a, sm); }

__global__ __launch_bounds__(FTL_MLP_THREADS) void ftl_mlp_forward_kernel(const Args a, const Forward fw) { mlp_body<false, FTL_MLP_ACT_RELU, true>(a, Sample{}, fw); }

__global__ __launch_bounds__(FTL_MLP_THREADS, 4) void ftl_mlp_forward_tanh_kernel(const Args a, const Forward fw) { mlp_body<false, FTL_MLP_ACT_TANH, true>(a, Sample{}, fw); }

// ---- the backward pass of the net on recorded rows (include/ftl.h: ftl_mlp_backward) ---------------------------------------------------
// ftl_mlp_backward_kernel / ftl_mlp_backward_tanh_kernel: one workgroup per SPAN of FTL_MLP_BWD_SPAN tiles of one set (the forward tile
// map, the set's tiles enumerated block-major), the tiles one after the other.  Per tile: the hidden layers are recomputed with the loop of
// mlp_body (same chunks, same MFMA order: the same bits), every hidden activation of the tile kept in LDS -- buffer l - 1 holds h_l
// [TILE][act_stride] with a 1.0 in column width[l], the bias's input --, dy is staged into a buffer of its own, and for l = L .. 1 the weight
// gradient takes h_{l-1}^T delta_l through the MFMA with K = the tile's 32 row slots and the span's running partial as the C operand, then
// delta_{l-1} = (delta_l W_l^T) * act' through the MFMA with K = width[l] overwrites h_{l-1} in place (its only later reader is the element's
// own derivative).  The running partial lives in the span's slice of the workspace, in the layout of a weight set: every lane loads the
// four words of its accumulator tile, advances them by the tile's rows and stores them -- the same lane the same words on every tile, so
// program order is all the ordering it needs and no workgroup ever reads another's.  The first tile of a span starts from +0 instead of a
// load: the workspace needs no clearing.  Row slots past a cut tile's end feed +0 to both MFMA operands (a select on the row, not the
// buffers' contents).  ftl_mlp_backward_reduce_kernel then sums a set's span partials in float64, ascending, one thread a word.
struct Backward {
    int64_t x_block_bytes;
    const float* dy; int64_t dy_block_bytes;       // block b of the head gradients, [n][width[L]], at (char*)dy + b * dy_block_bytes
    float* ws; int64_t count;                      // the span partials, [spans][count] floats; count = ftl_mlp_param_count
    int32_t n_blocks, spans0, spans_mid;           // spans of the first touched set and of a whole set (the divisor of the span -> set map)
};

struct Reduce {
    const float* ws; float* grad; int64_t count, set_stride;
    int32_t set0, n_touched, spans0, spans_mid, spans_last;     // spans_last: of the last touched set when it is not the first
};

constexpr int BSPAN = FTL_MLP_BWD_SPAN, DWB = 4;   // accumulator tiles of the weight gradient a wave advances together

// Row strides of the backward kernels' weight stage, chosen for the LDS banks (the values staged are the forward's): the forward product
// reads B[k = lane >> 4][j = lane & 15], 16 consecutive floats of 4 rows -- a stride of 16 mod 32 puts the 64 lanes two to a bank --; the
// delta product reads the transpose, B[j = lane >> 4][k = lane & 15] = W[k][j], 4 consecutive floats of 16 rows -- a stride of 4 mod 32.
__host__ __device__ inline int fwd_stride(int w_out) { return ((w_out + 15) & ~31) + 16; }
__host__ __device__ inline int bwd_stride(int w_out) { return ((w_out + 27) & ~31) + 4; }
__host__ __device__ inline int dy_stride(int wl) { return ((wl + 31) & ~31) + 2; }      // act_stride's rule for the head alone

// ws[kk * stride + j] = W[kk * w_out + j] for kk < kn, j < w_out, by all threads, without a division per element
__device__ __forceinline__ void stage_rows(float* ws, int stride, const float* W, int kn, int w_out, int t) {
    const int dk = FTL_MLP_THREADS / w_out, dj = FTL_MLP_THREADS - dk * w_out, n = kn * w_out;
    int kk = t / w_out, j = t - kk * w_out;
    for (int idx = t; idx < n; idx += FTL_MLP_THREADS) {
        ws[kk * stride + j] = W[idx];
        kk += dk; j += dj;
        if (j >= w_out) { j -= w_out; kk++; }
    }
}

// C += src^T delta over the tile's row slots, for the kn input columns [k0, k0 + kn) of a layer whose gradient matrix [w_in + 1][w_out]
// starts at G: src holds the columns at [row][0 .. kn) with stride sstride, delta [row][w_out] with stride dstride
__device__ __forceinline__ void dw_blocks(const float* src, int sstride, int k0, int kn, const float* delta, int dstride, int w_out,
                                          float* G, bool first, int tile_n, int wave, int li, int lk) {
    const int nkb = (kn + NB - 1) / NB, njb = (w_out + NB - 1) / NB, total = nkb * njb;
    for (int q0 = wave * DWB; q0 < total; q0 += WAVES * DWB) {
        f32x4 c[DWB];
        int kb[DWB], jb[DWB];
#pragma unroll
        for (int u = 0; u < DWB; u++) {
            const int q = q0 + u < total ? q0 + u : total - 1;
            kb[u] = q / njb; jb[u] = q - kb[u] * njb;
            const int j = jb[u] * NB + li;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int k = kb[u] * NB + 4 * lk + r;
                c[u][r] = (!first && q0 + u < total && k < kn && j < w_out) ? G[(size_t)(k0 + k) * w_out + j] : 0.0f;
            }
        }
        for (int rr = 0; rr < TILE; rr += 4) {
            const int row = rr + lk;
            const bool live = row < tile_n;
#pragma unroll
            for (int u = 0; u < DWB; u++) {
                if (q0 + u >= total) continue;                  // (wave-uniform)
                const int k = kb[u] * NB + li, j = jb[u] * NB + li;
                const float av = (live && k < kn) ? src[row * sstride + k] : 0.0f;
                const float bv = (live && j < w_out) ? delta[row * dstride + j] : 0.0f;
                c[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c[u], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < DWB; u++) {
            if (q0 + u >= total) continue;
            const int j = jb[u] * NB + li;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int k = kb[u] * NB + 4 * lk + r;
                if (k < kn && j < w_out) G[(size_t)(k0 + k) * w_out + j] = c[u][r];
            }
        }
    }
}

template <int ACT>
__device__ __forceinline__ void mlp_bwd_body(const Args& a, const Backward& bw) {
    extern __shared__ float4 mlp_lds[];
    const int L = a.n_layers, AS = a.act_stride;
    const int DS = dy_stride(a.width[L]);
    float* hb = reinterpret_cast<float*>(mlp_lds);             // [L - 1][TILE][AS]: buffer l - 1 is h_l, then delta_l
    float* dyb = hb + (L - 1) * TILE * AS;                      // [TILE][DS]: dy
    float* xs = dyb + TILE * DS;                                // [TILE][XS]
    float* ws = xs + TILE * XS;                                 // the weight stage: bwd_stage_floats of the host
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int g = wave % GROUPS, par = wave / GROUPS;
    const int row_a = g * EPW + li, row_d = g * EPW + 4 * lk;
    // the span's set, its rows of a block and its tiles
    int m, sp;
    if ((int)blockIdx.x < bw.spans0) { m = 0; sp = (int)blockIdx.x; }
    else { const int q = (int)blockIdx.x - bw.spans0; m = 1 + q / bw.spans_mid; sp = q % bw.spans_mid; }
    const int set = a.env_first / a.envs_per_set + m;
    int seg, seg_end;
    if (m == 0) { seg = 0; seg_end = a.len0; }
    else {
        const int64_t s0 = (int64_t)a.len0 + (int64_t)(m - 1) * a.envs_per_set, s1 = s0 + a.envs_per_set;
        seg = (int)s0; seg_end = s1 < (int64_t)a.n_envs ? (int)s1 : a.n_envs;
    }
    const int set_tiles = (seg_end - seg + TILE - 1) / TILE;
    const int64_t all_tiles = (int64_t)set_tiles * bw.n_blocks, tile0 = (int64_t)sp * BSPAN;
    const int n_tiles = all_tiles - tile0 < BSPAN ? (int)(all_tiles - tile0) : BSPAN;
    const float* P = a.params + (int64_t)set * a.set_stride;
    float* G = bw.ws + (int64_t)blockIdx.x * bw.count;
    const int w0 = a.width[0], wl = a.width[L];
    int off[FTL_MLP_MAX_LAYERS + 1];
    off[0] = 0;
#pragma unroll
    for (int l = 0; l < FTL_MLP_MAX_LAYERS; l++) off[l + 1] = off[l] + (l < L ? (a.width[l] + 1) * a.width[l + 1] : 0);
    for (int ti = 0; ti < n_tiles; ti++) {
        const int64_t gt = tile0 + ti;
        const int blk = (int)(gt / set_tiles), start = seg + (int)(gt - (int64_t)blk * set_tiles) * TILE;
        const int tile_n = seg_end - start < TILE ? seg_end - start : TILE;
        const bool busy = g * EPW < tile_n, first = ti == 0;
        const float* obs = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.obs) + (int64_t)blk * bw.x_block_bytes);
        const float* dy = reinterpret_cast<const float*>(reinterpret_cast<const char*>(bw.dy) + (int64_t)blk * bw.dy_block_bytes) + (size_t)start * wl;
        __syncthreads();                                        // the tile before this one has been read
        for (int idx = t; idx < TILE * wl; idx += FTL_MLP_THREADS) {
            const int r = idx / wl;
            dyb[r * DS + (idx - r * wl)] = r < tile_n ? dy[idx] : 0.0f;
        }
        // the hidden layers, as mlp_body computes them
        for (int l = 0; l + 1 < L; l++) {
            const int w_in = a.width[l], w_out = a.width[l + 1], nblk = (w_out + NB - 1) / NB;
            const float* W = P + off[l];
            const float* bias = W + (size_t)w_in * w_out;
            float* out = hb + l * TILE * AS;
            f32x4 acc[BPW];
#pragma unroll
            for (int mm = 0; mm < BPW; mm++) {
                const int j = (par + PARITIES * mm) * NB + li;
                const float b = j < w_out ? bias[j] : 0.0f;
                acc[mm] = f32x4{b, b, b, b};
            }
            const int kc = chunk_rows(w_out), wsf = fwd_stride(w_out);
            const int xstride = l == 0 ? XS : AS;
            for (int k0 = 0; k0 < w_in; k0 += kc) {
                const int kn = w_in - k0 < kc ? w_in - k0 : kc;
                __syncthreads();
                stage_rows(ws, wsf, W + (size_t)k0 * w_out, kn, w_out, t);
                if (l == 0) {
                    const int e = t >> 3;
                    if (e < tile_n) {
                        const size_t row = (size_t)(start + e) * w0 + k0;
                        for (int kk = t & 7; kk < kn; kk += 8) xs[e * XS + kk] = obs[row + kk];
                    }
                }
                __syncthreads();
                if (!busy) continue;
                const float* x = l == 0 ? xs : hb + (l - 1) * TILE * AS + k0;
                const float* xa = x + row_a * xstride + lk;
                const float* xd = x + row_d * xstride;
                int kk = 0;
                for (; kk + 4 <= kn; kk += 4) {
                    const float av = xa[kk];
                    const float* wrow = ws + (kk + lk) * wsf + li;
#pragma unroll
                    for (int mm = 0; mm < BPW; mm++) {
                        const int jb = par + PARITIES * mm;
                        if (jb < nblk) acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wrow[jb * NB], acc[mm], 0, 0, 0);
                    }
                }
                for (; kk < kn; kk++) {
#pragma unroll
                    for (int mm = 0; mm < BPW; mm++) {
                        const int jb = par + PARITIES * mm;
                        if (jb >= nblk) continue;
                        const float w = ws[kk * wsf + jb * NB + li];
#pragma unroll
                        for (int r = 0; r < 4; r++) acc[mm][r] = __builtin_fmaf(xd[r * xstride + kk], w, acc[mm][r]);
                    }
                }
            }
#pragma unroll
            for (int mm = 0; mm < BPW; mm++) {
                const int j = (par + PARITIES * mm) * NB + li;
                if (j >= w_out) continue;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float v = acc[mm][r];
                    out[(row_d + r) * AS + j] = ACT == FTL_MLP_ACT_TANH ? ftlrnnmath::tanh32(v) : (v > 0.0f ? v : 0.0f);
                }
            }
            if (t < TILE) out[t * AS + w_out] = 1.0f;            // the bias's input
        }
        // the gradients, from the head down
        for (int l = L; l >= 1; l--) {
            const int w_in = a.width[l - 1], w_out = a.width[l];
            const float* delta = hb + (l - 1) * TILE * AS;      // dy for l == L
            const int dst = l == L ? DS : AS;
            float* Gl = G + off[l - 1];
            if (l == 1) {
                for (int k0 = 0; k0 < w0 + 1; k0 += KC) {
                    const int kn = w0 + 1 - k0 < KC ? w0 + 1 - k0 : KC;
                    __syncthreads();
                    const int e = t >> 3;
                    if (e < tile_n) {
                        const size_t row = (size_t)(start + e) * w0;
                        for (int kk = t & 7; kk < kn; kk += 8) xs[e * XS + kk] = k0 + kk < w0 ? obs[row + k0 + kk] : 1.0f;
                    }
                    __syncthreads();
                    dw_blocks(xs, XS, k0, kn, delta, dst, w_out, Gl, first, tile_n, wave, li, lk);
                }
                break;
            }
            float* hprev = hb + (l - 2) * TILE * AS;            // h_{l-1}, with its 1.0 in column w_in
            __syncthreads();
            dw_blocks(hprev, AS, 0, w_in + 1, delta, dst, w_out, Gl, first, tile_n, wave, li, lk);
            // delta_{l-1}[r][k] = (the chain over j of W_l[k][j] * delta_l[r][j]) * act'(h_{l-1}[r][k]), in place of h_{l-1}
            const float* W = P + off[l - 1];
            const int kc = chunk_rows(w_out), wst = bwd_stride(w_out);
            for (int k0 = 0; k0 < w_in; k0 += kc) {
                const int kn = w_in - k0 < kc ? w_in - k0 : kc, nkb = (kn + NB - 1) / NB;
                __syncthreads();
                stage_rows(ws, wst, W + (size_t)k0 * w_out, kn, w_out, t);
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
                        const float w = wr[mm][j];
#pragma unroll
                        for (int r = 0; r < 4; r++) acc[mm][r] = __builtin_fmaf(w, delta[(row_d + r) * dst + j], acc[mm][r]);
                    }
                }
#pragma unroll
                for (int mm = 0; mm < 2; mm++) {
                    const int k = (par + PARITIES * mm) * NB + li;
                    if (k >= kn) continue;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float* p = hprev + (row_d + r) * AS + k0 + k;
                        const float h = *p, v = acc[mm][r];
                        if (ACT == FTL_MLP_ACT_TANH) *p = v * __builtin_fmaf(-h, h, 1.0f);
                        else *p = h > 0.0f ? v : 0.0f;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(FTL_MLP_THREADS, 3) void ftl_mlp_backward_kernel(const Args a, const Backward bw) { mlp_bwd_body<FTL_MLP_ACT_RELU>(a, bw); }

__global__ __launch_bounds__(FTL_MLP_THREADS, 3) void ftl_mlp_backward_tanh_kernel(const Args a, const Backward bw) { mlp_bwd_body<FTL_MLP_ACT_TANH>(a, bw); }

// grad[set][w] = the float64 sum of the set's span partials in ascending span order, rounded once; blockIdx.x the touched set
__global__ __launch_bounds__(FTL_MLP_THREADS) void ftl_mlp_backward_reduce_kernel(const Reduce rd) {
    const int64_t w = (int64_t)blockIdx.y * FTL_MLP_THREADS + threadIdx.x;
    if (w >= rd.count) return;
    const int m = (int)blockIdx.x;
    const int n = m == 0 ? rd.spans0 : m == rd.n_touched - 1 ? rd.spans_last : rd.spans_mid;
    const int64_t base = m == 0 ? 0 : (int64_t)rd.spans0 + (int64_t)(m - 1) * rd.spans_mid;
    const float* p = rd.ws + base * rd.count + w;
    double s = 0.0;
    for (int j = 0; j < n; j++) s += (double)p[(int64_t)j * rd.count];
    rd.grad[(int64_t)(rd.set0 + m) * rd.set_stride + w] = (float)s;
}

}  // namespace ftlmlp

// floats of one weight set; -1 outside the limits of include/ftl.h
static int64_t mlp_param_count(const int32_t* w, int32_t L) {
    if (!w || L < 1 || L > FTL_MLP_MAX_LAYERS) return -1;
    int64_t n = 0;
    for (int l = 0; l <= L; l++)
        if (w[l] < 1 || w[l] > (l == 0 ? FTL_MLP_MAX_IN : FTL_MLP_MAX_WIDTH)) return -1;
    for (int l = 1; l <= L; l++) n += ((int64_t)w[l - 1] + 1) * w[l];
    return n;
}

static size_t mlp_action_bytes(int32_t head) { return head == FTL_ACTION_BOX2 ? 16 : head == FTL_ACTION_TURN ? 8 : 4; }

// What mlp_net_check and rnn_net_check share; `pre` ("mlp: " / "rnn: ") heads the messages.  The widths width[0 .. last] ...
static int net_widths_check(const char* pre, const int32_t* width, int32_t last) {
    for (int l = 0; l <= last; l++) {
        if (width[l] < 1) return fail(FTL_E_INVALID, std::string(pre) + "every width must be at least 1");
        if (width[l] > (l == 0 ? FTL_MLP_MAX_IN : FTL_MLP_MAX_WIDTH))
            return fail(FTL_E_UNSUPPORTED, std::string(pre) + (l == 0 ? "input width beyond FTL_MLP_MAX_IN" : "layer width beyond FTL_MLP_MAX_WIDTH"));
    }
    return FTL_OK;
}

// ... and the weight sets of an ftl_mlp or ftl_rnn for `n` rows: `count` is the net's parameter count, `counter` the name of its function
template <typename Net>
static int net_sets_check(const char* pre, const Net* net, int64_t count, const char* counter, int64_t n, const char* rows) {
    if (((uintptr_t)net->params) & 3) return fail(FTL_E_INVALID, std::string(pre) + "params must be 4-byte aligned");
    if (net->set_stride < count) return fail(FTL_E_INVALID, std::string(pre) + "set_stride below " + counter);
    if (net->n_sets < 1 || net->envs_per_set < 1 || net->env_first < 0)
        return fail(FTL_E_INVALID, std::string(pre) + "n_sets and envs_per_set must be at least 1, env_first at least 0");
    const int64_t eps = net->envs_per_set, first = net->env_first;
    if ((first + n - 1) / eps >= net->n_sets) return fail(FTL_E_INVALID, std::string(pre) + rows + " lies beyond the last weight set");
    return FTL_OK;
}

// The tile map of `n` rows over the weight sets, which the kernels of both nets decode, forward and backward alike: the rows of the first
// touched set (possibly cut) and of the last one (0: it is whole, or the first is the only one), the whole sets after the first, and the
// tiles of each and of a block in all.  The one place that computes it: mlp_fill, rnn_fill, mlp_bwd_plan and rnn_bwd_plan read it.
struct TileMap { int64_t len0, rem, full, last, tiles0, tiles_per_set, tiles_last, tiles; };
static TileMap tile_map(int64_t env_first, int64_t envs_per_set, int64_t n) {
    const int64_t eps = envs_per_set, tile = FTL_MLP_ENV_TILE;
    TileMap m;
    m.len0 = std::min<int64_t>(n, (env_first / eps + 1) * eps - env_first); m.rem = n - m.len0; m.full = m.rem / eps; m.last = m.rem % eps;
    m.tiles0 = (m.len0 + tile - 1) / tile; m.tiles_per_set = (eps + tile - 1) / tile; m.tiles_last = (m.last + tile - 1) / tile;
    m.tiles = m.tiles0 + m.full * m.tiles_per_set + m.tiles_last;
    return m;
}

// ... into the kernel's arguments; returns the grid's tiles
static unsigned tile_map_fill(const TileMap& m, ftlmlp::Args& a) {
    a.len0 = (int32_t)m.len0; a.tiles0 = (int32_t)m.tiles0; a.tiles_per_set = (int32_t)m.tiles_per_set;
    return (unsigned)m.tiles;
}

// the checks of the net itself, for `n` rows (the handle's envs, or the rows of a block of ftl_mlp_forward: `rows` names them in the last
// message); `any_head` admits every head width of 1 .. FTL_MLP_MAX_WIDTH instead of those of the three action encodings
static int mlp_net_check(const ftl_mlp* net, int64_t n, bool any_head, const char* rows) {
    const int32_t L = net->n_layers;
    if (L < 1) return fail(FTL_E_INVALID, "mlp: n_layers must be at least 1");
    if (L > FTL_MLP_MAX_LAYERS) return fail(FTL_E_UNSUPPORTED, "mlp: more than FTL_MLP_MAX_LAYERS layers");
    if (int rc = net_widths_check("mlp: ", net->width, L)) return rc;
    const int32_t wl = net->width[L];
    if (!any_head && wl != 1 && wl != 2 && wl != 5) return fail(FTL_E_INVALID, "mlp: the head width must be 2 (Box(2)), 1 (Box(1) turn) or 5 (Discrete(5))");
    if (net->activation != FTL_MLP_ACT_RELU && net->activation != FTL_MLP_ACT_TANH)
        return fail(FTL_E_INVALID, "mlp: activation must be FTL_MLP_ACT_RELU (0) or FTL_MLP_ACT_TANH (1)");
    return net_sets_check("mlp: ", net, mlp_param_count(net->width, L), "ftl_mlp_param_count", n, rows);
}

// the kernel's arguments that follow from a checked net and its `n` rows: everything but obs, head, the bounds and `action`; the grid's
// tiles and the LDS bytes
static void mlp_fill(const ftl_mlp* net, int64_t n, ftlmlp::Args& a, unsigned& grid, size_t& lds) {
    const int32_t L = net->n_layers;
    a.params = net->params; a.set_stride = net->set_stride;
    a.n_envs = (int32_t)n; a.n_layers = L; a.env_first = net->env_first; a.envs_per_set = net->envs_per_set;
    int wmax = 0;
    for (int l = 0; l <= FTL_MLP_MAX_LAYERS; l++) {
        a.width[l] = l <= L ? net->width[l] : 0;
        if (l >= 1 && a.width[l] > wmax) wmax = a.width[l];
    }
    a.act_stride = ((wmax + 31) & ~31) + 2;
    grid = tile_map_fill(tile_map(net->env_first, net->envs_per_set, n), a);
    lds = ((size_t)FTL_MLP_ENV_TILE * a.act_stride + (size_t)FTL_MLP_ENV_TILE * ftlmlp::XS + FTL_MLP_W_STAGE + 64) * sizeof(float);
}

// the checks of the net that ftl_mlp_act and ftl_rollout_mlp share (check_ready comes after the caller's own, so that a missing state is the
// last thing reported); fills the kernel's arguments but for `action`, its grid and its LDS bytes
static int mlp_args(ftl_handle* h, const ftl_outputs* out, const ftl_mlp* net, ftlmlp::Args& a, unsigned& grid, size_t& lds) {
    if (!h || !out || !net || !net->params) return fail(FTL_E_INVALID, "null argument");
    if (int rc = mlp_net_check(net, h->P.n_envs, false, "the handle's last env")) return rc;
    const int32_t L = net->n_layers, wl = net->width[L];
    if (!out->policy_obs || h->P.pol_h <= 0 || h->P.pol_width <= 0) return fail(FTL_E_INVALID, "mlp: the policy reads policy_obs (ftl_outputs.policy_obs, a config with a sensor for it)");
    if ((int64_t)net->width[0] != (int64_t)h->P.pol_h * h->P.pol_width) return fail(FTL_E_INVALID, "mlp: width[0] must be H * W of policy_obs");
    a.obs = out->policy_obs;
    mlp_fill(net, h->P.n_envs, a, grid, lds);
    a.head = wl == 2 ? FTL_ACTION_BOX2 : wl == 1 ? FTL_ACTION_TURN : FTL_ACTION_DISCRETE;
    const ftl_robot_params& f = h->P.cfg.follower;
    a.lo0 = f.min_speed; a.hi0 = f.max_speed; a.lo1 = -f.max_rotation_speed; a.hi1 = f.max_rotation_speed;
    a.action = nullptr;
    return FTL_OK;
}

// The one launch of a decision: the kernel of the net's activation (mlp_args has checked it), with the sampling additions when `sm` is given.
static void mlp_launch(const ftl_mlp* net, const ftlmlp::Args& a, const ftlmlp::Sample* sm, unsigned grid, size_t lds, void* stream) {
    const bool th = net->activation == FTL_MLP_ACT_TANH;
    if (sm) hipLaunchKernelGGL(th ? ftlmlp::ftl_mlp_sample_tanh_kernel : ftlmlp::ftl_mlp_sample_kernel, dim3(grid), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a, *sm);
    else hipLaunchKernelGGL(th ? ftlmlp::ftl_mlp_tanh_kernel : ftlmlp::ftl_mlp_kernel, dim3(grid), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a);
}

// what ftl_mlp_sample and ftl_collect_mlp check of the sampling pointers alike; `name` heads the messages
static int mlp_sample_check(const char* name, int32_t head, const float* noise, const float* sigma, const float* head_rec, const float* obs_rec) {
    if (noise && !sigma && head != FTL_ACTION_DISCRETE)
        return fail(FTL_E_INVALID, std::string(name) + ": a Box head with noise needs sigma (z = y + sigma * noise)");
    if ((((uintptr_t)noise) | ((uintptr_t)sigma) | ((uintptr_t)head_rec) | ((uintptr_t)obs_rec)) & 3)
        return fail(FTL_E_INVALID, std::string(name) + ": noise, sigma, head and obs must be 4-byte aligned");
    return FTL_OK;
}

// The closed-loop rollout of a policy, for ftl_rollout_mlp and ftl_rollout_rnn; `name` heads the messages.  What comes before the checks
// of the entry's own net ...
static int policy_rollout_check(const char* name, const void* h, const void* out, const void* net, const ftl_rollout_outputs* ro, int32_t T,
                                uint32_t flags) {
    if (!h || !out || !net) return fail(FTL_E_INVALID, "null argument");
    if (flags & FTL_STEP_NO_SENSORS)
        return fail(FTL_E_INVALID, std::string(name) + " refuses FTL_STEP_NO_SENSORS: every step scans, because the next decision reads policy_obs");
    return rollout_check(name, ro, T, 0, flags);
}

// ... and what comes after them: `head` is the net's action encoding, ready() whatever its kernel needs on the handle's device before
// the first launch, decide(action) enqueues one decision that writes every env's encoded action to `action` (block t of the caller's
// `actions`, or the handle's scratch)
template <typename Ready, typename Decide>
static int policy_rollout(const char* name, ftl_handle* h, int32_t head, int32_t T, double gamma, const ftl_outputs* out,
                          const ftl_rollout_outputs* ro, void* actions, int64_t step_bytes, void* stream, Ready ready, Decide decide) {
    const int64_t block = (int64_t)h->P.n_envs * (int64_t)mlp_action_bytes(head);
    if (actions && step_bytes < block) return fail(FTL_E_INVALID, std::string(name) + ": step_bytes below one block of encoded actions");
    if (actions && ((((uintptr_t)actions) | (uintptr_t)step_bytes) & (head == FTL_ACTION_DISCRETE ? 3 : 7)))
        return fail(FTL_E_INVALID, std::string(name) + ": actions and step_bytes not aligned to the action element");
    if (int rc = check_ready(h, out)) return rc;
    if (int rc = set_device(h)) return rc;
    if (int rc = ready()) return rc;
    if (!actions && !h->bl_action) {                            // (16 bytes per env: any encoding fits the baseline's scratch)
        hipError_t e = hipMalloc((void**)&h->bl_action, align_up((size_t)h->P.n_envs * 16, 256));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(policy actions): ") + hipGetErrorString(e));
    }
    if (int rc = rollout_scratch(h)) return rc;                 // (a recurrent decision reads h->ro_alive)
    return rollout_loop(h, head, T, gamma, out, ro, 0, true, stream, [&](int32_t t) {
        void* action = actions ? (void*)((char*)actions + (int64_t)t * step_bytes) : (void*)h->bl_action;
        decide(action);
        return action;
    });
}

// the spans of ftl_mlp_backward for a checked net and its rows: those of the first touched set, of a whole set and of the last touched
// set (0 when the first is the only one), the touched sets and the sum; false when the sum leaves the grid
struct MlpBwdPlan { int64_t spans0, spans_mid, spans_last, n_touched, spans; };
static MlpBwdPlan mlp_bwd_plan(const ftl_mlp* net, int64_t n_blocks, int64_t n) {
    const TileMap m = tile_map(net->env_first, net->envs_per_set, n);
    auto spans_of = [&](int64_t tiles) { return (n_blocks * tiles + FTL_MLP_BWD_SPAN - 1) / FTL_MLP_BWD_SPAN; };
    MlpBwdPlan p;
    p.spans0 = spans_of(m.tiles0);
    p.spans_mid = m.rem ? spans_of(m.tiles_per_set) : 1;
    p.spans_last = !m.rem ? 0 : m.last ? spans_of(m.tiles_last) : p.spans_mid;
    p.n_touched = 1 + m.full + (m.last ? 1 : 0);
    p.spans = p.spans0 + m.full * p.spans_mid + (m.last ? p.spans_last : 0);
    return p;
}

// What ftl_mlp_forward and ftl_mlp_backward check alike, in their common order, between the checks of their own: `name` heads the
// messages, `limit` is the entry's text for more than 65,535 blocks, `io` ("y" / "dy") names the rows `r` beside x
struct MlpRows {
    const char *name, *limit, *io;
    const ftl_handle* h; const ftl_mlp* net; int32_t n_blocks, n;
    const float* x; int64_t x_block_bytes; const float* r; int64_t r_block_bytes;
    int no(int code, const std::string& what) const { return fail(code, std::string(name) + ": " + what); }
    int nulls() const {
        if (!h) return no(FTL_E_INVALID, "null argument: h");
        if (!net) return no(FTL_E_INVALID, "null argument: net");
        if (!net->params) return no(FTL_E_INVALID, "null argument: net->params");
        if (!x) return no(FTL_E_INVALID, "null argument: x");
        if (!r) return no(FTL_E_INVALID, std::string("null argument: ") + io);
        return FTL_OK;
    }
    int shape() const {
        if (n_blocks < 1 || n < 1) return no(FTL_E_INVALID, "n_blocks and n must be at least 1");
        if (n_blocks > 65535) return no(FTL_E_UNSUPPORTED, limit);
        return mlp_net_check(net, n, true, "the last row");
    }
    int block_bytes() const {
        const int64_t w0 = net->width[0], wl = net->width[net->n_layers];
        if (x_block_bytes < (int64_t)n * w0 * 4 || (x_block_bytes & 3))
            return no(FTL_E_INVALID, "x_block_bytes must be a multiple of 4 of at least one block, n * width[0] * 4");
        if (r_block_bytes < (int64_t)n * wl * 4 || (r_block_bytes & 3))
            return no(FTL_E_INVALID, std::string(io) + "_block_bytes must be a multiple of 4 of at least one block, n * width[L] * 4");
        return FTL_OK;
    }
    int aligned() const {
        if (((uintptr_t)x) & 3) return no(FTL_E_INVALID, "x must be 4-byte aligned");
        if (((uintptr_t)r) & 3) return no(FTL_E_INVALID, std::string(io) + " must be 4-byte aligned");
        return FTL_OK;
    }
    // the kernel's arguments of a block's rows: no head map, no bounds, no action
    void fill(ftlmlp::Args& a, unsigned& grid, size_t& lds) const {
        mlp_fill(net, n, a, grid, lds);
        a.obs = x; a.head = 0; a.lo0 = a.hi0 = a.lo1 = a.hi1 = 0.0; a.action = nullptr;
    }
};

extern "C" {

size_t ftl_sizeof_mlp(void) { return sizeof(ftl_mlp); }

int64_t ftl_mlp_param_count(const int32_t* widths, int32_t n_layers) { return mlp_param_count(widths, n_layers); }

int ftl_mlp_act(ftl_handle* h, const ftl_outputs* out, const ftl_mlp* net, void* action, void* stream) {
    if (!action) return fail(FTL_E_INVALID, "null argument");
    ftlmlp::Args a; unsigned grid; size_t lds;
    if (int rc = mlp_args(h, out, net, a, grid, lds)) return rc;
    if (((uintptr_t)action) & (a.head == FTL_ACTION_DISCRETE ? 3 : 7)) return fail(FTL_E_INVALID, "ftl_mlp_act: action not aligned to its element");
    if (int rc = check_ready(h, out)) return rc;
    if (int rc = set_device(h)) return rc;
    a.action = action;
    mlp_launch(net, a, nullptr, grid, lds, stream);
    return launched();
}

int ftl_mlp_sample(ftl_handle* h, const ftl_outputs* out, const ftl_mlp* net, const float* noise, const float* sigma, float* head_rec,
                   float* obs_rec, void* action, void* stream) {
    if (!action) return fail(FTL_E_INVALID, "null argument");
    ftlmlp::Args a; unsigned grid; size_t lds;
    if (int rc = mlp_args(h, out, net, a, grid, lds)) return rc;
    if (((uintptr_t)action) & (a.head == FTL_ACTION_DISCRETE ? 3 : 7)) return fail(FTL_E_INVALID, "ftl_mlp_sample: action not aligned to its element");
    if (int rc = mlp_sample_check("ftl_mlp_sample", a.head, noise, sigma, head_rec, obs_rec)) return rc;
    if (int rc = check_ready(h, out)) return rc;
    if (int rc = set_device(h)) return rc;
    a.action = action;
    const ftlmlp::Sample sm{noise, sigma, head_rec, obs_rec};
    mlp_launch(net, a, &sm, grid, lds, stream);
    return launched();
}

int ftl_rollout_mlp(ftl_handle* h, int32_t T, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro, const ftl_mlp* net,
                    void* actions, int64_t step_bytes, uint32_t flags, void* stream) {
    if (int rc = policy_rollout_check("ftl_rollout_mlp", h, out, net, ro, T, flags)) return rc;
    ftlmlp::Args a; unsigned grid; size_t lds;
    if (int rc = mlp_args(h, out, net, a, grid, lds)) return rc;
    return policy_rollout("ftl_rollout_mlp", h, a.head, T, gamma, out, ro, actions, step_bytes, stream, [] { return (int)FTL_OK; },
                          [&](void* action) { a.action = action; mlp_launch(net, a, nullptr, grid, lds, stream); });
}

int ftl_mlp_forward(const ftl_handle* h, const ftl_mlp* net, int32_t n_blocks, int32_t n, const float* x, int64_t x_block_bytes,
                    float* y, int64_t y_block_bytes, void* stream) {
    const MlpRows r{"ftl_mlp_forward", "n_blocks beyond 65,535 (the blocks are the grid's second dimension)", "y",
                    h, net, n_blocks, n, x, x_block_bytes, y, y_block_bytes};
    if (int rc = r.nulls()) return rc;
    if (int rc = r.shape()) return rc;
    if (int rc = r.block_bytes()) return rc;
    ftlmlp::Args a; unsigned grid; size_t lds;
    r.fill(a, grid, lds);
    if ((uint64_t)grid * FTL_MLP_THREADS > 0xFFFFFFFFull)       // (a grid dimension counts threads in 32 bits: 2^24 tiles, over 5e8 rows a block)
        return fail(FTL_E_UNSUPPORTED, "ftl_mlp_forward: n beyond the 2^24 - 1 tiles of one launch; split the rows into blocks");
    if (int rc = r.aligned()) return rc;
    if (int rc = set_device(h)) return rc;
    const ftlmlp::Forward fw{x_block_bytes, y, y_block_bytes};
    hipLaunchKernelGGL(net->activation == FTL_MLP_ACT_TANH ? ftlmlp::ftl_mlp_forward_tanh_kernel : ftlmlp::ftl_mlp_forward_kernel,
                       dim3(grid, (unsigned)n_blocks), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a, fw);
    return launched();
}

int64_t ftl_sizeof_mlp_backward_workspace(const ftl_mlp* net, int32_t n_blocks, int32_t n) {
    if (!net || n_blocks < 1 || n < 1 || net->envs_per_set < 1 || net->env_first < 0) return -1;
    const int64_t count = mlp_param_count(net->width, net->n_layers);
    if (count < 0) return -1;
    return mlp_bwd_plan(net, n_blocks, n).spans * count * 4;
}

int ftl_mlp_backward(const ftl_handle* h, const ftl_mlp* net, int32_t n_blocks, int32_t n, const float* x, int64_t x_block_bytes,
                     const float* dy, int64_t dy_block_bytes, float* grad, void* workspace, int64_t workspace_bytes, void* stream) {
    const MlpRows r{"ftl_mlp_backward", "n_blocks beyond 65,535 (the limit of ftl_mlp_forward)", "dy",
                    h, net, n_blocks, n, x, x_block_bytes, dy, dy_block_bytes};
    if (int rc = r.nulls()) return rc;
    if (!grad) return fail(FTL_E_INVALID, "ftl_mlp_backward: null argument: grad");
    if (!workspace) return fail(FTL_E_INVALID, "ftl_mlp_backward: null argument: workspace");
    if (int rc = r.shape()) return rc;
    if (net->width[0] > FTL_MLP_BWD_MAX_IN) return fail(FTL_E_UNSUPPORTED, "ftl_mlp_backward: input width beyond FTL_MLP_BWD_MAX_IN");
    if (int rc = r.block_bytes()) return rc;
    ftlmlp::Args a; unsigned grid; size_t lds;
    r.fill(a, grid, lds);
    const int64_t wl = net->width[net->n_layers];
    const MlpBwdPlan p = mlp_bwd_plan(net, n_blocks, n);
    if ((uint64_t)grid * FTL_MLP_THREADS > 0xFFFFFFFFull || (uint64_t)p.spans * FTL_MLP_THREADS > 0xFFFFFFFFull)
        return fail(FTL_E_UNSUPPORTED, "ftl_mlp_backward: n beyond the 2^24 - 1 tiles of a block, or beyond 2^24 - 1 spans in all; split the rows");
    const int64_t count = mlp_param_count(net->width, net->n_layers);
    if (workspace_bytes < p.spans * count * 4)
        return fail(FTL_E_INVALID, "ftl_mlp_backward: workspace_bytes below ftl_sizeof_mlp_backward_workspace");
    if (int rc = r.aligned()) return rc;
    if (((uintptr_t)grad) & 3) return fail(FTL_E_INVALID, "ftl_mlp_backward: grad must be 4-byte aligned");
    if (((uintptr_t)workspace) & 3) return fail(FTL_E_INVALID, "ftl_mlp_backward: workspace must be 4-byte aligned");
    if (int rc = set_device(h)) return rc;
    // LDS: a buffer per hidden layer and one for dy, the input chunk and the weight stage (a chunk's rows at the wider of the two strides)
    size_t stage = 0;
    for (int l = 1; l <= net->n_layers; l++) {
        const int w = net->width[l];
        stage = std::max(stage, (size_t)ftlmlp::chunk_rows(w) * std::max(ftlmlp::fwd_stride(w), ftlmlp::bwd_stride(w)));
    }
    lds = ((size_t)(net->n_layers - 1) * FTL_MLP_ENV_TILE * a.act_stride + (size_t)FTL_MLP_ENV_TILE * (ftlmlp::dy_stride((int)wl) + ftlmlp::XS) + stage) * sizeof(float);
    if (lds > 163840) return fail(FTL_E_UNSUPPORTED, "ftl_mlp_backward: the net needs more than the 160 KB of LDS of a workgroup");
    const bool th = net->activation == FTL_MLP_ACT_TANH;
    if (lds > 65536) {                                          // (beyond the default limit of dynamic LDS)
        hipError_t e = hipFuncSetAttribute(th ? (const void*)ftlmlp::ftl_mlp_backward_tanh_kernel : (const void*)ftlmlp::ftl_mlp_backward_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipFuncSetAttribute(ftl_mlp_backward_kernel): ") + hipGetErrorString(e));
    }
    const ftlmlp::Backward bw{x_block_bytes, dy, dy_block_bytes, static_cast<float*>(workspace), count, n_blocks, (int32_t)p.spans0, (int32_t)p.spans_mid};
    hipLaunchKernelGGL(th ? ftlmlp::ftl_mlp_backward_tanh_kernel : ftlmlp::ftl_mlp_backward_kernel,
                       dim3((unsigned)p.spans), dim3(FTL_MLP_THREADS), lds, (hipStream_t)stream, a, bw);
    const ftlmlp::Reduce rd{static_cast<const float*>(workspace), grad, count, net->set_stride, (int32_t)(net->env_first / net->envs_per_set),
                            (int32_t)p.n_touched, (int32_t)p.spans0, (int32_t)p.spans_mid, (int32_t)p.spans_last};
    hipLaunchKernelGGL(ftlmlp::ftl_mlp_backward_reduce_kernel, dim3((unsigned)p.n_touched, (unsigned)((count + FTL_MLP_THREADS - 1) / FTL_MLP_THREADS)),
                       dim3(FTL_MLP_THREADS), 0, (hipStream_t)stream, rd);
    return launched();
}

}  // extern "C"
