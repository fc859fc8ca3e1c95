// ftl_ppo.hpp -- the PPO loss head on the device (include/ftl.h: ftl_ppo_head): from the new heads, the record, the advantages and the
// critic's values to dhead, dvalue, d log_std and a table of statistics, per weight set, with the row arithmetic of ftl_ppo_math.hpp and
// reductions in a fixed order.  Four launches on the caller's stream:
//   ftl_ppo_moments_kernel   count, sum of adv and of adv * adv of every segment (float64 lanes, then a fixed tree)
//   ftl_ppo_scalars_kernel   a workgroup a set: the segment partials in ascending order, then mean, deviation and 1 / count
//   ftl_ppo_rows_kernel      every row: ratio, surrogate, gradients (coalesced stores), and the segment partials of the loss terms
//   ftl_ppo_stats_kernel     a workgroup a set: those partials in ascending order, the stats columns and d log_std
// A segment (up to FTL_PPO_SEG consecutive rows of one set's slice of one block) is one wavefront's work: lane k owns the rows at offsets
// k mod 64, so loads and stores are coalesced, and a wavefront walks over as many segments as the grid leaves it (a population of 64-env
// members has 32,768 segments of one row a lane).  Which wavefront takes which segment changes no result: a partial depends on its
// segment alone.  No atomics, no host synchronisation; the workspace needs no clearing, every word that is read was written by the call.
#ifndef FTL_PPO_HPP
#define FTL_PPO_HPP

#include "ftl_ppo_math.hpp"

namespace ftlppo {

constexpr int MOM = 3, ROWQ = 6;        // float64 words of a segment's partial: count, S1, S2 | -min, value loss, -d, clipped, k_0, k_1
constexpr int SUM_CHUNK = 128;          // segment partials a workgroup stages in LDS at a time when it sums a set

struct Args {
    const float *head_new, *head_old, *noise, *sigma_old, *sigma_new, *shift, *adv, *ret, *value;
    const uint8_t* kind;
    float *dhead, *dvalue, *dlog_std;
    double* stats;
    double *part_m, *part_r;            // [n_sets][n_blocks * sps][MOM], [n_sets][n_blocks * sps][ROWQ]
    float* scal;                        // [n_sets][4]: mean32, inv32, invc
    int64_t head_new_bb, head_old_bb, noise_bb, adv_bb, ret_bb, value_bb, kind_bb, dhead_bb, dvalue_bb;
    int64_t nseg;                       // n_blocks * n_sets * sps
    int32_t n_blocks, n_sets, rows, sps;    // rows of a set in a block, segments of such a slice
    float clip_lo, clip_hi, vf_coef;
    int32_t normalize;
};

// segment g in memory order (block, set, segment): its block, set, first row of the block, length, and its slot among the set's partials
struct Seg { int64_t block, row0, slot; int32_t set, len; };
__device__ inline Seg segment(const Args& a, int64_t g) {
    Seg s;
    const int64_t sg = g % a.sps, t = g / a.sps;
    s.set = (int32_t)(t % a.n_sets);
    s.block = t / a.n_sets;
    s.row0 = (int64_t)s.set * a.rows + sg * FTL_PPO_SEG;
    s.len = (int32_t)(a.rows - sg * FTL_PPO_SEG < FTL_PPO_SEG ? a.rows - sg * FTL_PPO_SEG : FTL_PPO_SEG);
    s.slot = ((int64_t)s.set * a.n_blocks + s.block) * a.sps + sg;
    return s;
}

// x[k] += x[k + stride] for stride 32 .. 1: lane 0 ends with the contract's tree
__device__ inline double tree(double x) {
    for (int stride = 32; stride >= 1; stride >>= 1) x += __shfl_down(x, stride);
    return x;
}
__device__ inline int tree(int x) {
    for (int stride = 32; stride >= 1; stride >>= 1) x += __shfl_down(x, stride);
    return x;
}

__global__ __launch_bounds__(256) void ftl_ppo_moments_kernel(const Args a) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < a.nseg; g += nwaves) {
        const Seg s = segment(a, g);
        const uint8_t* __restrict__ kind = a.kind + s.block * a.kind_bb + s.row0;
        const float* __restrict__ adv = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.adv) + s.block * a.adv_bb) + s.row0;
        double s1 = 0.0, s2 = 0.0;
        int cnt = 0;
#pragma unroll 4
        for (int o = lane; o < s.len; o += 64) {
            const double x = (double)adv[o];
            const bool valid = kind[o] != FTL_TR_VOID;
            const double xx = x * x;
            s1 = valid ? s1 + x : s1;
            s2 = valid ? s2 + xx : s2;
            cnt += valid ? 1 : 0;
        }
        s1 = tree(s1); s2 = tree(s2); cnt = tree(cnt);
        if (lane == 0) {
            double* p = a.part_m + s.slot * MOM;
            p[0] = (double)cnt; p[1] = s1; p[2] = s2;
        }
    }
}

// thread q < nq: the float64 sum from +0.0 of word q of the set's `count` partials, ascending; staged through LDS so that the loads are
// coalesced and only the additions are sequential
__device__ inline double sum_partials(const double* __restrict__ p, int64_t count, int nq, double* lds) {
    double s = 0.0;
    for (int64_t c0 = 0; c0 < count; c0 += SUM_CHUNK) {
        const int cn = (int)(count - c0 < SUM_CHUNK ? count - c0 : SUM_CHUNK);
        for (int i = (int)threadIdx.x; i < cn * nq; i += (int)blockDim.x) lds[i] = p[c0 * nq + i];
        __syncthreads();
        if ((int)threadIdx.x < nq) {
#pragma unroll 8
            for (int j = 0; j < cn; j++) s += lds[j * nq + threadIdx.x];
        }
        __syncthreads();
    }
    return s;
}

__global__ __launch_bounds__(256) void ftl_ppo_scalars_kernel(const Args a) {
    __shared__ double lds[SUM_CHUNK * ROWQ];
    __shared__ double tot[8];
    const int64_t set = blockIdx.x, count = (int64_t)a.n_blocks * a.sps;
    const double s = sum_partials(a.part_m + set * count * MOM, count, MOM, lds);
    if (threadIdx.x < MOM) tot[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const ftlppomath::Moments m = ftlppomath::moments(tot[0], tot[1], tot[2]);
        float* sc = a.scal + set * 4;
        sc[0] = m.mean32; sc[1] = m.inv32; sc[2] = m.invc; sc[3] = 0.0f;
        double* st = a.stats + set * FTL_PPO_STATS;
        st[0] = tot[0]; st[1] = m.mean; st[2] = m.std;
    }
}

template <int A>
__global__ __launch_bounds__(256) void ftl_ppo_rows_kernel(const Args a) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    ftlppomath::Set st;
    st.clip_lo = a.clip_lo; st.clip_hi = a.clip_hi; st.vf_coef = a.vf_coef; st.normalize = a.normalize; st.has_value = a.value != nullptr;
    for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < a.nseg; g += nwaves) {
        const Seg s = segment(a, g);
        for (int j = 0; j < A; j++) {
            st.sigma_new[j] = a.sigma_new[s.set * A + j]; st.sigma_old[j] = a.sigma_old[s.set * A + j];
            st.shift[j] = a.shift ? a.shift[s.set * A + j] : 0.0f;
        }
        st.mean32 = a.scal[s.set * 4]; st.inv32 = a.scal[s.set * 4 + 1]; st.invc = a.scal[s.set * 4 + 2];
        const uint8_t* __restrict__ kind = a.kind + s.block * a.kind_bb + s.row0;
        auto at = [&](const float* base, int64_t bb, int64_t w) {
            return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + s.block * bb) + s.row0 * w;
        };
        const float* __restrict__ hn = at(a.head_new, a.head_new_bb, A);
        const float* __restrict__ ho = at(a.head_old, a.head_old_bb, A);
        const float* __restrict__ nz = at(a.noise, a.noise_bb, A);
        const float* __restrict__ adv = at(a.adv, a.adv_bb, 1);
        const float* __restrict__ ret = at(a.ret, a.ret_bb, 1);
        const float* __restrict__ val = st.has_value ? at(a.value, a.value_bb, 1) : nullptr;
        float* __restrict__ dh = reinterpret_cast<float*>(reinterpret_cast<char*>(a.dhead) + s.block * a.dhead_bb) + s.row0 * A;
        float* __restrict__ dv = st.has_value ? reinterpret_cast<float*>(reinterpret_cast<char*>(a.dvalue) + s.block * a.dvalue_bb) + s.row0 : nullptr;
        double pl = 0.0, vl = 0.0, nd = 0.0, k0 = 0.0, k1 = 0.0;
        int clipped = 0;
#pragma unroll 2
        for (int o = lane; o < s.len; o += 64) {
            float x[2], y[2], z[2];
            if (A == 2) {
                const float2 xv = reinterpret_cast<const float2*>(hn)[o], yv = reinterpret_cast<const float2*>(ho)[o], zv = reinterpret_cast<const float2*>(nz)[o];
                x[0] = xv.x; x[1] = xv.y; y[0] = yv.x; y[1] = yv.y; z[0] = zv.x; z[1] = zv.y;
            } else {
                x[0] = hn[o]; y[0] = ho[o]; z[0] = nz[o]; x[1] = y[1] = z[1] = 0.0f;
            }
            const bool valid = kind[o] != FTL_TR_VOID;
            ftlppomath::Row r;
            ftlppomath::row<A>(st, x, y, z, adv[o], ret[o], st.has_value ? val[o] : 0.0f, r);
            if (A == 2) reinterpret_cast<float2*>(dh)[o] = valid ? make_float2(r.dhead[0], r.dhead[1]) : make_float2(0.0f, 0.0f);
            else dh[o] = valid ? r.dhead[0] : 0.0f;
            if (st.has_value) dv[o] = valid ? r.dvalue : 0.0f;
            pl = valid ? pl + (double)r.pl : pl;
            vl = valid ? vl + (double)r.vl : vl;
            nd = valid ? nd + (double)r.nd : nd;
            k0 = valid ? k0 + (double)r.k[0] : k0;
            if (A == 2) k1 = valid ? k1 + (double)r.k[1] : k1;
            clipped += valid ? r.clipped : 0;
        }
        pl = tree(pl); vl = tree(vl); nd = tree(nd); k0 = tree(k0); clipped = tree(clipped);
        if (A == 2) k1 = tree(k1);
        if (lane == 0) {
            double* p = a.part_r + s.slot * ROWQ;
            p[0] = pl; p[1] = vl; p[2] = nd; p[3] = (double)clipped; p[4] = k0; p[5] = k1;
        }
    }
}

__global__ __launch_bounds__(256) void ftl_ppo_stats_kernel(const Args a, const int width) {
    __shared__ double lds[SUM_CHUNK * ROWQ];
    __shared__ double tot[8];
    const int64_t set = blockIdx.x, count = (int64_t)a.n_blocks * a.sps;
    const double s = sum_partials(a.part_r + set * count * ROWQ, count, ROWQ, lds);
    if (threadIdx.x < ROWQ) tot[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* st = a.stats + set * FTL_PPO_STATS;
        const double cnt = st[0];
        const bool any = cnt > 0.0;
        const double c3 = any ? tot[0] / cnt : 0.0;
        const double c4 = any && a.value ? tot[1] / cnt : 0.0;
        const double vc = (double)a.vf_coef * c4;
        st[3] = c3; st[4] = c4; st[5] = any ? tot[2] / cnt : 0.0; st[6] = any ? tot[3] / cnt : 0.0; st[7] = c3 + vc;
        for (int j = 0; j < width; j++) a.dlog_std[set * width + j] = (float)tot[4 + j];
    }
}

}  // namespace ftlppo

// the segments of a call, or -1 where ftl_ppo_head refuses the counts (or beyond 2^31 - 1 segments)
static int64_t ppo_segments(int64_t n_blocks, int64_t n, int64_t n_sets, int64_t* sps_out) {
    if (n_blocks < 1 || n < 1 || n_sets < 1 || n % n_sets) return -1;
    const int64_t rows = n / n_sets, sps = (rows + FTL_PPO_SEG - 1) / FTL_PPO_SEG;
    const int64_t per_block = n_sets * sps;                    // (at most n: below 2^31)
    if (per_block > INT32_MAX / n_blocks) return -1;
    if (sps_out) *sps_out = sps;
    return per_block * n_blocks;
}

extern "C" {

size_t ftl_sizeof_ppo_head_args(void) { return sizeof(ftl_ppo_head_args); }

int64_t ftl_sizeof_ppo_head_workspace(int32_t n_blocks, int32_t n, int32_t n_sets) {
    const int64_t nseg = ppo_segments(n_blocks, n, n_sets, nullptr);
    if (nseg < 0) return -1;
    return nseg * (ftlppo::MOM + ftlppo::ROWQ) * 8 + (int64_t)n_sets * 16;
}

int ftl_ppo_head(const ftl_handle* h, const ftl_ppo_head_args* a, void* stream) {
    if (!h) return fail(FTL_E_INVALID, "ftl_ppo_head: null argument: h");
    if (!a) return fail(FTL_E_INVALID, "ftl_ppo_head: null argument: a");
    const struct { const void* p; const char* name; } need[] = {
        {a->head_new, "head_new"}, {a->head_old, "head_old"}, {a->noise, "noise"}, {a->sigma_old, "sigma_old"}, {a->sigma_new, "sigma_new"},
        {a->adv, "adv"}, {a->ret, "ret"}, {a->kind, "kind"}, {a->dhead, "dhead"}, {a->dlog_std, "dlog_std"}, {a->stats, "stats"},
        {a->workspace, "workspace"}};
    for (const auto& q : need)
        if (!q.p) return fail(FTL_E_INVALID, std::string("ftl_ppo_head: null argument: ") + q.name);
    if (a->dvalue && !a->value_new) return fail(FTL_E_INVALID, "ftl_ppo_head: dvalue without value_new");
    if (a->value_new && !a->dvalue) return fail(FTL_E_INVALID, "ftl_ppo_head: value_new without dvalue");
    if (a->n_blocks < 1 || a->n < 1) return fail(FTL_E_INVALID, "ftl_ppo_head: n_blocks and n must be at least 1");
    if (a->n_sets < 1 || a->n % a->n_sets) return fail(FTL_E_INVALID, "ftl_ppo_head: n_sets must be at least 1 and divide n");
    if (a->width != 1 && a->width != 2)
        return fail(FTL_E_UNSUPPORTED, "ftl_ppo_head: width must be 2 (Box(2)) or 1 (Box(1) turn); the Discrete(5) head needs a pinned logarithm "
                                       "that is not there yet");
    const int64_t n = a->n, A = a->width;
    const struct { int64_t bb, row; bool on; const char* name; } strides[] = {
        {a->head_new_block_bytes, A * 4, true, "head_new_block_bytes"}, {a->head_old_block_bytes, A * 4, true, "head_old_block_bytes"},
        {a->noise_block_bytes, A * 4, true, "noise_block_bytes"}, {a->adv_block_bytes, 4, true, "adv_block_bytes"},
        {a->ret_block_bytes, 4, true, "ret_block_bytes"}, {a->value_new_block_bytes, 4, a->value_new != nullptr, "value_new_block_bytes"},
        {a->kind_block_bytes, 1, true, "kind_block_bytes"}, {a->dhead_block_bytes, A * 4, true, "dhead_block_bytes"},
        {a->dvalue_block_bytes, 4, a->dvalue != nullptr, "dvalue_block_bytes"}};
    for (const auto& q : strides) {
        if (!q.on) continue;
        if (q.bb < n * q.row) return fail(FTL_E_INVALID, std::string("ftl_ppo_head: ") + q.name + " below one block of n rows");
        if (q.bb % q.row) return fail(FTL_E_INVALID, std::string("ftl_ppo_head: ") + q.name + " not aligned to the array's element");
    }
    const struct { const void* p; int64_t el; const char* name; } ptrs[] = {
        {a->head_new, A * 4, "head_new"}, {a->head_old, A * 4, "head_old"}, {a->noise, A * 4, "noise"}, {a->sigma_old, 4, "sigma_old"},
        {a->sigma_new, 4, "sigma_new"}, {a->log_sigma_shift, 4, "log_sigma_shift"}, {a->adv, 4, "adv"}, {a->ret, 4, "ret"},
        {a->value_new, 4, "value_new"}, {a->dhead, A * 4, "dhead"}, {a->dvalue, 4, "dvalue"}, {a->dlog_std, 4, "dlog_std"}, {a->stats, 8, "stats"}};
    for (const auto& q : ptrs)
        if (((uintptr_t)q.p) % (uintptr_t)q.el)
            return fail(FTL_E_INVALID, std::string("ftl_ppo_head: ") + q.name + " not aligned to its element (" + std::to_string(q.el) + " bytes)");
    if (!(a->clip_lo <= a->clip_hi)) return fail(FTL_E_INVALID, "ftl_ppo_head: clip_lo and clip_hi must be numbers with clip_lo <= clip_hi");
    if (a->normalize != 0 && a->normalize != 1) return fail(FTL_E_INVALID, "ftl_ppo_head: normalize must be 0 or 1");
    int64_t sps = 0;
    const int64_t nseg = ppo_segments(a->n_blocks, a->n, a->n_sets, &sps);
    if (nseg < 0) return fail(FTL_E_UNSUPPORTED, "ftl_ppo_head: more than 2^31 - 1 segments; split the blocks");
    const int64_t ws_need = nseg * (ftlppo::MOM + ftlppo::ROWQ) * 8 + (int64_t)a->n_sets * 16;
    if (a->workspace_bytes < ws_need) return fail(FTL_E_INVALID, "ftl_ppo_head: workspace_bytes below ftl_sizeof_ppo_head_workspace");
    if (((uintptr_t)a->workspace) & 7) return fail(FTL_E_INVALID, "ftl_ppo_head: workspace must be 8-byte aligned");
    if (int rc = set_device(h)) return rc;
    ftlppo::Args k;
    k.head_new = a->head_new; k.head_old = a->head_old; k.noise = a->noise; k.sigma_old = a->sigma_old; k.sigma_new = a->sigma_new;
    k.shift = a->log_sigma_shift; k.adv = a->adv; k.ret = a->ret; k.value = a->value_new; k.kind = a->kind;
    k.dhead = a->dhead; k.dvalue = a->dvalue; k.dlog_std = a->dlog_std; k.stats = a->stats;
    k.part_m = static_cast<double*>(a->workspace);
    k.part_r = k.part_m + nseg * ftlppo::MOM;
    k.scal = reinterpret_cast<float*>(k.part_r + nseg * ftlppo::ROWQ);
    k.head_new_bb = a->head_new_block_bytes; k.head_old_bb = a->head_old_block_bytes; k.noise_bb = a->noise_block_bytes;
    k.adv_bb = a->adv_block_bytes; k.ret_bb = a->ret_block_bytes; k.value_bb = a->value_new_block_bytes; k.kind_bb = a->kind_block_bytes;
    k.dhead_bb = a->dhead_block_bytes; k.dvalue_bb = a->dvalue_block_bytes;
    k.nseg = nseg; k.n_blocks = a->n_blocks; k.n_sets = a->n_sets; k.rows = a->n / a->n_sets; k.sps = (int32_t)sps;
    k.clip_lo = a->clip_lo; k.clip_hi = a->clip_hi; k.vf_coef = a->vf_coef; k.normalize = a->normalize;
    // four wavefronts a workgroup, a segment a wavefront at a time; at most 2,048 workgroups (8 wavefronts a SIMD of 256 CUs), the rest by stride
    const unsigned grid = (unsigned)std::min<int64_t>((nseg + 3) / 4, 2048);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ftlppo::ftl_ppo_moments_kernel, dim3(grid), dim3(256), 0, st, k);
    hipLaunchKernelGGL(ftlppo::ftl_ppo_scalars_kernel, dim3((unsigned)a->n_sets), dim3(256), 0, st, k);
    if (a->width == 2) hipLaunchKernelGGL(ftlppo::ftl_ppo_rows_kernel<2>, dim3(grid), dim3(256), 0, st, k);
    else hipLaunchKernelGGL(ftlppo::ftl_ppo_rows_kernel<1>, dim3(grid), dim3(256), 0, st, k);
    hipLaunchKernelGGL(ftlppo::ftl_ppo_stats_kernel, dim3((unsigned)a->n_sets), dim3(256), 0, st, k, (int)a->width);
    return launched();
}

}  // extern "C"
#endif
