// ftl_sampler.hpp -- the scenario sampler (include/ftl.h: ftl_set_scenario_sampler, ftl_sampler_refresh, ftl_sampler_start,
// FTL_STEP_SAMPLE_RESET).  Included by ftl_abi.hip after ftl_restart.hpp (same translation unit: it reads the handle).
//
// ftl_sampler_kernel is the sampler's chooser (ftl_restart.hpp): it runs between a step without auto-reset and the masked reset pass of
// ftl_step_final, where ftl_queue_kernel runs for the queue.  One lane per env, any number of workgroups: the draw of a slot is a pure
// function of its own state words, so the finishing slots need no rank and no order among themselves (the queue's hand-out does, hence its
// single workgroup).  A lane reads its done byte (coalesced); the few lanes whose byte is set (about 0.5 % per step) add their episode to
// the table row of their scenario with agent-scope atomics and search the cdf.  The search runs a fixed number of trips on clamped indices
// with masked results ("loads without guards"): the lanes of a wavefront that search stay in step and a trip's load
// is issued without waiting for a range test.  ftl_sampler_scan_kernel builds the cdf: one workgroup walks the weights in chunks of its
// size with a carry.  Every write of both kernels is an ordinary vector store or a vector atomic.
#include <hip/hip_runtime.h>

#define FTL_SK_THREADS 256        // ftl_sampler_kernel: envs per workgroup
#define FTL_SCAN_THREADS 1024     // ftl_sampler_scan_kernel: weights per chunk (16 wavefronts)

namespace ftlsm {

using ftlrs::MODE_START;

struct Args : ftlrs::Args {
    ftl_scenario_sampler s;
    unsigned long long rng_seed;
};

__device__ __forceinline__ void add64(int64_t* p, long long v) {
    (void)__hip_atomic_fetch_add(reinterpret_cast<long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// device twin of ftl_sample_scenario (include/ftl.h): the number of cdf entries <= r, counted with a power-of-two descent
__device__ __forceinline__ int draw(const Args& a, int stream, int resets) {
    const unsigned long long key = ftl::d_mix64(a.rng_seed + 0x9E3779B97F4A7C15ULL * ((unsigned long long)stream + 1)) ^
                                   ftl::d_mix64(0xD1B54A32D192ED03ULL * ((unsigned long long)resets + 1));
    const unsigned long long x = ftl::d_mix64(key + 0x9E3779B97F4A7C15ULL * ((1ULL << 42) + 1));
    const int count = a.s.count;
    const unsigned long long total = a.s.cdf[count - 1];
    if (total == 0) return (int)__umul64hi(x, (unsigned long long)count);
    const unsigned long long r = __umul64hi(x, total);
    int lo = 0;                                                  // entries known to be <= r
    for (int step = 1 << (31 - __clz(count)); step > 0; step >>= 1) {
        const int j = lo + step;                                 // are the first j entries all <= r?  (the cdf ascends: entry j - 1 decides)
        const unsigned long long v = a.s.cdf[min(j, count) - 1];
        lo = (j <= count && v <= r) ? j : lo;
    }
    return min(lo, count - 1);                                   // (lo < count on a cdf that ftl_sampler_refresh wrote: its last entry is total > r)
}

__global__ __launch_bounds__(FTL_SK_THREADS) void ftl_sampler_kernel(const Args a) {
    const int e = (int)(blockIdx.x * FTL_SK_THREADS + threadIdx.x);
    if (e >= a.n_envs) return;
    const bool start = a.mode == MODE_START;
    const bool fin = start || a.done[e] != 0;
    if (!start) {
        a.restarted[e] = fin ? 1 : 0;
        if (a.ended) a.ended[e] = fin ? 1 : 0;
    }
    if (!fin) return;
    if (!start) {
        const ftlrs::Ended v = ftlrs::end_episode(a, e);
        const int row = v.scen - a.s.base;
        if (row >= 0 && row < a.s.count) {                        // (outside: drawn before the window moved)
            int64_t* t = a.s.table + (size_t)row * FTL_N_SCEN_STATS;
            add64(t + FTL_SS_EPISODES, 1);
            if (v.at_reset) add64(t + FTL_SS_DONE_AT_RESET, 1);
            else {
                add64(t + FTL_SS_FRAMES_SUM, v.frames);
                add64(t + FTL_SS_RETURN_Q16, __double2ll_rn(v.ret * 65536.0));
                if (v.status[0] == FTL_MISSION_SUCCESS) add64(t + FTL_SS_SUCCESS, 1);
                if (v.status[1] == FTL_AGENT_CRASH) add64(t + FTL_SS_CRASH, 1);
                if (v.status[1] == FTL_AGENT_LOW_REWARD) add64(t + FTL_SS_LOW_REWARD, 1);
                if (v.status[1] == FTL_AGENT_TOO_FAR) add64(t + FTL_SS_TOO_FAR, 1);
                if (v.status[0] == FTL_MISSION_FINISHED_BY_TIME) add64(t + FTL_SS_TIMEOUT, 1);
                (void)__hip_atomic_fetch_max(reinterpret_cast<long long*>(t + FTL_SS_LAST_CALL), (long long)a.now, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    const int* ei = ftlrs::env_words(a, e);
    a.scen_idx[e] = a.s.base + draw(a, a.env_id_base + e + ei[FTL_EI_STREAM], ei[FTL_EI_RESETS]);
}

// cdf[i] = weight[0] + .. + weight[i] in uint64.  One workgroup; per chunk of FTL_SCAN_THREADS weights an inclusive scan inside every
// wavefront (shuffles), the sixteen wavefront totals through LDS, and the running carry of the chunks before.
__global__ __launch_bounds__(FTL_SCAN_THREADS) void ftl_sampler_scan_kernel(const uint32_t* __restrict__ weight, uint64_t* __restrict__ cdf, int count) {
    __shared__ unsigned long long s_tot[FTL_SCAN_THREADS / FTL_WAVE];
    const int lane = (int)threadIdx.x % FTL_WAVE, wave = (int)threadIdx.x / FTL_WAVE;
    unsigned long long carry = 0;
    for (int c0 = 0; c0 < count; c0 += FTL_SCAN_THREADS) {
        const int i = c0 + (int)threadIdx.x;
        unsigned long long v = i < count ? (unsigned long long)weight[i] : 0ull;
#pragma unroll
        for (int d = 1; d < FTL_WAVE; d <<= 1) {
            const unsigned long long u = __shfl_up(v, (unsigned)d, FTL_WAVE);
            v += lane >= d ? u : 0ull;
        }
        if (lane == FTL_WAVE - 1) s_tot[wave] = v;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < FTL_SCAN_THREADS / FTL_WAVE; w++) { const unsigned long long t = s_tot[w]; before += w < wave ? t : 0ull; all += t; }
        if (i < count) cdf[i] = carry + before + v;
        carry += all;
        __syncthreads();                                         // s_tot is rewritten by the next chunk
    }
}

}  // namespace ftlsm

// base + count <= n_scenarios: checked against the pool when a sampling call is issued
static int ftl_sampler_check_window(const ftl_handle* h) {
    const ftl_scenario_sampler& s = h->sampler.v;
    if ((int64_t)s.base + s.count > (int64_t)h->P.scen.n_scenarios)
        return fail(FTL_E_INVALID, "ftl_scenario_sampler: base + count lies outside the scenario pool");
    return FTL_OK;
}

// FtlChoose of the sampler: table rows and draws (MODE_START: every slot draws, nothing is recorded)
static int ftl_sampler_choose(ftl_handle* h, const ftl_outputs* out, const ftl_final_outputs* fin, int mode, void* stream, ftlrs::Args& r) {
    int rc = ftl_sampler_check_window(h);        // (ftl_step_final has checked it before its step, ftl_sampler_start has not)
    if (rc) return rc;
    rc = restart_args(h, r, out, fin, mode, h->sampler.calls);
    if (rc) return rc;
    if (!fin) r.ended = nullptr;                 // ended = restarted here, and without final buffers nothing reads the scratch's copy
    hipLaunchKernelGGL(ftlsm::ftl_sampler_kernel, dim3((unsigned)((r.n_envs + FTL_SK_THREADS - 1) / FTL_SK_THREADS)), dim3(FTL_SK_THREADS), 0,
                       (hipStream_t)stream, ftlsm::Args{r, h->sampler.v, h->P.cfg.rng_seed});
    return FTL_OK;
}

extern "C" {

size_t ftl_sizeof_scenario_sampler(void) { return sizeof(ftl_scenario_sampler); }

int ftl_set_scenario_sampler(ftl_handle* h, const ftl_scenario_sampler* s) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!s) { h->sampler.attached = false; return FTL_OK; }
    if (!s->weight || !s->cdf || !s->table) return fail(FTL_E_INVALID, "ftl_scenario_sampler: weight / cdf / table missing");
    if (s->count <= 0) return fail(FTL_E_INVALID, "ftl_scenario_sampler: count must be positive");
    if (s->base < 0) return fail(FTL_E_INVALID, "ftl_scenario_sampler: base must not be negative");
    if ((((uintptr_t)s->cdf) & 7) || (((uintptr_t)s->table) & 7)) return fail(FTL_E_INVALID, "ftl_scenario_sampler: cdf and table must be 8-byte aligned");
    h->sampler = {*s, true, 0};
    return FTL_OK;
}

int ftl_sampler_refresh(ftl_handle* h, void* stream) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!h->sampler.attached) return fail(FTL_E_STATE, "ftl_set_scenario_sampler has not been called");
    if (int rc = set_device(h)) return rc;
    const ftl_scenario_sampler& s = h->sampler.v;
    hipLaunchKernelGGL(ftlsm::ftl_sampler_scan_kernel, dim3(1), dim3(FTL_SCAN_THREADS), 0, (hipStream_t)stream, s.weight, s.cdf, (int)s.count);
    return launched();
}

int ftl_sampler_start(ftl_handle* h, const ftl_outputs* out, void* stream) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!h->sampler.attached) return fail(FTL_E_STATE, "ftl_set_scenario_sampler has not been called");
    ftlrs::Args r;
    return start_chosen(h, out, stream, ftl_sampler_choose, r);
}

}  // extern "C"
