// ftl_sampler.hpp -- the scenario sampler (include/ftl.h: ftl_set_scenario_sampler, ftl_sampler_refresh, ftl_sampler_start,
// FTL_STEP_SAMPLE_RESET).  Included at the end of ftl_abi.hip (same translation unit: it reads the handle).
//
// ftl_sampler_kernel runs between a step without auto-reset and the masked reset pass of ftl_step_final, where ftl_queue_kernel runs for
// the queue.  One lane per env, any number of workgroups: the draw of a slot is a pure function of its own state words, so the finishing
// slots need no rank and no order among themselves (the queue's hand-out does, hence its single workgroup).  A lane reads its done byte
// (coalesced); the few lanes whose byte is set (about 0.5 % per step) add their episode to the table row of their scenario with agent-scope
// atomics and search the cdf.  The search runs a fixed number of trips on clamped indices with masked results ("loads
// without guards"): the lanes of a wavefront that search stay in step and a trip's load is issued without waiting for a range test.
// ftl_sampler_scan_kernel builds the cdf: one workgroup walks the weights in chunks of its size with a carry.  Every write of both
// kernels is an ordinary vector store or a vector atomic.
#include <hip/hip_runtime.h>

#define FTL_SK_THREADS 256        // ftl_sampler_kernel: envs per workgroup
#define FTL_SCAN_THREADS 1024     // ftl_sampler_scan_kernel: weights per chunk (16 wavefronts)

namespace ftlsm {

enum { MODE_STEP = 0, MODE_START = 1 };

struct Args {
    ftl_scenario_sampler s;
    int32_t* env_int; const double* env_dbl; double* ep_stats;   // state fields (record 0 / env 0), as in FtlDevParams
    const int32_t* route_len;       // of the scenario pool: 0 = the world is done at reset
    const uint8_t* done; const uint8_t* status;                  // ftl_outputs of the step
    int32_t* scen_idx;              // [n_envs] out: pool index every finishing slot drew (the reset pass's scen_idx)
    uint8_t* ended; uint8_t* restarted;                          // [n_envs] out, every slot (ended may be null)
    unsigned long long rng_seed;
    int32_t rec_stride, n_envs, env_id_base, mode;
    int32_t now, _pad;              // the handle's sample-call counter
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
    const int* ei = reinterpret_cast<const int*>(reinterpret_cast<const char*>(a.env_int) + (size_t)e * a.rec_stride);
    if (!start) {
        const int scen = ei[FTL_EI_SCEN], row = scen - a.s.base;
        const bool at_reset = a.route_len[scen] == 0;            // the only world g_reset leaves done (ENV:508-510)
        if (row >= 0 && row < a.s.count) {                        // (outside: drawn before the window moved)
            int64_t* t = a.s.table + (size_t)row * FTL_N_SCEN_STATS;
            add64(t + FTL_SS_EPISODES, 1);
            if (at_reset) add64(t + FTL_SS_DONE_AT_RESET, 1);
            else {
                const double* ed = reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.env_dbl) + (size_t)e * a.rec_stride);
                const int i0 = a.status[3 * (size_t)e], i1 = a.status[3 * (size_t)e + 1];
                add64(t + FTL_SS_FRAMES_SUM, ei[FTL_EI_STEP_COUNT]);
                add64(t + FTL_SS_RETURN_Q16, __double2ll_rn(ed[FTL_ED_OVERALL_REWARD] * 65536.0));
                if (i0 == FTL_MISSION_SUCCESS) add64(t + FTL_SS_SUCCESS, 1);
                if (i1 == FTL_AGENT_CRASH) add64(t + FTL_SS_CRASH, 1);
                if (i1 == FTL_AGENT_LOW_REWARD) add64(t + FTL_SS_LOW_REWARD, 1);
                if (i1 == FTL_AGENT_TOO_FAR) add64(t + FTL_SS_TOO_FAR, 1);
                if (i0 == FTL_MISSION_FINISHED_BY_TIME) add64(t + FTL_SS_TIMEOUT, 1);
                (void)__hip_atomic_fetch_max(reinterpret_cast<long long*>(t + FTL_SS_LAST_CALL), (long long)a.now, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (at_reset) a.ep_stats[(size_t)e * FTL_N_METRICS + FTL_M_EPISODES] += 1.0;      // (the step records the others when it raises done)
    }
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

struct FtlSamplerState {
    ftl_scenario_sampler s;
    bool attached;
    int32_t calls;               // ftl_step* calls with FTL_STEP_SAMPLE_RESET on this handle since the attach (the table's FTL_SS_LAST_CALL)
    void* mem;                   // scen_idx | restarted (library-owned, allocated by the first launch)
};

// base + count <= n_scenarios: checked against the pool when a sampling call is issued
static int ftl_sampler_check_window(const ftl_handle* h) {
    const ftl_scenario_sampler& s = h->sampler->s;
    if ((int64_t)s.base + s.count > (int64_t)h->P.scen.n_scenarios)
        return fail(FTL_E_INVALID, "ftl_scenario_sampler: base + count lies outside the scenario pool");
    return FTL_OK;
}

namespace ftlsm {

static int prepare(ftl_handle* h, Args& a, const ftl_outputs* out, int mode) {
    FtlSamplerState& S = *h->sampler;
    { int rc = ftl_sampler_check_window(h); if (rc) return rc; }
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    const size_t n = (size_t)h->P.n_envs, o_rest = align_up(n * 4, 256);
    if (!S.mem) {
        e = hipMalloc(&S.mem, o_rest + align_up(n, 256));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(sampler): ") + hipGetErrorString(e));
    }
    memset(&a, 0, sizeof a);
    a.s = S.s;
    a.env_int = h->P.env_int; a.env_dbl = h->P.env_dbl; a.ep_stats = h->P.ep_stats; a.route_len = h->P.scen.route_len;
    a.done = out->done; a.status = out->status;
    a.scen_idx = (int32_t*)S.mem; a.ended = nullptr; a.restarted = (uint8_t*)S.mem + o_rest;
    a.rng_seed = h->P.cfg.rng_seed;
    a.rec_stride = h->P.rec_stride; a.n_envs = h->P.n_envs; a.env_id_base = h->P.cfg.env_id_base; a.mode = mode; a.now = S.calls;
    return FTL_OK;
}

static void launch_kernel(const Args& a, void* stream) {
    hipLaunchKernelGGL(ftl_sampler_kernel, dim3((unsigned)((a.n_envs + FTL_SK_THREADS - 1) / FTL_SK_THREADS)), dim3(FTL_SK_THREADS), 0,
                       (hipStream_t)stream, a);
}

}  // namespace ftlsm

extern "C" {

size_t ftl_sizeof_scenario_sampler(void) { return sizeof(ftl_scenario_sampler); }

int ftl_set_scenario_sampler(ftl_handle* h, const ftl_scenario_sampler* s) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!s) { if (h->sampler) h->sampler->attached = false; return FTL_OK; }
    if (!s->weight || !s->cdf || !s->table) return fail(FTL_E_INVALID, "ftl_scenario_sampler: weight / cdf / table missing");
    if (s->count <= 0) return fail(FTL_E_INVALID, "ftl_scenario_sampler: count must be positive");
    if (s->base < 0) return fail(FTL_E_INVALID, "ftl_scenario_sampler: base must not be negative");
    if ((((uintptr_t)s->cdf) & 7) || (((uintptr_t)s->table) & 7)) return fail(FTL_E_INVALID, "ftl_scenario_sampler: cdf and table must be 8-byte aligned");
    if (!h->sampler) {
        h->sampler = new (std::nothrow) FtlSamplerState();
        if (!h->sampler) return fail(FTL_E_DEVICE, "out of host memory");
        h->sampler->mem = nullptr;
    }
    h->sampler->s = *s; h->sampler->attached = true; h->sampler->calls = 0;
    return FTL_OK;
}

int ftl_sampler_refresh(ftl_handle* h, void* stream) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!h->sampler || !h->sampler->attached) return fail(FTL_E_STATE, "ftl_set_scenario_sampler has not been called");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    const ftl_scenario_sampler& s = h->sampler->s;
    hipLaunchKernelGGL(ftlsm::ftl_sampler_scan_kernel, dim3(1), dim3(FTL_SCAN_THREADS), 0, (hipStream_t)stream, s.weight, s.cdf, (int)s.count);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
    return FTL_OK;
}

int ftl_sampler_start(ftl_handle* h, const ftl_outputs* out, void* stream) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!h->sampler || !h->sampler->attached) return fail(FTL_E_STATE, "ftl_set_scenario_sampler has not been called");
    if (!h->bound) return fail(FTL_E_STATE, "ftl_bind_state has not been called");
    if (!h->have_scen) return fail(FTL_E_STATE, "ftl_load_scenarios has not been called");
    int rc = check_out(h, out);
    if (rc) return rc;
    ftlsm::Args a;
    rc = ftlsm::prepare(h, a, out, ftlsm::MODE_START);
    if (rc) return rc;
    ftlsm::launch_kernel(a, stream);
    return ftl_reset(h, a.scen_idx, nullptr, out, stream);
}

}  // extern "C"

static void ftl_sampler_destroy(ftl_handle* h) {
    if (!h->sampler) return;
    if (h->sampler->mem) { (void)hipSetDevice(h->device); (void)hipFree(h->sampler->mem); }
    delete h->sampler; h->sampler = nullptr;
}

static int ftl_sampler_attached(const ftl_handle* h) { return h->sampler && h->sampler->attached; }

// FTL_STEP_SAMPLE_RESET of ftl_step_final, after the step (a plain one: no flag) was launched on `stream`: table rows and draws, the terminal
// rows, the reset pass over the slots that finished
static int ftl_sampler_finish_step(ftl_handle* h, const FtlCall& step, const ftl_outputs* out, const ftl_final_outputs* fin, void* stream) {
    h->sampler->calls += 1;
    ftlsm::Args a;
    int rc = ftlsm::prepare(h, a, out, ftlsm::MODE_STEP);
    if (rc) return rc;
    if (fin) { a.ended = fin->ended; a.restarted = fin->restarted; }
    ftlsm::launch_kernel(a, stream);
    if (fin) {
        const int n = h->P.n_envs, epb = FTL_FC_THREADS;
        const int pol_len = (fin->policy_obs && out->policy_obs) ? h->P.pol_h * h->P.pol_width : 0;
        hipLaunchKernelGGL(ftl::ftl_final_copy_kernel, dim3((unsigned)((n + epb - 1) / epb)), dim3(FTL_FC_THREADS), 0, (hipStream_t)stream,
                           *out, *fin, n, h->P.lasers_len, pol_len);
    }
    FtlCall rcall = step;
    rcall.mode = 1; rcall.flags = FTL_CALL_FINISH | FTL_CALL_QUEUE; rcall.scen_idx = a.scen_idx; rcall.mask = a.restarted; rcall.action = nullptr;
    rcall.ended = nullptr; rcall.restarted = nullptr;
    return launch(h, rcall, stream);
}
