// ftl_search.hpp -- action search on the device (include/ftl.h: ftl_search, ftl_search_begin / _sample / _select): K candidate action
// sequences per env, rolled out blind on clones in a second handle, the best one kept, refined with a shrinking radius.  Included by
// ftl_abi.hip after ftl_baseline.hpp and before ftl_guided.hpp, which searches over residuals (same translation unit: it reads the handles
// and calls ftl_pack_envs, ftl_unpack_envs_from and ftl_rollout).  The checks both searches share (check_buffers, check_handles) and the
// one loop over their rounds (rounds, with what a round rolls as a callable) are here; each entry keeps its own checks and its decision.
// Everything heavy is those three calls; the kernels here move a few doubles per candidate:
//
// ftl_search_begin_kernel   one thread per env: the nominal sequence of this call -- the default (max speed, straight on) for a new episode,
//                           else the last call's plan shifted by one step.  Reads one word of the env's packed row.
// ftl_search_sample_kernel  one thread per (step, clone): candidate 0 copies the nominal, the others add a uniform offset drawn from the
//                           counter stream keyed by the env's absolute stream id (a word of the packed row), clipped to the Box.  Lanes
//                           write consecutive 16-byte actions; the K lanes of an env read the same nominal action and row word.
// ftl_search_select_kernel  one wavefront per env (four per workgroup): lanes stride over the K returns keeping (largest ret, lowest k), a
//                           xor butterfly over the 64 lanes leaves the winner in every lane, lane 0 writes best_k / best_ret and the lanes
//                           stride over the T steps copying the winner's column into the nominal.  No LDS.
#include <hip/hip_runtime.h>

namespace ftlse {

struct BeginArgs {
    const unsigned char* rows; unsigned long long row_bytes;   // [n] packed rows
    int32_t w_step;          // row word index (4-byte units) of env_int[FTL_EI_STEP_COUNT]
    int32_t n, T, fresh;     // fresh: call == 0 or no warm start -- every env takes the default
    double speed;            // follower.max_speed
    double* nominal;         // [T][n][2]
};

__global__ __launch_bounds__(256) void ftl_search_begin_kernel(const BeginArgs a) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= a.n) return;
    const int32_t step = reinterpret_cast<const int32_t*>(a.rows + (size_t)e * a.row_bytes)[a.w_step];
    double* nom = a.nominal + 2 * (size_t)e;
    const size_t st = 2 * (size_t)a.n;                         // doubles from step t to step t + 1
    if (a.fresh || step == 0) {
        for (int t = 0; t < a.T; t++) { nom[t * st] = a.speed; nom[t * st + 1] = 0.0; }
        return;
    }
    for (int t = 0; t + 1 < a.T; t++) { nom[t * st] = nom[(t + 1) * st]; nom[t * st + 1] = nom[(t + 1) * st + 1]; }
}

struct SampleArgs {
    const unsigned char* rows; unsigned long long row_bytes;
    int32_t w_stream;        // row word index of env_int[FTL_EI_STREAM]: the env's absolute stream id
    int32_t n, K, T, hold, it;
    unsigned long long seed, call;
    double s;                // the round's radius as a share of the Box width
    double lo0, hi0, lo1, hi1;
    const double* nominal;   // [T][n][2]
    double* cand;            // [T][n * K][2]
};

__global__ __launch_bounds__(256) void ftl_search_sample_kernel(const SampleArgs a) {
    const size_t nk = (size_t)a.n * a.K;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // (t, clone)
    if (i >= nk * a.T) return;
    const int t = (int)(i / nk);
    const size_t c = i - (size_t)t * nk;
    const int e = (int)(c / a.K), k = (int)(c - (size_t)e * a.K);
    const double2 nom = *reinterpret_cast<const double2*>(a.nominal + 2 * ((size_t)t * a.n + e));
    double2 x = nom;
    if (k > 0) {
        const int32_t sid = reinterpret_cast<const int32_t*>(a.rows + (size_t)e * a.row_bytes)[a.w_stream];
        const unsigned long long key = (1ULL << 43) | (unsigned long long)(t / a.hold) | ((unsigned long long)a.it << 17) | ((unsigned long long)k << 24);
        const double u0 = ftl::d_uniform01(a.seed, (unsigned long long)sid, a.call, key);
        const double u1 = ftl::d_uniform01(a.seed, (unsigned long long)sid, a.call, key | (1ULL << 16));
        x.x = nom.x + (a.s * (u0 - 0.5)) * (a.hi0 - a.lo0);
        x.y = nom.y + (a.s * (u1 - 0.5)) * (a.hi1 - a.lo1);
        x.x = fmin(fmax(x.x, a.lo0), a.hi0);
        x.y = fmin(fmax(x.y, a.lo1), a.hi1);
    }
    *reinterpret_cast<double2*>(a.cand + 2 * i) = x;
}

struct SelectArgs {
    const double* ret;       // [n * K]
    const double* cand;      // [T][n * K][2]
    double* nominal;         // [T][n][2]
    int32_t* best_k; double* best_ret;   // [n]
    int32_t n, K, T;
};

__global__ __launch_bounds__(256) void ftl_search_select_kernel(const SelectArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));           // wave-uniform
    if (e >= a.n) return;
    const double* ret = a.ret + (size_t)e * a.K;
    double br = 0.0; int bk = -1;                                          // bk < 0: this lane holds no candidate (K < 64)
    for (int k = lane; k < a.K; k += 64) {                                 // ascending k: a strict > keeps the lowest among equals
        const double r = ret[k];
        if (bk < 0 || r > br) { br = r; bk = k; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {                              // butterfly: every lane ends with the winner
        const double orr = __shfl_xor(br, off, 64);
        const int ok = __shfl_xor(bk, off, 64);
        if (ok >= 0 && (bk < 0 || orr > br || (orr == br && ok < bk))) { br = orr; bk = ok; }
    }
    if (lane == 0) { a.best_k[e] = bk; a.best_ret[e] = br; }
    const size_t nk = (size_t)a.n * a.K, c = (size_t)e * a.K + bk;
    for (int t = lane; t < a.T; t += 64)
        *reinterpret_cast<double2*>(a.nominal + 2 * ((size_t)t * a.n + e)) = *reinterpret_cast<const double2*>(a.cand + 2 * ((size_t)t * nk + c));
}

static int check_params(const ftl_search_params* p) {
    if (!p) return fail(FTL_E_INVALID, "null argument");
    if (p->K < 1 || p->T < 1 || p->hold < 1 || p->iters < 1) return fail(FTL_E_INVALID, "ftl_search_params: K, T, hold and iters must be at least 1");
    if (p->K >= (1 << 19) || p->iters >= 128 || p->T / p->hold >= 65536)
        return fail(FTL_E_INVALID, "ftl_search_params: beyond the limits of the draw key (K < 2^19, iters < 128, T / hold < 65536)");
    if (!(p->spread > 0.0 && p->spread <= 1.0)) return fail(FTL_E_INVALID, "ftl_search_params: spread must lie in (0, 1]");
    if (!(p->decay > 0.0 && p->decay <= 1.0)) return fail(FTL_E_INVALID, "ftl_search_params: decay must lie in (0, 1]");
    if (!(p->gamma - p->gamma == 0.0)) return fail(FTL_E_INVALID, "ftl_search_params: gamma must be finite");
    if (p->flags & ~(uint32_t)FTL_SEARCH_OWN_STREAM) return fail(FTL_E_INVALID, "unknown ftl_search_params flag bits");
    return FTL_OK;
}

// a [n] x [K] x [T] problem whose element-wise launch fits one grid
static int check_size(int32_t n, int32_t K, int32_t T) {
    if (n < 1 || K < 1 || T < 1) return fail(FTL_E_INVALID, "action search: n, K and T must be at least 1");
    if ((unsigned long long)n * (unsigned long long)K > 0x7fffffffull || (unsigned long long)n * K * T > (0x7fffffffull << 8))
        return fail(FTL_E_INVALID, "action search: n * K * T is too large for one launch");
    return FTL_OK;
}

static int32_t row_word(const ftl_handle* h, int which) { return (int32_t)(h->fields[F_env_int].offset / 4 + which); }

// ftl_search_begin with the default plan's speed given (ftl_search_guided starts from the zero residual)
static int begin(const ftl_handle* h, const void* rows, int32_t n, int32_t T, uint64_t call, int32_t warm, double speed, double* nominal, void* stream) {
    if (!h || !rows || !nominal) return fail(FTL_E_INVALID, "null argument");
    if (int rc = check_size(n, 1, T)) return rc;
    if (int rc = set_device(h)) return rc;
    BeginArgs a;
    a.rows = (const unsigned char*)rows; a.row_bytes = ftls::make_args(h).row_bytes; a.w_step = row_word(h, FTL_EI_STEP_COUNT);
    a.n = n; a.T = T; a.fresh = (call == 0 || !warm) ? 1 : 0; a.speed = speed; a.nominal = nominal;
    hipLaunchKernelGGL(ftl_search_begin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launched();
}

// ftl_search_sample on the action Box(2), or (residual: ftl_search_guided) on the box of the same width centred on 0
static int sample(const ftl_handle* h, const void* rows, int32_t n, const ftl_search_params* p, uint64_t call, int32_t it, double s, bool residual,
                  const double* nominal, double* cand, void* stream) {
    if (!h || !rows || !nominal || !cand) return fail(FTL_E_INVALID, "null argument");
    if (int rc = check_params(p)) return rc;
    if (int rc = check_size(n, p->K, p->T)) return rc;
    if (it < 0 || it >= 128) return fail(FTL_E_INVALID, "ftl_search_sample: round outside 0 .. 127");
    if (!(s >= 0.0 && s <= 1.0)) return fail(FTL_E_INVALID, "ftl_search_sample: the radius s must lie in [0, 1]");
    if ((((uintptr_t)nominal) | ((uintptr_t)cand)) & 15) return fail(FTL_E_INVALID, "nominal and cand must be 16-byte aligned");
    if (int rc = set_device(h)) return rc;
    const ftl_robot_params& f = h->P.cfg.follower;
    SampleArgs a;
    a.rows = (const unsigned char*)rows; a.row_bytes = ftls::make_args(h).row_bytes; a.w_stream = row_word(h, FTL_EI_STREAM);
    a.n = n; a.K = p->K; a.T = p->T; a.hold = p->hold; a.it = it; a.seed = p->seed; a.call = call; a.s = s;
    a.lo0 = f.min_speed; a.hi0 = f.max_speed; a.lo1 = -f.max_rotation_speed; a.hi1 = f.max_rotation_speed;
    if (residual) {                                            // hi - lo is the Box's width again, exactly
        const double h0 = (a.hi0 - a.lo0) / 2.0, h1 = (a.hi1 - a.lo1) / 2.0;
        a.lo0 = -h0; a.hi0 = h0; a.lo1 = -h1; a.hi1 = h1;
    }
    a.nominal = nominal; a.cand = cand;
    const unsigned long long total = (unsigned long long)n * p->K * p->T;
    hipLaunchKernelGGL(ftl_search_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launched();
}

// What ftl_search and ftl_search_guided check alike of the ten buffers their structs share (ftl_guided_buffers: copied into `b` by value)
// and of the two handles, after check_params; `bufs` and `entry` head the messages
static int check_buffers(const char* bufs, const char* entry, const ftl_handle* real, const ftl_handle* search, const ftl_search_params* p,
                         const ftl_search_buffers& b) {
    if (!b.rows || !b.row_ids || !b.env_ids || !b.nominal || !b.cand || !b.action || !b.best_k || !b.best_ret || !b.out || !b.ro)
        return fail(FTL_E_INVALID, std::string(bufs) + ": a buffer is missing");
    if ((((uintptr_t)b.rows) | ((uintptr_t)b.nominal) | ((uintptr_t)b.cand)) & 15) return fail(FTL_E_INVALID, "rows, nominal and cand must be 16-byte aligned");
    if (!b.ro->ret || !b.ro->steps || !b.ro->status) return fail(FTL_E_INVALID, "ftl_rollout_outputs: ret / steps / status missing");
    const int32_t n = real->P.n_envs;
    if (int rc = check_size(n, p->K, p->T)) return rc;
    if ((long long)search->P.n_envs != (long long)n * p->K) return fail(FTL_E_INVALID, std::string(entry) + ": the search handle must hold n * K envs");
    if (real->device != search->device) return fail(FTL_E_INVALID, std::string(entry) + ": the two handles live on different devices");
    if (real == search || ftl_env_layout_id(real) != ftl_env_layout_id(search))
        return fail(FTL_E_INVALID, std::string(entry) + ": the two handles must be distinct and share one env layout (ftl_env_layout_id)");
    return FTL_OK;
}

// ... and last of all their checks (the guided search has its own between the two): the output arrays of every struct, then the state
static int check_handles(const ftl_handle* real, const ftl_handle* search, std::initializer_list<const ftl_outputs*> outs) {
    for (const ftl_outputs* o : outs)
        if (!o->obs_num || !o->target || !o->reward || !o->done || !o->status || (search->P.lasers_len > 0 && !o->lasers))
            return fail(FTL_E_INVALID, "output arrays missing");
    if (!real->bound || !search->bound) return fail(FTL_E_STATE, "ftl_bind_state has not been called");
    if (!real->have_scen || !search->have_scen) return fail(FTL_E_STATE, "ftl_load_scenarios has not been called");
    return FTL_OK;
}

// The rounds of both searches on `stream`: the real envs packed, the start plan (default: `speed`, straight on), then per round the draws
// (`residual`: sample), the rows unpacked to the clones, roll() -- whatever leaves the clones' returns in b.ro->ret --, the selection.
// Leaves the plan in b.nominal; the decision is the caller's.
template <typename Roll>
static int rounds(const ftl_handle* real, ftl_handle* search, const ftl_search_params* p, uint64_t call, int32_t warm, double speed, bool residual,
                  const ftl_search_buffers& b, void* stream, Roll roll) {
    const int32_t n = real->P.n_envs, K = p->K, T = p->T;
    if (int rc = ftl_pack_envs(real, b.env_ids, n, b.rows, stream)) return rc;
    if (int rc = begin(real, b.rows, n, T, call, warm, speed, b.nominal, stream)) return rc;
    const uint32_t uflags = (p->flags & FTL_SEARCH_OWN_STREAM) ? (uint32_t)FTL_ENV_OWN_STREAM : 0u;
    double s = p->spread;
    for (int32_t it = 0; it < p->iters; it++) {
        if (int rc = sample(real, b.rows, n, p, call, it, s, residual, b.nominal, b.cand, stream)) return rc;
        if (int rc = ftl_unpack_envs_from(search, b.rows, b.row_ids, b.env_ids, n * K, uflags, stream)) return rc;
        if (int rc = roll()) return rc;
        if (int rc = ftl_search_select(search, b.ro->ret, n, K, T, b.cand, b.nominal, b.best_k, b.best_ret, stream)) return rc;
        s = s * p->decay;
    }
    return FTL_OK;
}

}  // namespace ftlse

extern "C" {

size_t ftl_sizeof_search_params(void) { return sizeof(ftl_search_params); }
size_t ftl_sizeof_search_buffers(void) { return sizeof(ftl_search_buffers); }

int ftl_search_begin(const ftl_handle* h, const void* rows, int32_t n, int32_t T, uint64_t call, int32_t warm, double* nominal, void* stream) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    return ftlse::begin(h, rows, n, T, call, warm, h->P.cfg.follower.max_speed, nominal, stream);
}

int ftl_search_sample(const ftl_handle* h, const void* rows, int32_t n, const ftl_search_params* p, uint64_t call, int32_t it, double s,
                      const double* nominal, double* cand, void* stream) {
    return ftlse::sample(h, rows, n, p, call, it, s, false, nominal, cand, stream);
}

int ftl_search_select(const ftl_handle* h, const double* ret, int32_t n, int32_t K, int32_t T, const double* cand, double* nominal,
                      int32_t* best_k, double* best_ret, void* stream) {
    if (!h || !ret || !cand || !nominal || !best_k || !best_ret) return fail(FTL_E_INVALID, "null argument");
    if (int rc = ftlse::check_size(n, K, T)) return rc;
    if ((((uintptr_t)nominal) | ((uintptr_t)cand)) & 15) return fail(FTL_E_INVALID, "nominal and cand must be 16-byte aligned");
    if (int rc = set_device(h)) return rc;
    ftlse::SelectArgs a;
    a.ret = ret; a.cand = cand; a.nominal = nominal; a.best_k = best_k; a.best_ret = best_ret; a.n = n; a.K = K; a.T = T;
    hipLaunchKernelGGL(ftlse::ftl_search_select_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return launched();
}

int ftl_search(const ftl_handle* real, ftl_handle* search, const ftl_search_params* p, uint64_t call, int32_t warm,
               const ftl_search_buffers* b, void* stream) {
    if (!real || !search || !b) return fail(FTL_E_INVALID, "null argument");
    if (int rc = ftlse::check_params(p)) return rc;
    if (int rc = ftlse::check_buffers("ftl_search_buffers", "ftl_search", real, search, p, *b)) return rc;
    if (int rc = ftlse::check_handles(real, search, {b->out})) return rc;
    const int32_t n = real->P.n_envs;
    int rc = ftlse::rounds(real, search, p, call, warm, real->P.cfg.follower.max_speed, false, *b, stream, [&] {
        return ftl_rollout(search, b->cand, (int64_t)n * p->K * 16, FTL_ACTION_BOX2, p->T, p->gamma, b->out, b->ro, FTL_STEP_NO_SENSORS, stream);
    });
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(b->action, b->nominal, (size_t)n * 16, hipMemcpyDeviceToDevice, (hipStream_t)stream);   // nominal[0]
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    return FTL_OK;
}

}  // extern "C"
