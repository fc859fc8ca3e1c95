// ftl_rollout.hpp -- T steps of an open-loop action sequence with one call (ftl_rollout, include/ftl.h), and the one rollout loop of the
// library: rollout_loop, which ftl_rollout calls with a pointer into the caller's sequence as the action of step t, ftl_baseline.hpp
// (ftl_rollout_baseline, ftl_rollout_guided) with the follower's act kernel and ftl_mlp.hpp (ftl_rollout_mlp) with the policy's forward
// kernel and a scan in every step, and ftl_collect.hpp (ftl_collect_mlp) with the sampling kernel, no fold, next-step reset and a record
// kernel after every step.  Included by ftl_abi.hip after ftl_step_final (same translation unit: it reads the handle and calls
// launch()).
//
// The rollout is T launches of a step without auto-reset -- the first T - 1 of them without the sensor kernels -- and, after each frame
// launch, ftl_rollout_fold_kernel: one thread per env adds the step's discounted reward to the env's return while its episode runs.  The
// fold lives outside the frame kernel on purpose (that kernel has no register to spare).  Which envs are still running is a byte per env
// in a scratch the handle owns (allocated by the first rollout), set from the state's done word by a first pass before step 0.
#include <hip/hip_runtime.h>

namespace ftlro {

struct Args {
    const int32_t* env_int; int32_t rec_stride, n_envs;      // state: the done word of record 0, as in FtlDevParams
    const double* reward; const uint8_t* done; const uint8_t* status;   // ftl_outputs of the step
    ftl_rollout_outputs ro;
    uint8_t* alive;          // [n_envs] 1: the env's done word was 0 on entry to the next step
    double disc;             // gamma^t of the step being folded
    int32_t first;           // 1: the pass before step 0 (zero ro, alive from the state); nothing is folded
};

__global__ __launch_bounds__(256) void ftl_rollout_fold_kernel(const Args a) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= a.n_envs) return;
    if (a.first) {
        const int32_t* ei = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(a.env_int) + (size_t)e * a.rec_stride);
        a.alive[e] = ei[FTL_EI_DONE] ? 0 : 1;
        a.ro.ret[e] = 0.0; a.ro.steps[e] = 0;
        for (int k = 0; k < 3; k++) a.ro.status[3 * (size_t)e + k] = 0;
        return;
    }
    if (!a.alive[e]) return;
    const double term = a.disc * a.reward[e];                  // two roundings (the unit is built with -ffp-contract=off)
    a.ro.ret[e] = a.ro.ret[e] + term;
    a.ro.steps[e] += 1;
    if (a.done[e]) {                                            // the step that raises done counts; later ones do not
        for (int k = 0; k < 3; k++) a.ro.status[3 * (size_t)e + k] = a.status[3 * (size_t)e + k];
        a.alive[e] = 0;
    }
}

}  // namespace ftlro

// What the three rollout entries check alike, in their common order; `name` heads the messages.  (ftl_rollout has no tail: it passes 0.)
static int rollout_check(const char* name, const ftl_rollout_outputs* ro, int32_t T, int32_t tail, uint32_t flags) {
    if (!ro) return fail(FTL_E_INVALID, "null argument");
    if (!ro->ret || !ro->steps || !ro->status) return fail(FTL_E_INVALID, "ftl_rollout_outputs: ret / steps / status missing");
    if (T <= 0) return fail(FTL_E_INVALID, std::string(name) + ": T must be positive");
    if (tail < 0 || tail > INT32_MAX - T) return fail(FTL_E_INVALID, std::string(name) + ": tail must be at least 0 (and T + tail an int32)");
    if (flags & ~(uint32_t)FTL_STEP_NO_SENSORS)
        return fail(FTL_E_INVALID, std::string(name) + " takes no flag but FTL_STEP_NO_SENSORS (there is no auto-reset inside a rollout)");
    return FTL_OK;
}

// The rollout loop of every entry, after its checks and set_device: T steps on `stream`, each followed by the fold.  scan_every false: the
// first T - 1 steps are blind and the last one takes `flags`; true (a policy that reads the sensors: ftl_rollout_mlp): every step takes
// `flags`.  action(t) enqueues whatever decides step t and returns what the step reads: [n_envs][2] doubles, or the encoded actions.
// ro == nullptr: no fold (ftl_collect_mlp keeps a record per step instead of a sum, and is the one caller whose `flags` may carry
// FTL_STEP_NEXT_RESET).  post(t) enqueues whatever follows step t and its fold on `stream`, and returns an error code.
static int rollout_scratch(ftl_handle* h) {
    if (!h->ro_alive) {
        hipError_t e = hipMalloc((void**)&h->ro_alive, align_up((size_t)h->P.n_envs, 256));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(rollout scratch): ") + hipGetErrorString(e));
    }
    return FTL_OK;
}

template <typename Action, typename Post>
static int rollout_loop(ftl_handle* h, int32_t encoding, int32_t T, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro,
                        uint32_t flags, bool scan_every, void* stream, Action action, Post post) {
    if (int rc = rollout_scratch(h)) return rc;
    ftlro::Args a;
    a.env_int = h->P.env_int; a.rec_stride = h->P.rec_stride; a.n_envs = h->P.n_envs;
    a.reward = out->reward; a.done = out->done; a.status = out->status;
    a.ro = ro ? *ro : ftl_rollout_outputs{}; a.alive = h->ro_alive; a.disc = 1.0; a.first = 1;
    const dim3 grid((unsigned)((h->P.n_envs + 255) / 256));
    if (ro) hipLaunchKernelGGL(ftlro::ftl_rollout_fold_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    a.first = 0;
    FtlCall call = make_call(h, 0, out);
    call.action_kind = encoding;
    h->last_lasers = h->P.lasers_len > 0 ? out->lasers : nullptr;
    for (int32_t t = 0; t < T; t++) {
        call.action = (const double*)action(t);
        call.flags = (t < T - 1 && !scan_every) ? (uint32_t)FTL_STEP_NO_SENSORS : flags;
        // (a two-stream handle forks after what action(t) enqueued, and the caller's stream has joined the side stream before the fold)
        if (int rc = launch(h, call, stream)) return rc;
        if (ro) hipLaunchKernelGGL(ftlro::ftl_rollout_fold_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
        a.disc = a.disc * gamma;                                // disc_{t+1} = disc_t * gamma, one rounding each
        if (int rc = post(t)) return rc;
    }
    return launched();
}

// (the rollouts that fold and have nothing to add after a step)
template <typename Action>
static int rollout_loop(ftl_handle* h, int32_t encoding, int32_t T, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro,
                        uint32_t flags, bool scan_every, void* stream, Action action) {
    return rollout_loop(h, encoding, T, gamma, out, ro, flags, scan_every, stream, action, [](int32_t) { return (int)FTL_OK; });
}

extern "C" {

size_t ftl_sizeof_rollout_outputs(void) { return sizeof(ftl_rollout_outputs); }

int ftl_rollout(ftl_handle* h, const void* actions, int64_t step_bytes, int32_t encoding, int32_t T, double gamma,
                const ftl_outputs* out, const ftl_rollout_outputs* ro, uint32_t flags, void* stream) {
    if (!h || !actions || !out) return fail(FTL_E_INVALID, "null argument");
    if (int rc = rollout_check("ftl_rollout", ro, T, 0, flags)) return rc;
    if (encoding < FTL_ACTION_BOX2 || encoding > FTL_ACTION_TURN) return fail(FTL_E_INVALID, "unknown action encoding");
    if (int rc = check_ready(h, out)) return rc;
    if (int rc = set_device(h)) return rc;
    return rollout_loop(h, encoding, T, gamma, out, ro, flags, false, stream, [&](int32_t t) { return (const char*)actions + (int64_t)t * step_bytes; });
}

}  // extern "C"
