// ftl_rollout.hpp -- T steps of an open-loop action sequence with one call (ftl_rollout, include/ftl.h).  Included by ftl_abi.hip after
// ftl_step_final (same translation unit: it reads the handle and calls launch()).
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

extern "C" {

size_t ftl_sizeof_rollout_outputs(void) { return sizeof(ftl_rollout_outputs); }

int ftl_rollout(ftl_handle* h, const void* actions, int64_t step_bytes, int32_t encoding, int32_t T, double gamma,
                const ftl_outputs* out, const ftl_rollout_outputs* ro, uint32_t flags, void* stream) {
    if (!h || !actions || !out || !ro) return fail(FTL_E_INVALID, "null argument");
    if (!ro->ret || !ro->steps || !ro->status) return fail(FTL_E_INVALID, "ftl_rollout_outputs: ret / steps / status missing");
    if (T <= 0) return fail(FTL_E_INVALID, "ftl_rollout: T must be positive");
    if (flags & ~(uint32_t)FTL_STEP_NO_SENSORS) return fail(FTL_E_INVALID, "ftl_rollout takes no flag but FTL_STEP_NO_SENSORS (there is no auto-reset inside a rollout)");
    if (encoding < FTL_ACTION_BOX2 || encoding > FTL_ACTION_TURN) return fail(FTL_E_INVALID, "unknown action encoding");
    int rc = check_ready(h, out);
    if (rc) return rc;
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    if (!h->ro_alive) {
        e = hipMalloc((void**)&h->ro_alive, align_up((size_t)h->P.n_envs, 256));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(rollout scratch): ") + hipGetErrorString(e));
    }
    ftlro::Args a;
    a.env_int = h->P.env_int; a.rec_stride = h->P.rec_stride; a.n_envs = h->P.n_envs;
    a.reward = out->reward; a.done = out->done; a.status = out->status;
    a.ro = *ro; a.alive = h->ro_alive; a.disc = 1.0; a.first = 1;
    const dim3 grid((unsigned)((h->P.n_envs + 255) / 256));
    hipLaunchKernelGGL(ftlro::ftl_rollout_fold_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    a.first = 0;
    FtlCall call = make_call(h, 0, out);
    call.action_kind = encoding;
    h->last_lasers = h->P.lasers_len > 0 ? out->lasers : nullptr;
    for (int32_t t = 0; t < T; t++) {
        call.action = (const double*)((const char*)actions + (int64_t)t * step_bytes);
        call.flags = (t < T - 1) ? (uint32_t)FTL_STEP_NO_SENSORS : flags;
        rc = launch(h, call, stream);                           // (on a two-stream handle the caller's stream has joined the side stream)
        if (rc) return rc;
        hipLaunchKernelGGL(ftlro::ftl_rollout_fold_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
        a.disc = a.disc * gamma;                                // disc_{t+1} = disc_t * gamma, one rounding each
    }
    e = hipGetLastError();
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
    return FTL_OK;
}

}  // extern "C"
