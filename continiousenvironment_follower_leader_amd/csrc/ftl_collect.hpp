// ftl_collect.hpp -- what a policy-gradient method needs after the forward pass (include/ftl.h: ftl_collect_mlp, ftl_gae): T stochastic
// closed-loop steps through episode boundaries with one call, recorded step by step, and the advantages of such a record.  Included by
// ftl_abi.hip after ftl_mlp.hpp (same translation unit: it launches ftl_mlp_sample_kernel and hands it to rollout_loop, which owns the
// steps; there is no second loop here).  collect_check and collect_loop are the one collect of both net families: ftl_collect_rnn
// (ftl_rnn.hpp) calls them with its state blocks and its own kernel.
//
// ftl_collect_record_kernel: one thread per env after every step.  It copies the step's reward into block t and classifies the transition
// from the byte "the episode was running on entry to the step" (the handle's rollout scratch, the one ftl_rollout_fold_kernel keeps), the
// step's done and its mission status; then the byte becomes !done for the next step.  A first pass before step 0 sets the byte from the
// state's done word, as the fold's first pass does.
//
// ftl_gae_kernel: one thread per env walks t from T - 1 down to 0 with the carry in a register; consecutive threads read consecutive
// envs of every block.
#include <hip/hip_runtime.h>

namespace ftlcol {

struct Args {
    const int32_t* env_int; int32_t rec_stride, n_envs;      // state: the done word of record 0, as in FtlDevParams
    const double* reward; const uint8_t* done; const uint8_t* status;   // ftl_outputs of the step
    uint8_t* alive;          // [n_envs] 1: the env's done word was 0 on entry to the step just played
    double* rec_reward; uint8_t* rec_kind;                    // block t of the record
    int32_t first;           // 1: the pass before step 0 (alive from the state); nothing is recorded
};

__global__ __launch_bounds__(256) void ftl_collect_record_kernel(const Args a) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= a.n_envs) return;
    if (a.first) {
        const int32_t* ei = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(a.env_int) + (size_t)e * a.rec_stride);
        a.alive[e] = ei[FTL_EI_DONE] ? 0 : 1;
        return;
    }
    const uint8_t done = a.done[e];
    a.rec_reward[e] = a.reward[e];
    a.rec_kind[e] = !a.alive[e] ? FTL_TR_VOID : !done ? FTL_TR_STEP
                  : a.status[3 * (size_t)e] == FTL_MISSION_FINISHED_BY_TIME ? FTL_TR_TRUNCATED : FTL_TR_TERMINATED;
    a.alive[e] = done ? 0 : 1;
}

struct Gae {
    const double* reward; const uint8_t* kind; const float* values; float* adv; float* ret;
    int64_t reward_step_bytes, kind_step_bytes;
    double gamma, gl;
    int32_t T, n;
};

__global__ __launch_bounds__(256) void ftl_gae_kernel(const Gae a) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= a.n) return;
    double c = 0.0;
    double v1 = (double)a.values[(size_t)a.T * a.n + e];
    for (int t = a.T - 1; t >= 0; t--) {
        const size_t i = (size_t)t * a.n + e;
        const double v0 = (double)a.values[i];
        const double r = reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.reward) + (int64_t)t * a.reward_step_bytes)[e];
        const uint8_t k = a.kind[(int64_t)t * a.kind_step_bytes + e];
        float adv = 0.0f, ret = 0.0f;
        if (k == FTL_TR_VOID) c = 0.0;
        else {
            if (k == FTL_TR_TERMINATED) c = r - v0;
            else {
                const double x = a.gamma * v1;
                const double y = r + x;
                const double d = y - v0;
                if (k == FTL_TR_TRUNCATED) c = d;
                else { const double z = a.gl * c; c = d + z; }
            }
            adv = (float)c; ret = (float)(c + v0);
        }
        a.adv[i] = adv; a.ret[i] = ret;
        v1 = v0;
    }
}

}  // namespace ftlcol

// One collect for ftl_collect_mlp and ftl_collect_rnn; `name` heads the messages.  What comes before the checks of the entry's own net ...
static int collect_check(const char* name, const void* h, const void* out, const void* net, const void* b, uint32_t flags, int32_t T) {
    if (!h || !out || !net || !b) return fail(FTL_E_INVALID, "null argument");
    const std::string who(name);                                // (collect is called once per T steps)
    if (flags & FTL_STEP_NO_SENSORS)
        return fail(FTL_E_INVALID, who + " refuses FTL_STEP_NO_SENSORS: every step scans, because the next decision reads policy_obs");
    if (flags & FTL_STEP_AUTO_RESET)
        return fail(FTL_E_INVALID, who + " refuses FTL_STEP_AUTO_RESET: a same-step reset puts the next episode's first observation where "
                                   "the terminal one belongs, so obs[t+1] would not be the successor of transition t (FTL_STEP_NEXT_RESET keeps it)");
    if (flags & FTL_STEP_QUEUE_RESET)
        return fail(FTL_E_INVALID, who + " refuses FTL_STEP_QUEUE_RESET: the queue restarts a finished env inside the step that ended its "
                                   "episode, so obs[t+1] would not be the successor of transition t (FTL_STEP_NEXT_RESET keeps it)");
    if (flags & FTL_STEP_SAMPLE_RESET)
        return fail(FTL_E_INVALID, who + " refuses FTL_STEP_SAMPLE_RESET: the sampler restarts a finished env inside the step that ended its "
                                   "episode, so obs[t+1] would not be the successor of transition t (FTL_STEP_NEXT_RESET keeps it)");
    if (flags & ~(uint32_t)FTL_STEP_NEXT_RESET) return fail(FTL_E_INVALID, who + " takes no flag but FTL_STEP_NEXT_RESET");
    if (T <= 0) return fail(FTL_E_INVALID, who + ": T must be positive");
    return FTL_OK;
}

// ... and what comes after them, on the checked kernel arguments `m` of the net's feed-forward part (its head and width[0] are read) and
// the head width `wl`.  extra(is_short, misaligned) refuses what the entry records beside `b` and reports whether one of its *_step_bytes
// is below a block or not aligned; ready() is whatever the kernel needs on the handle's device before the first launch; decide(t, sm,
// action) enqueues decision t with the sampling additions `sm`, which writes every env's encoded action to `action`
template <typename Extra, typename Ready, typename Decide>
static int collect_loop(const char* name, ftl_handle* h, int32_t T, const ftl_outputs* out, const ftlmlp::Args& m, int64_t wl,
                        const ftl_collect_buffers* b, uint32_t flags, void* stream, Extra extra, Ready ready, Decide decide) {
    if (!b->obs || !b->head || !b->action || !b->reward || !b->kind)
        return fail(FTL_E_INVALID, "ftl_collect_buffers: obs / head / action / reward / kind missing");
    bool is_short = false, misaligned = false;
    if (int rc = extra(is_short, misaligned)) return rc;
    const int64_t n = h->P.n_envs, w0 = m.width[0], arow = (int64_t)mlp_action_bytes(m.head);
    if (b->obs_step_bytes < n * w0 * 4 || b->head_step_bytes < n * wl * 4 || b->action_step_bytes < n * arow ||
        b->reward_step_bytes < n * 8 || b->kind_step_bytes < n || (b->noise && b->noise_step_bytes < n * wl * 4) || is_short)
        return fail(FTL_E_INVALID, "ftl_collect_buffers: a *_step_bytes below one block of its array");
    if (((((uintptr_t)b->obs) | (uintptr_t)b->obs_step_bytes | ((uintptr_t)b->head) | (uintptr_t)b->head_step_bytes) & 3) ||
        ((((uintptr_t)b->action) | (uintptr_t)b->action_step_bytes) & (uintptr_t)(arow == 4 ? 3 : 7)) ||
        ((((uintptr_t)b->reward) | (uintptr_t)b->reward_step_bytes) & 7) || (b->noise && (b->noise_step_bytes & 3)) || misaligned)
        return fail(FTL_E_INVALID, "ftl_collect_buffers: a base pointer or a *_step_bytes not aligned to the element of its array");
    if (int rc = mlp_sample_check(name, m.head, b->noise, b->sigma, b->head, b->obs)) return rc;
    if (int rc = check_ready(h, out)) return rc;
    if (int rc = set_device(h)) return rc;
    if (int rc = ready()) return rc;
    if (int rc = rollout_scratch(h)) return rc;
    ftlcol::Args r;
    r.env_int = h->P.env_int; r.rec_stride = h->P.rec_stride; r.n_envs = h->P.n_envs;
    r.reward = out->reward; r.done = out->done; r.status = out->status;
    r.alive = h->ro_alive; r.rec_reward = nullptr; r.rec_kind = nullptr; r.first = 1;
    const dim3 rgrid((unsigned)((h->P.n_envs + 255) / 256));
    hipLaunchKernelGGL(ftlcol::ftl_collect_record_kernel, rgrid, dim3(256), 0, (hipStream_t)stream, r);
    r.first = 0;
    ftlmlp::Sample sm{nullptr, b->sigma, nullptr, nullptr};
    const int rc = rollout_loop(h, m.head, T, 1.0, out, nullptr, flags, true, stream,
        [&](int32_t t) {
            sm.noise = b->noise ? (const float*)((const char*)b->noise + (int64_t)t * b->noise_step_bytes) : nullptr;
            sm.head_rec = (float*)((char*)b->head + (int64_t)t * b->head_step_bytes);
            sm.obs_rec = (float*)((char*)b->obs + (int64_t)t * b->obs_step_bytes);
            void* action = (char*)b->action + (int64_t)t * b->action_step_bytes;
            decide(t, sm, action);
            return action;
        },
        [&](int32_t t) {
            r.rec_reward = (double*)((char*)b->reward + (int64_t)t * b->reward_step_bytes);
            r.rec_kind = b->kind + (int64_t)t * b->kind_step_bytes;
            hipLaunchKernelGGL(ftlcol::ftl_collect_record_kernel, rgrid, dim3(256), 0, (hipStream_t)stream, r);
            return (int)FTL_OK;
        });
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync((char*)b->obs + (int64_t)T * b->obs_step_bytes, out->policy_obs, (size_t)n * w0 * 4,
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMemcpyAsync(obs[T]): ") + hipGetErrorString(e));
    return FTL_OK;
}

extern "C" {

size_t ftl_sizeof_collect_buffers(void) { return sizeof(ftl_collect_buffers); }

int ftl_collect_mlp(ftl_handle* h, int32_t T, const ftl_outputs* out, const ftl_mlp* net, const ftl_collect_buffers* b, uint32_t flags, void* stream) {
    if (int rc = collect_check("ftl_collect_mlp", h, out, net, b, flags, T)) return rc;
    ftlmlp::Args a; unsigned grid; size_t lds;
    if (int rc = mlp_args(h, out, net, a, grid, lds)) return rc;
    return collect_loop("ftl_collect_mlp", h, T, out, a, net->width[net->n_layers], b, flags, stream, [](bool&, bool&) { return (int)FTL_OK; },
                        [] { return (int)FTL_OK; },
                        [&](int32_t, const ftlmlp::Sample& sm, void* action) { a.action = action; mlp_launch(net, a, &sm, grid, lds, stream); });
}

int ftl_gae(const ftl_handle* h, int32_t T, int32_t n, const double* reward, int64_t reward_step_bytes, const uint8_t* kind, int64_t kind_step_bytes,
            const float* values, double gamma, double lambda, float* adv, float* ret, void* stream) {
    if (!h || !reward || !kind || !values || !adv || !ret) return fail(FTL_E_INVALID, "null argument");
    if (T <= 0 || n <= 0) return fail(FTL_E_INVALID, "ftl_gae: T and n must be positive");
    if (reward_step_bytes < (int64_t)n * 8 || kind_step_bytes < (int64_t)n) return fail(FTL_E_INVALID, "ftl_gae: a *_step_bytes below one block of n elements");
    if ((((uintptr_t)reward) | (uintptr_t)reward_step_bytes) & 7) return fail(FTL_E_INVALID, "ftl_gae: reward and reward_step_bytes must be 8-byte aligned");
    if ((((uintptr_t)values) | ((uintptr_t)adv) | ((uintptr_t)ret)) & 3) return fail(FTL_E_INVALID, "ftl_gae: values, adv and ret must be 4-byte aligned");
    if (int rc = set_device(h)) return rc;
    ftlcol::Gae g;
    g.reward = reward; g.kind = kind; g.values = values; g.adv = adv; g.ret = ret;
    g.reward_step_bytes = reward_step_bytes; g.kind_step_bytes = kind_step_bytes;
    g.gamma = gamma; g.gl = gamma * lambda; g.T = T; g.n = n;
    hipLaunchKernelGGL(ftlcol::ftl_gae_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
    return launched();
}

}  // extern "C"
