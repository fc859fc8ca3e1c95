// ftl_guided.hpp -- guided search (include/ftl.h: ftl_search_guided, ftl_guided_fanout): the action search of ftl_search.hpp over RESIDUALS
// added to the baseline follower's own closed-loop action, scored over a horizon that ends in a closed-loop baseline tail.  Included at the
// end of ftl_abi.hip after ftl_search.hpp (same translation unit).  The shared checks and the rounds are those of ftl_search.hpp
// (check_buffers, check_handles, rounds); what is here is the fan-out, the guided search's own checks, what a round rolls
// (ftl_guided_fanout, ftl_rollout_guided) and the decision (ftl_baseline_act_guided).
//
// ftl_guided_fanout_kernel  what ftl_unpack_envs_from does not carry to a clone: the follower row of its source env and the two output rows
//                           the follower's next decision reads (obs_num, target).  One lane per piece of a clone's rows, pieces in the order
//                           [C = 1 + cap chunks of 16 bytes of the follower row][the target row, 16 bytes][FTL_OBS_NUM floats], clone after
//                           clone: consecutive lanes load and store consecutive 16-byte chunks of one follower row (dwordx4 both ways), a
//                           wavefront covers 1 KB of it.  The K clones of an env read the same source row, which the L2 serves after the
//                           first.  Written bytes: n K (16 + 16 cap + 16 + 40), about 1.1 KB per clone at cap = 64.  Plain vector stores.
#include <hip/hip_runtime.h>

namespace ftlgd {

struct FanoutArgs {
    const unsigned char* src_bl; unsigned char* dst_bl;        // [n] and [n * K] follower rows of 16 * chunks bytes, 16-byte aligned
    const float* src_obs; float* dst_obs;                      // obs_num rows of FTL_OBS_NUM floats
    const double* src_target; double* dst_target;              // target rows of two doubles
    unsigned long long total;                                  // n * K * (chunks + 1 + FTL_OBS_NUM) pieces
    int32_t K, chunks;
};

__global__ __launch_bounds__(256) void ftl_guided_fanout_kernel(const FanoutArgs a) {
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.total) return;
    const unsigned per = (unsigned)a.chunks + 1u + (unsigned)FTL_OBS_NUM;
    const size_t i = (size_t)(j / per);                        // clone
    const unsigned c = (unsigned)(j - (unsigned long long)i * per);
    const size_t e = i / (unsigned)a.K;                        // its source env
    if (c < (unsigned)a.chunks) {
        const uint4* s = reinterpret_cast<const uint4*>(a.src_bl) + e * (size_t)a.chunks + c;
        uint4* d = reinterpret_cast<uint4*>(a.dst_bl) + i * (size_t)a.chunks + c;
        *d = *s;
    } else if (c == (unsigned)a.chunks) {
        a.dst_target[2 * i] = a.src_target[2 * e];
        a.dst_target[2 * i + 1] = a.src_target[2 * e + 1];
    } else {
        const unsigned f = c - (unsigned)a.chunks - 1u;
        a.dst_obs[i * FTL_OBS_NUM + f] = a.src_obs[e * FTL_OBS_NUM + f];
    }
}

}  // namespace ftlgd

extern "C" {

size_t ftl_sizeof_guided_buffers(void) { return sizeof(ftl_guided_buffers); }

int ftl_guided_fanout(const ftl_handle* real, const ftl_handle* search, int32_t K, const ftl_outputs* real_out, const ftl_outputs* search_out,
                      const void* real_bl, size_t real_bl_bytes, void* search_bl, size_t search_bl_bytes, int32_t cap, void* stream) {
    if (!real || !search || !real_out || !search_out || !real_bl || !search_bl) return fail(FTL_E_INVALID, "null argument");
    if (!real_out->obs_num || !real_out->target || !search_out->obs_num || !search_out->target) return fail(FTL_E_INVALID, "output arrays missing");
    if (cap < 2) return fail(FTL_E_INVALID, "baseline follower: cap must be at least 2");
    const int32_t n = real->P.n_envs;
    if (int rc = ftlse::check_size(n, K, 1)) return rc;
    if ((long long)search->P.n_envs != (long long)n * K) return fail(FTL_E_INVALID, "ftl_guided_fanout: the search handle must hold n * K envs");
    if (real->device != search->device) return fail(FTL_E_INVALID, "ftl_guided_fanout: the two handles live on different devices");
    const size_t row = baseline_row_bytes(cap);
    if (real_bl_bytes < (size_t)n * row || search_bl_bytes < (size_t)n * K * row)
        return fail(FTL_E_INVALID, "baseline follower: state buffer too small (ftl_baseline_bytes)");
    if ((((uintptr_t)real_bl) | ((uintptr_t)search_bl)) & 15) return fail(FTL_E_INVALID, "ftl_guided_fanout: the follower buffers must be 16-byte aligned");
    if (real_bl == search_bl || real_out->obs_num == search_out->obs_num || real_out->target == search_out->target)
        return fail(FTL_E_INVALID, "ftl_guided_fanout: source and destination must be distinct buffers");
    ftlgd::FanoutArgs a;
    a.src_bl = (const unsigned char*)real_bl; a.dst_bl = (unsigned char*)search_bl;
    a.src_obs = real_out->obs_num; a.dst_obs = search_out->obs_num; a.src_target = real_out->target; a.dst_target = search_out->target;
    a.K = K; a.chunks = 1 + cap;
    a.total = (unsigned long long)n * K * ((unsigned long long)a.chunks + 1 + FTL_OBS_NUM);
    if ((a.total + 255) / 256 > 0x7fffffffull) return fail(FTL_E_INVALID, "ftl_guided_fanout: n * K * cap is too large for one launch");
    if (int rc = set_device(search)) return rc;
    hipLaunchKernelGGL(ftlgd::ftl_guided_fanout_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launched();
}

int ftl_search_guided(ftl_handle* real, ftl_handle* search, const ftl_search_params* p, uint64_t call, int32_t warm, int32_t tail,
                      const ftl_guided_buffers* b, void* stream) {
    if (!real || !search || !b) return fail(FTL_E_INVALID, "null argument");
    if (int rc = ftlse::check_params(p)) return rc;
    if (tail < 0 || tail > INT32_MAX - p->T) return fail(FTL_E_INVALID, "ftl_search_guided: tail must be at least 0 (and T + tail an int32)");
    if (!b->real_out || !b->real_bl || !b->search_bl) return fail(FTL_E_INVALID, "ftl_guided_buffers: a buffer is missing");
    const ftl_search_buffers sb = {b->rows, b->row_ids, b->env_ids, b->nominal, b->cand, b->action, b->best_k, b->best_ret, b->out, b->ro};
    if (int rc = ftlse::check_buffers("ftl_guided_buffers", "ftl_search_guided", real, search, p, sb)) return rc;
    const int32_t n = real->P.n_envs, K = p->K, cap = b->cap;
    if (cap < 2) return fail(FTL_E_INVALID, "baseline follower: cap must be at least 2");
    if (b->real_bl_bytes < (size_t)n * baseline_row_bytes(cap) || b->search_bl_bytes < (size_t)n * K * baseline_row_bytes(cap))
        return fail(FTL_E_INVALID, "baseline follower: state buffer too small (ftl_baseline_bytes)");
    if ((((uintptr_t)b->real_bl) | ((uintptr_t)b->search_bl)) & 15) return fail(FTL_E_INVALID, "ftl_search_guided: the follower buffers must be 16-byte aligned");
    if (int rc = ftlse::check_handles(real, search, {b->out, b->real_out})) return rc;
    // the default plan is the zero residual: the baseline itself
    int rc = ftlse::rounds(real, search, p, call, warm, 0.0, true, sb, stream, [&] {
        if (int rc = ftl_guided_fanout(real, search, K, b->real_out, b->out, b->real_bl, b->real_bl_bytes, b->search_bl, b->search_bl_bytes, cap, stream))
            return rc;
        return ftl_rollout_guided(search, p->T, tail, p->gamma, b->out, b->ro, b->search_bl, b->search_bl_bytes, cap, b->cand, (int64_t)n * K * 16, nullptr, 0,
                                  FTL_STEP_NO_SENSORS, stream);
    });
    if (rc) return rc;
    // last, so that every round fanned out the follower rows as they were before this decision: books the real follower's step exactly once
    return ftl_baseline_act_guided(real, b->real_out, b->real_bl, b->real_bl_bytes, cap, b->nominal, b->action, stream);
}

}  // extern "C"
