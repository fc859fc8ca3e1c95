// ftl_queue.hpp -- the episode queue (include/ftl.h: ftl_set_episode_queue, ftl_queue_start, FTL_STEP_QUEUE_RESET).  Included by
// ftl_abi.hip after ftl_restart.hpp (same translation unit: it reads the handle).
//
// ftl_queue_kernel is the queue's chooser (ftl_restart.hpp): it runs between a step without auto-reset and the masked reset pass of
// ftl_step_final.  It is ONE workgroup: the hand-out order (ascending slot order within a call) needs a rank over all finishing slots, and
// there are few of them (about 0.5 % of the envs per step).  Wavefront w owns the contiguous slots [w * span, (w + 1) * span), in rows of
// 64; a lane looks at one done byte per row, sixteen rows in flight.  Sweep 1 counts the finishing slots of every wavefront with ballots;
// one pass over the wavefronts' totals in LDS gives every wavefront its offset, and one lane takes `total` entries with a single
// agent-scope fetch-add on the queue's head.  Sweep 2 ranks the finishing slots of a row with the same ballots and writes them, in
// ascending order, to a list; then every lane does the work of one list entry (rank = list index): the record of the entry that ended, the
// next entry, the scenario index / mask byte of the reset pass, the random-stream words of a fresh env.  (Doing that work inside sweep 2
// serialised its dependent loads row by row: 90 us a call at 65,536 envs with 280 finishing slots.)  Every write is an ordinary vector
// store.
#include <hip/hip_runtime.h>

#define FTL_QK_THREADS 1024       // 16 wavefronts
#define FTL_QK_ROWS 16            // done bytes in flight per lane

namespace ftlq {

using ftlrs::MODE_STEP;
using ftlrs::MODE_START;

struct Args : ftlrs::Args {
    ftl_episode_queue q;
    int32_t* list;                  // [n_envs] scratch: the finishing slots of this call in ascending order
    int32_t span;                   // slots per wavefront (a multiple of 64)
};

__device__ __forceinline__ bool finishing(const Args& a, int e) {      // (the ticket is read only where the done byte is set)
    return e < a.n_envs && (a.mode == MODE_START || (a.done[e] != 0 && a.q.ticket[e] >= 0));
}

// slot e ended the episode of its ticket (MODE_STEP) and takes entry `next`
__device__ __forceinline__ void hand_over(const Args& a, int e, int next) {
    int* ei = ftlrs::env_words(a, e);
    if (a.mode == MODE_STEP) {
        const ftlrs::Ended v = ftlrs::end_episode(a, e);
        ftl_episode_record* r = a.q.records + a.q.ticket[e];
        r->scenario = v.scen; r->env = e;
        r->frames = v.frames;
        r->calls = v.at_reset ? 0 : a.now - r->calls;
        r->status[0] = v.status[0]; r->status[1] = v.status[1]; r->status[2] = v.status[2];
        r->errors = v.errors;
        r->flags = v.at_reset ? FTL_EPISODE_DONE_AT_RESET : 0u;
        r->ret = v.ret;
        r->stream = (int64_t)a.env_id_base + e + ei[FTL_EI_STREAM];
        r->state = 2;
    }
    const bool take = next < a.q.n;
    if (take) {
        const int64_t sid = a.q.stream ? a.q.stream[next] : a.q.stream_base + next;
        const int scen = a.q.scenario[next];
        ftl_episode_record* r = a.q.records + next;
        r->state = 1; r->scenario = scen; r->env = e; r->calls = a.now; r->stream = sid;
        a.scen_idx[e] = scen;
        // a fresh env whose global index is the stream id
        ei[FTL_EI_STREAM] = (int)((uint32_t)(uint64_t)sid - (uint32_t)a.env_id_base - (uint32_t)e);
        ei[FTL_EI_RESETS] = 0; ei[FTL_EI_FPS] = 0; ei[FTL_EI_ACC_CONSUMED] = 0;
        if (sid < 0 || sid > 0x7fffffffLL) ei[FTL_EI_ERROR_STICKY] |= (int)FTL_ERR_BAD_STREAM;
    } else {
        a.scen_idx[e] = a.q.scenario[0];                       // (MODE_START places a parked slot on a valid world)
        if (a.mode == MODE_STEP) ei[FTL_EI_EPISODES] += 1;     // the reset pass counts the episodes of the slots it restarts
    }
    a.q.ticket[e] = take ? next : -1;
    a.restarted[e] = take ? 1 : 0;
}

__global__ __launch_bounds__(FTL_QK_THREADS) void ftl_queue_kernel(const Args a) {
    __shared__ int s_tot[FTL_QK_THREADS / FTL_WAVE];
    __shared__ int s_base;
    const int lane = (int)threadIdx.x % FTL_WAVE, wave = (int)threadIdx.x / FTL_WAVE;
    const int lo = wave * a.span, hi = min(lo + a.span, a.n_envs);
    const bool start = a.mode == MODE_START;                   // every slot takes an entry: no flags to look at, rank = slot
    int mine = 0;                                              // sweep 1: finishing slots of this wavefront (wave-uniform)
    if (!start)
        for (int r0 = lo; r0 < hi; r0 += FTL_QK_ROWS * FTL_WAVE) {
            bool f[FTL_QK_ROWS];
#pragma unroll
            for (int j = 0; j < FTL_QK_ROWS; j++) { const int e = r0 + j * FTL_WAVE + lane; f[j] = e < hi && finishing(a, e); }
#pragma unroll
            for (int j = 0; j < FTL_QK_ROWS; j++) mine += __popcll(__ballot(f[j]));
        }
    if (lane == 0) s_tot[wave] = start ? max(hi - lo, 0) : mine;
    __syncthreads();
    int before = 0, total = 0;                                 // the one pass across the wavefronts
#pragma unroll
    for (int w = 0; w < FTL_QK_THREADS / FTL_WAVE; w++) { const int t = s_tot[w]; before += w < wave ? t : 0; total += t; }
    if (threadIdx.x == 0) s_base = total > 0 ? __hip_atomic_fetch_add(a.q.head, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    if (!start) {
        // sweep 2: the finishing slots in ascending order into `list` (ranked by the same ballots), the masks of the others
        const unsigned long long below = (1ull << lane) - 1ull;
        int pos = before;
        for (int r0 = lo; r0 < hi; r0 += FTL_QK_ROWS * FTL_WAVE) {
            bool f[FTL_QK_ROWS];
#pragma unroll
            for (int j = 0; j < FTL_QK_ROWS; j++) { const int e = r0 + j * FTL_WAVE + lane; f[j] = e < hi && finishing(a, e); }
#pragma unroll
            for (int j = 0; j < FTL_QK_ROWS; j++) {
                const int e = r0 + j * FTL_WAVE + lane;
                const unsigned long long m = __ballot(f[j]);
                if (e < hi) {
                    a.ended[e] = f[j] ? 1 : 0;
                    if (f[j]) a.list[pos + __popcll(m & below)] = e;
                    else a.restarted[e] = 0;
                }
                pos += __popcll(m);
            }
        }
    }
    __syncthreads();                                           // s_base and the list (global memory, this workgroup's own writes)
    // the hand-over of every finishing slot, one per lane: entry base + rank
    for (int i = (int)threadIdx.x; i < total; i += FTL_QK_THREADS) hand_over(a, start ? i : a.list[i], s_base + i);
}

// ftl_queue_start, after the reset: a slot without a ticket steps like a finished env
__global__ void ftl_queue_park_kernel(const Args a) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= a.n_envs || a.q.ticket[e] >= 0) return;
    ftlrs::env_words(a, e)[FTL_EI_DONE] = 1;
    a.done[e] = 1;
}

}  // namespace ftlq

// the kernels' arguments of one call: the shared ones and the queue's own
static ftlq::Args ftl_queue_args(const ftl_handle* h, const ftlrs::Args& r) {
    const size_t waves = FTL_QK_THREADS / FTL_WAVE;
    return ftlq::Args{r, h->queue.v, h->rs.list, (int32_t)align_up(((size_t)h->P.n_envs + waves - 1) / waves, FTL_WAVE)};
}

// FtlChoose of the queue: records and hand-out (MODE_START: every slot takes an entry)
static int ftl_queue_choose(ftl_handle* h, const ftl_outputs* out, const ftl_final_outputs* fin, int mode, void* stream, ftlrs::Args& r) {
    int rc = restart_args(h, r, out, fin, mode, h->queue.calls);
    if (rc) return rc;
    hipLaunchKernelGGL(ftlq::ftl_queue_kernel, dim3(1), dim3(FTL_QK_THREADS), 0, (hipStream_t)stream, ftl_queue_args(h, r));
    return FTL_OK;
}

extern "C" {

size_t ftl_sizeof_episode_record(void) { return sizeof(ftl_episode_record); }
size_t ftl_sizeof_episode_queue(void) { return sizeof(ftl_episode_queue); }

int ftl_set_episode_queue(ftl_handle* h, const ftl_episode_queue* q) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!q) { h->queue.attached = false; return FTL_OK; }
    if (!q->scenario || !q->head || !q->records || !q->ticket) return fail(FTL_E_INVALID, "ftl_episode_queue: scenario / head / records / ticket missing");
    if (q->n <= 0) return fail(FTL_E_INVALID, "ftl_episode_queue: n must be positive");
    if (((uintptr_t)q->records) & 7) return fail(FTL_E_INVALID, "ftl_episode_queue: records must be 8-byte aligned");
    if (!q->stream && (q->stream_base < 0 || q->stream_base + (int64_t)q->n - 1 > 0x7fffffffLL))
        return fail(FTL_E_INVALID, "ftl_episode_queue: stream ids stream_base .. stream_base + n - 1 must lie in 0 .. INT32_MAX");
    h->queue = {*q, true, 0};
    return FTL_OK;
}

int ftl_queue_start(ftl_handle* h, const ftl_outputs* out, void* stream) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!h->queue.attached) return fail(FTL_E_STATE, "ftl_set_episode_queue has not been called");
    ftlrs::Args r;
    int rc = start_chosen(h, out, stream, ftl_queue_choose, r);
    if (rc) return rc;
    hipLaunchKernelGGL(ftlq::ftl_queue_park_kernel, dim3((unsigned)((r.n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ftl_queue_args(h, r));
    return launched();
}

}  // extern "C"
