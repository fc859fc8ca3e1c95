// ftl_restart.hpp -- the one restart path of ftl_step_final.  Included by ftl_abi.hip after launch() (same translation unit: it reads the
// handle), before ftl_queue.hpp and ftl_sampler.hpp.
//
// Finished envs restart after the step in three ways -- same-step (FTL_STEP_AUTO_RESET with final buffers), the episode queue
// (FTL_STEP_QUEUE_RESET), the scenario sampler (FTL_STEP_SAMPLE_RESET) -- and all three are: (1) a step that restarts nothing; (2) for the
// queue and the sampler a small "chooser" kernel that says which slots restart and on which pool entry; (3) with final buffers,
// ftl_final_copy_kernel; (4) a masked reset pass with FTL_CALL_FINISH.  (3) and (4) are finish_step.  A chooser gets the arguments below
// (restart_args), reads the episode a slot has just ended through end_episode, and writes scen_idx and the masks; its start call
// (ftl_queue_start, ftl_sampler_start) is "choose, then ftl_reset" (start_chosen).
#include <hip/hip_runtime.h>

namespace ftlrs {

enum { MODE_STEP = 0, MODE_START = 1 };

struct Args {
    int32_t* env_int; const double* env_dbl; double* ep_stats;   // state fields (record 0 / env 0), as in FtlDevParams
    const int32_t* route_len;       // of the scenario pool: 0 = the world is done at reset
    uint8_t* done; const uint8_t* status;                        // ftl_outputs of the step
    int32_t* scen_idx;              // [n_envs] out: pool index of every slot that restarts (the reset pass's scen_idx)
    uint8_t* ended; uint8_t* restarted;                          // [n_envs] out, every slot: the final buffers' masks, or the scratch's (ended may be null)
    int32_t rec_stride, n_envs, env_id_base, mode;
    int32_t now;                    // the ftl_step* calls that used this chooser since it was attached, this one included
};

__device__ __forceinline__ int* env_words(const Args& a, int e) {
    return reinterpret_cast<int*>(reinterpret_cast<char*>(a.env_int) + (size_t)e * a.rec_stride);
}

// The episode slot e has just ended, from its record and the step's outputs, before the reset pass replaces them.  A world that is done
// at reset (an empty route: the only world g_reset leaves done, ENV:508-510) played nothing: frames, return and status read 0.
struct Ended {
    int scen; bool at_reset;
    int frames; double ret; uint8_t status[3]; uint32_t errors;
};

__device__ __forceinline__ Ended end_episode(const Args& a, int e) {
    const int* ei = env_words(a, e);
    const double* ed = reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.env_dbl) + (size_t)e * a.rec_stride);
    Ended v;
    v.scen = ei[FTL_EI_SCEN];
    v.at_reset = a.route_len[v.scen] == 0;
    v.frames = v.at_reset ? 0 : ei[FTL_EI_STEP_COUNT];
    v.ret = v.at_reset ? 0.0 : ed[FTL_ED_OVERALL_REWARD];
    for (int k = 0; k < 3; k++) v.status[k] = v.at_reset ? 0 : a.status[3 * (size_t)e + k];
    v.errors = (uint32_t)ei[FTL_EI_ERROR];
    if (v.at_reset) a.ep_stats[(size_t)e * FTL_N_METRICS + FTL_M_EPISODES] += 1.0;      // (the step records the others when it raises done)
    return v;
}

}  // namespace ftlrs

// Launches the kernel that fills a.scen_idx (and, MODE_STEP, the masks) on `stream`, after filling `a` with restart_args
typedef int FtlChoose(ftl_handle* h, const ftl_outputs* out, const ftl_final_outputs* fin, int mode, void* stream, ftlrs::Args& a);

// The chooser arguments of one call; MODE_STEP counts the call in `calls`.  The masks go to the final buffers when the caller gave them.
// Allocates the handle's restart scratch at first use.
static int restart_args(ftl_handle* h, ftlrs::Args& a, const ftl_outputs* out, const ftl_final_outputs* fin, int mode, int32_t& calls) {
    a.now = mode == ftlrs::MODE_STEP ? ++calls : calls;
    if (int rc = set_device(h)) return rc;
    if (!h->rs.scen_idx) {
        const size_t n = (size_t)h->P.n_envs, o_list = align_up(n * 4, 256), o_ended = 2 * o_list, o_rest = o_ended + align_up(n, 256);
        char* b = nullptr;
        hipError_t e = hipMalloc((void**)&b, o_rest + align_up(n, 256));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(restart scratch): ") + hipGetErrorString(e));
        h->rs = {(int32_t*)b, (int32_t*)(b + o_list), (uint8_t*)b + o_ended, (uint8_t*)b + o_rest};
    }
    a.env_int = h->P.env_int; a.env_dbl = h->P.env_dbl; a.ep_stats = h->P.ep_stats; a.route_len = h->P.scen.route_len;
    a.done = out->done; a.status = out->status;
    a.scen_idx = h->rs.scen_idx; a.ended = fin ? fin->ended : h->rs.ended; a.restarted = fin ? fin->restarted : h->rs.restarted;
    a.rec_stride = h->P.rec_stride; a.n_envs = h->P.n_envs; a.env_id_base = h->P.cfg.env_id_base; a.mode = mode;
    return FTL_OK;
}

// After the step `step` (one that restarted nothing) was launched on `stream`: the terminal rows go to `fin`, then the reset pass
// re-initialises the slots of `mask` -- on scen_idx[slot], or, scen_idx null, on the next entry of the reset window's walk.
static int finish_step(ftl_handle* h, const FtlCall& step, const ftl_outputs* out, const ftl_final_outputs* fin, const int32_t* scen_idx,
                       const uint8_t* mask, void* stream) {
    if (fin) {
        const int n = h->P.n_envs, epb = FTL_FC_THREADS;                  // envs per workgroup (64 per wavefront)
        const int pol_len = (fin->policy_obs && out->policy_obs) ? h->P.pol_h * h->P.pol_width : 0;
        hipLaunchKernelGGL(ftl::ftl_final_copy_kernel, dim3((unsigned)((n + epb - 1) / epb)), dim3(FTL_FC_THREADS), 0, (hipStream_t)stream,
                           *out, *fin, n, h->P.lasers_len, pol_len);
    }
    FtlCall rcall = step;
    rcall.mode = 1; rcall.flags = FTL_CALL_FINISH | (scen_idx ? FTL_CALL_SCEN_IDX : 0u) | (step.flags & FTL_STEP_NO_SENSORS);   // a blind step's reset pass is blind too
    rcall.scen_idx = scen_idx; rcall.mask = mask;
    rcall.action = nullptr; rcall.ended = nullptr; rcall.restarted = nullptr;
    return launch(h, rcall, stream);
}

// ftl_queue_start / ftl_sampler_start after their own first checks: every slot chooses, then ftl_reset on what it chose (ftl_reset
// checks policy_obs, as it always has for these calls: after the chooser's launch)
static int start_chosen(ftl_handle* h, const ftl_outputs* out, void* stream, FtlChoose* choose, ftlrs::Args& a) {
    int rc = check_ready(h, out, false);
    if (rc) return rc;
    rc = choose(h, out, nullptr, ftlrs::MODE_START, stream, a);
    return rc ? rc : ftl_reset(h, a.scen_idx, nullptr, out, stream);
}
