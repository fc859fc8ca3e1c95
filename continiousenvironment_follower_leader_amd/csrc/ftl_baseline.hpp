// ftl_baseline.hpp -- the reference's way-point chase ("base algorithm", run_2d.py --mode base, lines 109-151, around
// utils/misc.py:move_to_the_point, MISC:65-95) as a policy on the device (ftl_baseline_act) and as closed-loop rollouts with one call
// (ftl_rollout_baseline); the contract is in include/ftl.h.  Included by ftl_abi.hip after ftl_rollout.hpp (same translation unit: it
// reads the handle and hands its act kernels to rollout_loop, which owns the steps and the fold).
//
// ftl_baseline_kernel: one thread per env.  It reads the env's step word (env_int + e * rec_stride: an env index, not a slot of the cost
// permutation), three floats of its obs_num row and its target, reads and writes its follower row (16 + 16 * cap bytes) and writes 16
// bytes of action.  Neighbouring lanes read rows that lie a row stride apart, so nothing here coalesces; per env it touches a handful of
// cache lines against the kilobytes of a step.  ftl_baseline_guided_kernel (ftl_baseline_act_guided, ftl_rollout_guided) is the same
// bookkeeping and decision -- one __device__ function, decide() -- with the action clipped to the Box(2), a residual added, clipped again.
//
// v = distance.euclidean(position, next_point) is BLAS dnrm2 on x87 in the reference (oracle/ftl_oracle.c, numeric notes): squares and sum
// in a 64-bit mantissa, sqrtl, one more rounding to double.  The device has no such format, so it returns the correctly rounded
// sqrt(dx^2 + dy^2) of the two float64 differences: exact squares (fma), their sum in double-double, the square root of the leading part
// corrected by the exact residual, one final rounding.  The two agree unless the x87 value rounds twice across a tie of the double grid
// (about 2^-12 of random inputs); then they are one ulp apart.  (The correction is itself a rounded double: a sum within 2^-50 ulp of a
// tie could round the other way.  Nothing measurable.)
#include <hip/hip_runtime.h>

#include "ftl_crmath.hpp"

namespace ftlbl {

struct Args {
    const int32_t* env_int; int32_t rec_stride, n_envs, cap;   // state: the step word of record 0, as in FtlDevParams
    const float* obs_num; const double* target;                // ftl_outputs of the last reset / step
    unsigned char* bl;       // [n_envs] rows of {int32 head, count, pending, flags} + cap points of two doubles
    double* action;          // [n_envs][2]
};

__device__ __forceinline__ double euclid_cr(double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    const ftl_cr::dd s = ftl_cr::add(ftl_cr::two_prod(dx, dx), ftl_cr::two_prod(dy, dy));
    if (!(s.hi > 0.0) || s.hi > 1.0e300) return sqrt(s.hi);    // 0, NaN, about to overflow: nothing to correct
    const double q = sqrt(s.hi);
    const double r = fma(-q, q, s.hi) + s.lo;                  // the residual of a correctly rounded root is a double
    return q + r / (2.0 * q);
}

// The bookkeeping and the decision of env e (e < n_envs): reads and writes the env's follower row, returns the unclipped action (v, w).
// What ftl_baseline_kernel and ftl_baseline_guided_kernel share.
__device__ __forceinline__ double2 decide(const Args& a, const int e) {
    const int cap = a.cap;
    unsigned char* row = a.bl + (size_t)e * (16 + 16 * (size_t)cap);
    int32_t* w = reinterpret_cast<int32_t*>(row);
    double* pts = reinterpret_cast<double*>(row + 16);
    // whatever the words hold, every index below stays inside the row
    int head = (int)((uint32_t)w[0] % (uint32_t)cap), count = w[1] < 0 ? 0 : (w[1] > cap ? cap : w[1]), pending = w[2];
    uint32_t flags = (uint32_t)w[3];
    const int32_t* ei = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(a.env_int) + (size_t)e * a.rec_stride);
    const double tx = a.target[2 * (size_t)e], ty = a.target[2 * (size_t)e + 1];
    if (ei[FTL_EI_STEP_COUNT] == 0 || count == 0) {            // a reset observation (run_2d.py:119-122), or a zeroed row
        head = 0; count = 1;
        pts[0] = tx; pts[1] = ty;
    } else {                                                   // the bookkeeping of the step just taken (run_2d.py:141-145)
        const int back = (head + count - 1) % cap;
        if (tx != pts[2 * back] || ty != pts[2 * back + 1]) {
            if (count == cap) { head = (head + 1) % cap; count--; flags |= FTL_BL_OVERFLOW; }
            const int at = (head + count) % cap;
            pts[2 * at] = tx; pts[2 * at + 1] = ty;
            count++;
        }
        if (pending) {
            if (count > 1) { head = (head + 1) % cap; count--; }
            else flags |= FTL_BL_EMPTY;
        }
    }
    const float* num = a.obs_num + (size_t)e * FTL_OBS_NUM;
    const double px = (double)num[5], py = (double)num[6], fx = pts[2 * head], fy = pts[2 * head + 1];
    const int cur = (int)num[8];
    const int desirable = (int)ftl::angle_to_point(px, py, fx, fy);
    int delta = 0, sign = 0;                                   // MISC:73-91
    if (desirable - cur > 0) {
        if (desirable - cur > 180) { delta = cur + (360 - desirable); sign = -1; }
        else { delta = desirable - cur; sign = 1; }
    } else if (desirable - cur < 0) {
        if (cur - desirable > 180) { sign = 1; delta = (360 - cur) + desirable; }
        else { sign = -1; delta = cur - desirable; }
    }
    const double v = euclid_cr(px, py, fx, fy);
    w[0] = head; w[1] = count; w[2] = v <= 20.0 ? 1 : 0; w[3] = (int32_t)flags;
    return make_double2(v, (double)(delta * sign) / 10.0);
}

__global__ __launch_bounds__(256) void ftl_baseline_kernel(const Args a) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= a.n_envs) return;
    const double2 x = decide(a, e);
    a.action[2 * (size_t)e] = x.x;
    a.action[2 * (size_t)e + 1] = x.y;
}

// ftl_baseline_act_guided: the same row bookkeeping and decision, then the action clipped to the Box(2), the residual added, clipped again
struct GuidedArgs {
    Args b;
    const double* resid;     // [n_envs][2]
    double lo0, hi0, lo1, hi1;
};

__global__ __launch_bounds__(256) void ftl_baseline_guided_kernel(const GuidedArgs g) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= g.b.n_envs) return;
    const double2 x = decide(g.b, e);
    const double r0 = g.resid[2 * (size_t)e], r1 = g.resid[2 * (size_t)e + 1];
    g.b.action[2 * (size_t)e] = fmin(fmax(fmin(fmax(x.x, g.lo0), g.hi0) + r0, g.lo0), g.hi0);
    g.b.action[2 * (size_t)e + 1] = fmin(fmax(fmin(fmax(x.y, g.lo1), g.hi1) + r1, g.lo1), g.hi1);
}

}  // namespace ftlbl

static size_t baseline_row_bytes(int32_t cap) { return 16 + 16 * (size_t)cap; }

// the checks ftl_baseline_act and ftl_rollout_baseline share; fills the kernel's arguments but for `action`
static int baseline_args(ftl_handle* h, const ftl_outputs* out, void* bl, size_t bl_bytes, int32_t cap, ftlbl::Args& a) {
    if (!h || !out || !bl) return fail(FTL_E_INVALID, "null argument");
    if (cap < 2) return fail(FTL_E_INVALID, "baseline follower: cap must be at least 2");
    if (bl_bytes < (size_t)h->P.n_envs * baseline_row_bytes(cap)) return fail(FTL_E_INVALID, "baseline follower: state buffer too small (ftl_baseline_bytes)");
    if (((uintptr_t)bl) & 7) return fail(FTL_E_INVALID, "baseline follower: state buffer must be 8-byte aligned");
    if (int rc = check_ready(h, out)) return rc;
    a.env_int = h->P.env_int; a.rec_stride = h->P.rec_stride; a.n_envs = h->P.n_envs; a.cap = cap;
    a.obs_num = out->obs_num; a.target = out->target; a.bl = (unsigned char*)bl; a.action = nullptr;
    return FTL_OK;
}

// the Box(2) bounds of ENV:374-378 (those of ftl_search_sample and of the env's own clip)
static void baseline_box(const ftl_handle* h, ftlbl::GuidedArgs& g) {
    const ftl_robot_params& f = h->P.cfg.follower;
    g.lo0 = f.min_speed; g.hi0 = f.max_speed; g.lo1 = -f.max_rotation_speed; g.hi1 = f.max_rotation_speed;
}

extern "C" {

size_t ftl_baseline_bytes(const ftl_handle* h, int32_t cap) { return (h && cap >= 2) ? (size_t)h->P.n_envs * baseline_row_bytes(cap) : 0; }

int ftl_baseline_act(ftl_handle* h, const ftl_outputs* out, void* bl, size_t bl_bytes, int32_t cap, double* action, void* stream) {
    if (!action) return fail(FTL_E_INVALID, "null argument");
    ftlbl::Args a;
    if (int rc = baseline_args(h, out, bl, bl_bytes, cap, a)) return rc;
    if (int rc = set_device(h)) return rc;
    a.action = action;
    hipLaunchKernelGGL(ftlbl::ftl_baseline_kernel, dim3((unsigned)((h->P.n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launched();
}

int ftl_baseline_act_guided(ftl_handle* h, const ftl_outputs* out, void* bl, size_t bl_bytes, int32_t cap, const double* resid, double* action,
                            void* stream) {
    if (!action || !resid) return fail(FTL_E_INVALID, "null argument");
    if (((uintptr_t)resid) & 7) return fail(FTL_E_INVALID, "ftl_baseline_act_guided: resid must be 8-byte aligned");
    ftlbl::GuidedArgs g;
    if (int rc = baseline_args(h, out, bl, bl_bytes, cap, g.b)) return rc;
    if (int rc = set_device(h)) return rc;
    g.b.action = action; g.resid = resid;
    baseline_box(h, g);
    hipLaunchKernelGGL(ftlbl::ftl_baseline_guided_kernel, dim3((unsigned)((h->P.n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
    return launched();
}

}  // extern "C"

// ftl_rollout_baseline (T steps, no residual) and ftl_rollout_guided: steps 0 .. T-1 add resid + t * resid_step_bytes when `resid` is given,
// steps T .. T+tail-1 are the plain baseline; one fold, one discount across both parts.  `name` heads the messages.  The loop is
// rollout_loop of ftl_rollout.hpp; what is here is the action of step t: the act kernel of its part, into the caller's record or bl_action.
static int baseline_rollout(const char* name, ftl_handle* h, int32_t T, int32_t tail, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro,
                            void* bl, size_t bl_bytes, int32_t cap, const double* resid, int64_t resid_step_bytes, double* actions,
                            int64_t step_bytes, uint32_t flags, void* stream) {
    if (!h || !out || !bl) return fail(FTL_E_INVALID, "null argument");
    if (int rc = rollout_check(name, ro, T, tail, flags)) return rc;
    if (actions && step_bytes < (int64_t)h->P.n_envs * 16) return fail(FTL_E_INVALID, std::string(name) + ": step_bytes below one block of [n_envs][2] doubles");
    if (resid && resid_step_bytes < (int64_t)h->P.n_envs * 16) return fail(FTL_E_INVALID, std::string(name) + ": resid_step_bytes below one block of [n_envs][2] doubles");
    if (resid && ((((uintptr_t)resid) | (uintptr_t)resid_step_bytes) & 7)) return fail(FTL_E_INVALID, std::string(name) + ": resid and resid_step_bytes must be 8-byte aligned");
    ftlbl::GuidedArgs g;
    ftlbl::Args& b = g.b;
    if (int rc = baseline_args(h, out, bl, bl_bytes, cap, b)) return rc;
    baseline_box(h, g);
    const int32_t guided = resid ? T : 0;
    if (int rc = set_device(h)) return rc;
    if (!actions && !h->bl_action) {
        hipError_t e = hipMalloc((void**)&h->bl_action, align_up((size_t)h->P.n_envs * 16, 256));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(baseline actions): ") + hipGetErrorString(e));
    }
    const dim3 grid((unsigned)((h->P.n_envs + 255) / 256));
    return rollout_loop(h, FTL_ACTION_BOX2, T + tail, gamma, out, ro, flags, false, stream, [&](int32_t t) {
        b.action = actions ? (double*)((char*)actions + (int64_t)t * step_bytes) : h->bl_action;
        if (t < guided) {
            g.resid = (const double*)((const char*)resid + (int64_t)t * resid_step_bytes);
            hipLaunchKernelGGL(ftlbl::ftl_baseline_guided_kernel, grid, dim3(256), 0, (hipStream_t)stream, g);
        } else hipLaunchKernelGGL(ftlbl::ftl_baseline_kernel, grid, dim3(256), 0, (hipStream_t)stream, b);
        return b.action;
    });
}

extern "C" {

int ftl_rollout_baseline(ftl_handle* h, int32_t T, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro,
                         void* bl, size_t bl_bytes, int32_t cap, double* actions, int64_t step_bytes, uint32_t flags, void* stream) {
    return baseline_rollout("ftl_rollout_baseline", h, T, 0, gamma, out, ro, bl, bl_bytes, cap, nullptr, 0, actions, step_bytes, flags, stream);
}

int ftl_rollout_guided(ftl_handle* h, int32_t T, int32_t tail, double gamma, const ftl_outputs* out, const ftl_rollout_outputs* ro,
                       void* bl, size_t bl_bytes, int32_t cap, const double* resid, int64_t resid_step_bytes, double* actions, int64_t step_bytes,
                       uint32_t flags, void* stream) {
    return baseline_rollout("ftl_rollout_guided", h, T, tail, gamma, out, ro, bl, bl_bytes, cap, resid, resid_step_bytes, actions, step_bytes, flags, stream);
}

}  // extern "C"
