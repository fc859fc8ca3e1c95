// ftl_abi.hip -- host side of the C-ABI declared in include/ftl.h: config validation, state layout, kernel launch.
// There is no CPU fallback anywhere in this file: every entry point that computes launches the HIP kernel.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <cstdlib>
#include <cmath>

#include "ftl_device.hpp"
#include "ftl_frames_group.hpp"
#include "ftl_aux.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }

struct Field { const char* name; size_t offset, per_env; int dtype; size_t stride; };     // stride: bytes from one env's row to the next

// The state fields, one row each: name (= the pointer member of FtlDevParams), dtype (0 int32, 1 float32, 2 float64), element size, "part
// of the per-env record".  The order is that of ftl_state_field, of the snapshot rows and of ftl_env_layout_id: new fields go to the end.
#define FTL_FIELDS(X) \
    X(rb_pos, 1, 4, true) X(rb_dbl, 2, 8, true) X(rb_int, 0, 4, true) X(env_int, 0, 4, true) X(env_dbl, 2, 8, true) \
    X(traj, 1, 4, false) X(hist, 2, 8, false) X(corr, 2, 8, false) X(snap_rects, 0, 4, true) X(snap_win, 0, 4, true) \
    X(traj_bb, 1, 4, false) X(ep_stats, 2, 8, false) X(hist1, 1, 4, false) X(fol_cs, 2, 8, true) X(corr32, 1, 4, false)
#define X(n, dtype, esz, rec) F_##n,
enum { FTL_FIELDS(X) FTL_N_FIELDS };
#undef X
struct FieldSpec { const char* name; int dtype; size_t esz; bool rec; size_t ptr; };      // ptr: where FtlDevParams keeps the field's pointer
#define X(n, dtype, esz, rec) {#n, dtype, esz, rec, offsetof(FtlDevParams, n)},
constexpr FieldSpec kFields[FTL_N_FIELDS] = {FTL_FIELDS(X)};
#undef X
// the per-env record, the ray kernel's inputs first
constexpr int kRecOrder[] = {F_env_int, F_fol_cs, F_rb_pos, F_rb_dbl, F_snap_win, F_snap_rects, F_env_dbl, F_rb_int};

// The environment switches, read once by ftl_create.  -1 = not given: a given 0 / 1 wins over the library's rule and over ftl_tune.
struct Switches {
    int split, no_regroup, g8, one_pass, defer;                       // FTL_SPLIT, FTL_NO_REGROUP, FTL_DEBUG_G8, FTL_RAYS_ONE_PASS, FTL_DEFER
    int class_cull;                                                   // FTL_RAYS_CLASS_CULL
    int regroup_every, corr_lds_cap, lds_pad, lds_pad_rays;            // FTL_REGROUP_EVERY, FTL_DEBUG_CORR_LDS_CAP, FTL_DEBUG_LDS_PAD[_RAYS] (0: not given)
    int pair_window;                                                  // FTL_DEBUG_PAIR_WINDOW (0: not given)
    bool print_lds;                                                   // FTL_DEBUG_PRINT_LDS
    int trk_running; double trk_band;                                 // FTL_TRK_RUNNING, FTL_DEBUG_TRK_BAND (pixels; 0: not given)
};

Switches read_switches() {
    auto tri = [](const char* name, int other) { const char* v = getenv(name); return !v ? -1 : v[0] == '1' ? 1 : v[0] == '0' ? 0 : other; };
    auto num = [](const char* name, int hi) { const char* v = getenv(name); const int p = v ? atoi(v) : 0; return p < 0 ? 0 : (p > hi ? hi : p); };
    auto px = [](const char* name) { const char* v = getenv(name); const double p = v ? atof(v) : 0.0; return p > 0.0 && p < 1024.0 ? p : 0.0; };
    return Switches{tri("FTL_SPLIT", 0), tri("FTL_NO_REGROUP", 0), tri("FTL_DEBUG_G8", 0), tri("FTL_RAYS_ONE_PASS", 1), tri("FTL_DEFER", 1),
                    tri("FTL_RAYS_CLASS_CULL", 1),
                    num("FTL_REGROUP_EVERY", INT32_MAX), num("FTL_DEBUG_CORR_LDS_CAP", INT32_MAX), num("FTL_DEBUG_LDS_PAD", 48 * 1024),
                    num("FTL_DEBUG_LDS_PAD_RAYS", 48 * 1024), num("FTL_DEBUG_PAIR_WINDOW", FTL_PAIR_CAP), getenv("FTL_DEBUG_PRINT_LDS") != nullptr,
                    tri("FTL_TRK_RUNNING", 1), px("FTL_DEBUG_TRK_BAND")};
}

// What ftl_create and ftl_tune decide about the frame kernel and the cost sort: plan_schedule()
struct Schedule {
    int G, epw, rg_slots;    // lanes per env (4 or 8), envs per wavefront, frame-kernel wavefronts one round holds on this device
    int32_t fr_rec_off, fr_rec_stride, fr_pend_off, fr_env_off, fr_defer, fr_lds;   // the kernel's LDS layout (FtlDevParams has the meanings)
    bool regroup, fits;      // envs are regrouped by expected cost after every rg_every-th launch; fr_lds is within the 64 KiB of a workgroup
};

// The template arguments of the kernels a handle launches, as values: frame_inst(), rays_inst()
struct FrameInst { int G; bool reg, xr; };
struct RaysInst { int hm; bool expl, split, capped, one_pass, mask; };
typedef void (*FtlKernel)(const FtlDevParams*, const FtlCall);

}  // namespace

// a restart source the caller attached (ftl_queue.hpp, ftl_sampler.hpp): its struct, and the ftl_step* calls that used it since the attach
template <typename T> struct FtlAttached { T v; bool attached; int32_t calls; };
struct FtlRestartScratch { int32_t* scen_idx; int32_t* list; uint8_t* ended; uint8_t* restarted; };   // [n_envs] each, one allocation: scen_idx is its base

struct ftl_handle {
    FtlDevParams P;          // host copy of the frozen parameters
    FtlDevParams* dP;        // device copy read by the kernel (library-owned, ~1 KB)
    bool dirty;
    int device;
    size_t state_bytes;
    Field fields[FTL_N_FIELDS];
    void* mt_mem;            // partial sums of ftl_episode_metrics (library-owned)
    bool timing;             // ftl_kernel_timing: events around every launch of a step
    std::vector<hipEvent_t> tev;   // 5 per timed step: before frames | after frames | after rays | after aux | after regroup
    size_t tev_used;
    bool bound, have_scen;
    Switches sw;             // the environment switches as ftl_create found them
    Schedule sched;          // the committed plan_schedule() of (co_envs, cus): P.fr_* are its copy for the kernel
    int co_envs, cus;        // envs stepped on the device at the same time (ftl_tune; default: this handle's), CUs of the device
    bool one_pass;           // all ray sensors sit on one side of the tracker, and FTL_RAYS_ONE_PASS=0 is not set
    // what launch() launches (apply_plan): the frame kernel without / with XR, the ray kernel of one-stream / two-stream launches
    // (null: no ray sensors), "the config has a compas / lidar / detector sensor", "the config has the v1 tracker"
    FtlKernel k_frames[2], k_rays[2]; RaysInst rays[2];
    bool has_aux, has_trk1;
    void* rg_mem;            // perm | bh | rank | keys | two key-total buffers (library-owned)
    int* rg_tot;             // [2][FTL_NKEYS]
    unsigned rg_parity, rg_launches, rg_every;
    // optionally the slot groups are stepped as two interleaved halves on two streams (the caller's stream waits for the side
    // stream): the ray kernel of one half fills the tail of the other half's frame kernel
    hipStream_t side; hipEvent_t ev_fork, ev_join; bool split;
    int win_base, win_count, win_stride; // pool entries the auto-reset draws from (ftl_set_reset_window)
    float* last_lasers;      // ftl_outputs.lasers of the last ftl_reset / ftl_step* call (ftl_render's hit points)
    FtlAttached<ftl_episode_queue> queue;         // ftl_set_episode_queue
    FtlAttached<ftl_scenario_sampler> sampler;    // ftl_set_scenario_sampler
    FtlRestartScratch rs;    // what a queue or sampler call hands to the reset pass (library-owned, allocated by the first such call: ftl_restart.hpp)
    uint8_t* ro_alive;       // [n_envs] "the episode was running on entry to the step" of ftl_rollout (library-owned, allocated by the first rollout: ftl_rollout.hpp)
    double* bl_action;       // [n_envs][2] the actions of ftl_rollout_baseline when the caller keeps no record (library-owned, allocated on first use: ftl_baseline.hpp)
};

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The first and the last line of every entry that launches.  set_device: the device of the handle (an ftl_handle or an ftl_gz_handle)
// becomes the thread's current one.  launched: the runtime accepted every launch since the last such check.
template <typename H> int set_device(const H* h) {
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return FTL_OK;
}

int launched() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
    return FTL_OK;
}

int validate(const ftl_config& c, std::string& why) {
    char buf[256];
#define REQ(cond, ...) do { if (!(cond)) { snprintf(buf, sizeof buf, __VA_ARGS__); why = buf; return FTL_E_INVALID; } } while (0)
    REQ(c.abi_version == FTL_ABI_VERSION, "abi_version %d != %d", c.abi_version, FTL_ABI_VERSION);
    REQ(c.width > 0 && c.height > 0, "bad field size");
    REQ(c.frames_per_step > 0, "frames_per_step must be positive");
    REQ(c.rand_fps_hi == 0 || (c.rand_fps_lo > 0 && c.rand_fps_lo < c.rand_fps_hi), "random_frames_per_step must be (low, high) with 0 < low < high");
    REQ(c.trajectory_saving_period > 0, "trajectory_saving_period must be positive");
    REQ(c.n_static >= 0 && c.n_static <= 4096, "n_static out of range");
    REQ(c.n_bears >= 0 && c.n_bears <= FTL_MAX_BEARS, "n_bears out of range (0..%d)", FTL_MAX_BEARS);
    REQ(c.n_lasers >= 0 && c.n_lasers <= FTL_MAX_LASERS, "n_lasers out of range");
    REQ(c.n_lasers == 0 || c.has_tracker, "ray sensors need the tracker (classes.py:280 would raise NameError)");
    REQ(c.traj_cap >= 8, "traj_cap %d is below 8", c.traj_cap);
    REQ(c.corr_cap >= 8, "corr_cap %d is below 8", c.corr_cap);
    REQ(c.corr_cap <= FTL_MAX_CORR_CAP, "corr_cap %d is above the limit of %d points (FTL_MAX_CORR_CAP)", c.corr_cap, FTL_MAX_CORR_CAP);
    REQ(c.route_cap >= 2, "route_cap %d is below 2", c.route_cap);
    REQ(c.init_traj_cap >= 1, "init_traj_cap %d is below 1", c.init_traj_cap);
    REQ((c.corr_cap & (c.corr_cap - 1)) == 0, "corr_cap must be a power of two (the tracker rings are indexed with a mask)");
    REQ(c.init_traj_cap <= c.traj_cap, "init_traj_cap > traj_cap");
    REQ(c.traj_cap % FTL_TRAJ_BLOCK == 0, "traj_cap must be a multiple of FTL_TRAJ_BLOCK");
    if (c.has_tracker == 2) {
        REQ(c.tracker_saving_period > 0, "tracker saving_period must be positive");
        REQ(c.corridor_length > 0 && c.corridor_width > 0, "corridor_length / corridor_width must be positive");
    }
    REQ(c.n_speed_regime <= FTL_MAX_REGIME && c.n_acc_regime <= FTL_MAX_REGIME, "too many regime entries");
    REQ(c.has_tracker >= 0 && c.has_tracker <= 2, "has_tracker must be 0, 1 (v1) or 2 (v2)");
    if (c.has_tracker == 1) REQ(c.tracker_saving_period > 0 && c.hist1_cap >= 8 && c.corridor_width > 0, "bad v1 tracker parameters");
    REQ(c.n_aux >= 0 && c.n_aux <= FTL_MAX_AUX, "n_aux out of range");
    for (int j = 0; j < c.n_aux; j++) {
        const ftl_aux_cfg& a = c.aux[j];
        REQ(a.kind >= FTL_AUX_LIDAR && a.kind <= FTL_AUX_TRACK_RADAR, "aux %d: unknown sensor kind", j);
        if (a.kind == FTL_AUX_LIDAR) {
            REQ(a.n_angles > 0 && a.n_angles <= 512 && a.points_number > 0 && a.range_px > 0, "aux %d: bad lidar parameters", j);
            // the (ray, marching point) index of the lidar is split with a float quotient that is exact below 2^16 items (ftl_aux.hpp)
            REQ(a.points_number <= 1024 && a.n_angles * a.points_number < 65536, "aux %d: lidar with more than 1024 points per ray or 65535 (ray, point) pairs", j);
        }
        else {
            REQ(c.has_tracker != 0, "aux %d: a leader-track detector needs a tracker (classes.py:272 would raise NameError)", j);
            REQ(a.seq_len > 0 && a.detectable >= 0 && a.detectable <= (a.kind == FTL_AUX_TRACK_RADAR ? 2 : 1), "aux %d: bad detector parameters", j);
            if (a.kind == FTL_AUX_TRACK_RADAR) REQ(a.radar_sectors > 0 && a.radar_sectors <= 4096, "aux %d: bad radar_sectors_number", j);
        }
    }
    for (int k = 0; k < c.n_lasers; k++) {
        const ftl_laser_cfg& l = c.lasers[k];
        REQ(l.count > 0 && l.count <= 1024, "laser %d: bad lasers_count", k);
        REQ(l.history > 0 && l.history <= FTL_HMAX, "laser %d: max_prev_obs must be in 1..%d", k, FTL_HMAX);
        REQ(l.react_obstacles >= 0 && l.react_obstacles <= 3, "laser %d: bad react_to_obstacles", k);
        REQ(l.length > 0, "laser %d: bad laser_length", k);
    }
#undef REQ
    return FTL_OK;
}

int frames_max(const ftl_config& c) { return c.rand_fps_hi > 0 ? c.rand_fps_hi - 1 : c.frames_per_step; }      // frames of the longest step

// The schedule of a handle of n_envs envs that shares a device of `cus` CUs with co_envs envs in all.  Pure: ftl_create and ftl_tune
// commit what it returns (apply_plan).
// Lanes per env (G): configs with more than 2 dynamic obstacles need 8.  The others take 8 as well -- 8 envs per wavefront, five lanes of
// a group idle -- when the batch is small enough for every such wavefront to have a SIMD of its own: the launch then takes as long as its
// slowest wavefront, and a wavefront with half the envs meets half the rare paths (resets, searches, walks): config B at 8,192 envs +3 %,
// config D +4 %, nothing from 16,384 envs on.  FTL_DEBUG_G8=0/1 overrides.
// Cost sort (regroup): it pays when the frame kernel runs in more than one round of wavefronts (the long ones start first, the short ones
// fill in behind them: +10 % on config B at 65,536 envs).  When every wavefront is resident from the start the launch takes as long as its
// slowest wavefront, and a wavefront that holds ALL the expensive envs is slower than any wavefront of an unsorted batch: config E at
// 32,768 envs -9 %, config D at 4,096 envs -16 % with the sort.  So it is on only beyond one round -- or with random frame counts, whose
// keys make the wavefronts uniform in length.  FTL_NO_REGROUP=0/1 overrides.  (The scatter pass reads one histogram row per block of
// 1024 envs: fine up to a few hundred blocks.)
Schedule plan_schedule(const ftl_config& cfg, int R, int n_envs, int co_envs, int cus, const Switches& sw) {
    Schedule s;
    s.G = (R > 4 || (sw.g8 >= 0 ? sw.g8 == 1 : co_envs <= cus * 4 * 8)) ? 8 : 4;
    s.epw = FTL_WAVE / s.G;
    const int f_max = frames_max(cfg);
    // The searches of frames 1.. wait for the end of the step when the step is short enough for their items to sit in LDS and the frame
    // count is the same for every env; otherwise every frame's searches run right after it (one item per env at most).  FTL_DEFER=0: never.
    s.fr_defer = (cfg.rand_fps_hi == 0 && f_max >= 2 && f_max <= 16 && cfg.traj_cap <= 65535 && sw.defer != 0) ? 1 : 0;
    // LDS: near lists + their counters | frame records (one byte per env and frame) | pending position checks | slot -> env, item counter,
    // box of the trajectory block being filled
    size_t o = align_up((size_t)s.epw * cfg.n_static * 16 + (size_t)s.epw * 4 + 32, 16);
    s.fr_rec_stride = (int)align_up((size_t)f_max, 16);
    s.fr_rec_off = (int)o; o += (size_t)s.fr_rec_stride * s.epw;
    s.fr_pend_off = (int)o; o += (size_t)s.epw * (s.fr_defer ? f_max - 1 : 1) * 16;
    s.fr_env_off = (int)o; o += (size_t)s.epw * 4 + 16 + (size_t)s.epw * 16;
    s.fr_lds = (int)o;
    s.fits = o <= 64 * 1024;
    s.rg_slots = cus * 4 * FTL_FRAMESG_WPE;
    s.regroup = (sw.no_regroup >= 0 ? sw.no_regroup == 0 : ((co_envs + s.epw - 1) / s.epw > s.rg_slots || cfg.rand_fps_hi > 0))
                && (n_envs + FTL_RG_BLOCK - 1) / FTL_RG_BLOCK <= 512;
    return s;
}

// Which instantiation of the frame kernel runs: G lanes per env, REG = the config has leader regimes or random frame counts, XR = the call
// restarts finished envs on a later call or writes the masks (ftl_frames_group.hpp)
FrameInst frame_inst(const ftl_config& c, int G, bool xr) { return FrameInst{G, c.n_speed_regime >= 0 || c.n_acc_regime >= 0 || c.rand_fps_hi > 0, xr}; }

bool call_xr(const FtlCall& c) { return (c.flags & (FTL_STEP_NEXT_RESET | FTL_CALL_DEFER_RESET | FTL_CALL_FINISH)) != 0 || c.ended || c.restarted; }

// Which instantiation of the ray kernel runs (DESIGN.md has the table).  expl: a sensor with explicit angles, padded sectors or a compas
// is in the config; capped: the LDS copy of the corridor ring is smaller than the ring; two_streams: the launch covers one half of the slot
// groups.  Only the one-stream kernels of the common sensors exist in every HM and without the loop over the passes; of those, the
// one-pass ones also exist in the mask form of phase 3, which a pass of at most 64 rays (pass_rays) runs.
RaysInst rays_inst(int hmax, bool expl, bool capped, bool two_streams, bool one_pass, int pass_rays) {
    const int wide = hmax <= 5 ? 5 : FTL_HMAX;
    if (two_streams) return (!expl && hmax > 5 && hmax <= 10) ? RaysInst{10, false, true, capped, false, false} : RaysInst{wide, true, true, capped, false, false};
    if (expl) return RaysInst{wide, true, false, capped, false, false};
    return RaysInst{hmax <= 5 ? 5 : hmax <= 8 ? 8 : hmax <= 10 ? 10 : FTL_HMAX, false, false, capped, one_pass, one_pass && pass_rays <= 64};
}

// The instantiations: 2 x 2 x 2 of the frame kernel, and of the ray kernel the 3 + 2 + 4 x 3 (HM, EXPL, SPLIT, ONE_PASS, MASK) rows that
// rays_inst can return, each with and without CAPPED
template <bool XR> FtlKernel frame_kernel_x(int G, bool reg) {
    if (G == 4) return reg ? ftl_frames_group_kernel<4, true, XR> : ftl_frames_group_kernel<4, false, XR>;
    return reg ? ftl_frames_group_kernel<8, true, XR> : ftl_frames_group_kernel<8, false, XR>;
}
FtlKernel frame_kernel(const FrameInst& f) { return f.xr ? frame_kernel_x<true>(f.G, f.reg) : frame_kernel_x<false>(f.G, f.reg); }

template <int HM, bool EXPL, bool SPLIT, bool ONE, bool MASK = false> FtlKernel rays_kernel_c(bool capped) {
    return capped ? ftl_rays_kernel<HM, EXPL, SPLIT, true, ONE, MASK> : ftl_rays_kernel<HM, EXPL, SPLIT, false, ONE, MASK>;
}
template <int HM> FtlKernel rays_kernel_1(const RaysInst& r) {
    if (r.mask) return rays_kernel_c<HM, false, false, true, true>(r.capped);
    return r.one_pass ? rays_kernel_c<HM, false, false, true>(r.capped) : rays_kernel_c<HM, false, false, false>(r.capped);
}
FtlKernel rays_kernel(const RaysInst& r) {
    if (r.split) return r.hm == 10 ? rays_kernel_c<10, false, true, false>(r.capped) : r.hm == 5 ? rays_kernel_c<5, true, true, false>(r.capped) : rays_kernel_c<FTL_HMAX, true, true, false>(r.capped);
    if (r.expl) return r.hm == 5 ? rays_kernel_c<5, true, false, false>(r.capped) : rays_kernel_c<FTL_HMAX, true, false, false>(r.capped);
    return r.hm == 5 ? rays_kernel_1<5>(r) : r.hm == 8 ? rays_kernel_1<8>(r) : r.hm == 10 ? rays_kernel_1<10>(r) : rays_kernel_1<FTL_HMAX>(r);
}

// Plans for co_envs co-scheduled envs.  A plan whose LDS layout fits is committed, with the kernels that go with it and what the config
// says about the other launches; otherwise the handle stays exactly as it was.
int apply_plan(ftl_handle* h, int co_envs) {
    FtlDevParams& P = h->P;
    const ftl_config& c = P.cfg;
    const Schedule s = plan_schedule(c, P.R, P.n_envs, co_envs, h->cus, h->sw);
    if (!s.fits) return fail(FTL_E_INVALID, "the frame kernel needs more than 64 KiB of LDS per wavefront (static rects x frames per step)");
    h->sched = s; h->co_envs = co_envs; h->dirty = true;
    P.fr_rec_off = s.fr_rec_off; P.fr_rec_stride = s.fr_rec_stride; P.fr_pend_off = s.fr_pend_off; P.fr_env_off = s.fr_env_off;
    P.fr_defer = s.fr_defer; P.fr_lds = s.fr_lds;
    bool expl = false, compas = false;
    for (int k = 0; k < c.n_lasers; k++) { compas = compas || c.lasers[k].compas != 0; expl = expl || c.lasers[k].explicit_angles != 0 || c.lasers[k].pad_sectors != 0; }
    for (int i = 0; i < 2; i++) {
        h->k_frames[i] = frame_kernel(frame_inst(c, s.G, i == 1));
        h->rays[i] = rays_inst(P.hmax, expl || compas, P.corr_lds_cap < c.corr_cap, i == 1, h->one_pass, h->one_pass ? P.pass_rays[P.pass_single] : 0);
        h->k_rays[i] = c.n_lasers > 0 ? rays_kernel(h->rays[i]) : nullptr;
    }
    h->has_aux = c.n_aux > 0 || compas; h->has_trk1 = c.has_tracker == 1;
    return FTL_OK;
}

// The FTL_DEBUG_PRINT_LDS report: what ftl_create, and every ftl_tune that succeeded, left on the handle
void report_plan(const ftl_handle* h) {
    if (!h->sw.print_lds) return;
    const FtlDevParams& P = h->P;
    fprintf(stderr, "ftl: frame kernel LDS %d B per wavefront, %d lanes per env, %d frames at most, searches %s\n", P.fr_lds, h->sched.G, frames_max(P.cfg), P.fr_defer ? "deferred" : "in frame");
    fprintf(stderr, "ftl: ray kernel LDS %d B per env\n", P.lds_rays);
    char r[2][40] = {"no rays", "no rays"};
    for (int i = 0; i < 2; i++)
        if (h->k_rays[i]) snprintf(r[i], sizeof r[i], "rays<%d,%d,%d,%d,%d>", h->rays[i].hm, h->rays[i].expl, h->rays[i].split, h->rays[i].capped, h->rays[i].one_pass);
    fprintf(stderr, "ftl: kernels frames<%d,%d>, %s on one stream, %s on two; regroup %s every %u, two streams %s\n", h->sched.G, frame_inst(P.cfg, h->sched.G, false).reg,
            r[0], r[1], h->sched.regroup ? "on" : "off", h->rg_every, h->split ? "on" : "off");
    // (a continuation line: the three lines above are parsed as they stand)
    if (h->k_rays[0]) fprintf(stderr, "     ray candidates: %s form on one stream, %s form on two, window %d\n", h->rays[0].mask ? "mask" : "list", h->rays[1].mask ? "mask" : "list", P.pair_window);
    // (one more per pass that has rays: the reach phase 1 culls each segment class with, in px)
    if (h->k_rays[0]) for (int which = 0; which < 2; which++) if (P.pass_rays[which] > 0) {
        char r[4][24];
        for (int q = 0; q < 4; q++) {
            if (P.cls_reach[which][q] < 0.0f) snprintf(r[q], sizeof r[q], "none");
            else snprintf(r[q], sizeof r[q], "%g", (double)P.cls_reach[which][q]);
        }
        fprintf(stderr, "     ray cull: pass %d static %s dynamic %s corridor %s green %s\n", which, r[0], r[1], r[2], r[3]);
    }
}

}  // namespace

extern "C" {

const char* ftl_last_error(void) { return g_err.c_str(); }

size_t ftl_sizeof_config(void) { return sizeof(ftl_config); }
size_t ftl_sizeof_scenarios(void) { return sizeof(ftl_scenarios); }
size_t ftl_sizeof_outputs(void) { return sizeof(ftl_outputs); }
size_t ftl_sizeof_scen_params(void) { return sizeof(ftl_scen_params); }
size_t ftl_sizeof_final_outputs(void) { return sizeof(ftl_final_outputs); }

int ftl_create(const ftl_config* cfg, int32_t n_envs, int32_t device, ftl_handle** out) {
    if (!cfg || !out) return fail(FTL_E_INVALID, "null argument");
    if (n_envs <= 0) return fail(FTL_E_INVALID, "n_envs must be positive");
    if (device < 0) return fail(FTL_E_INVALID, "device < 0: this library has no CPU path");
    std::string why;
    if (int rc = validate(*cfg, why)) return fail(rc, why);
    ftl_handle* h = new (std::nothrow) ftl_handle();       // value-initialised: every member, P and its padding included, starts as zero
    if (!h) return fail(FTL_E_DEVICE, "out of host memory");
    h->P.cfg = *cfg;
    // (which pass a sensor belongs to is a flag: the host tables and the kernels compare it with 0 / 1)
    for (int k = 0; k < FTL_MAX_LASERS; k++) h->P.cfg.lasers[k].after_tracker = cfg->lasers[k].after_tracker ? 1 : 0;
    h->device = device; h->dirty = true;
    h->sw = read_switches();
    // two streams: measured +9 % with random_frames_per_step (long frame kernels whose tails the other half's ray kernel fills), -1 % with a
    // fixed 10 frames per step -- so it is on for the former only; FTL_SPLIT=0/1 overrides.  (The v1 tracker kernel covers all envs at once.)
    h->split = n_envs >= 8192 && (h->sw.split >= 0 ? h->sw.split == 1 : cfg->rand_fps_hi > 0) && cfg->has_tracker != 1;
    // the permutation of the cost sort is rebuilt every k-th launch (round 3: every 4th launch, 212 against 209 M env-steps/s at every
    // 2nd -- with the later frames' searches deferred the frame kernel is as fast on a staler order); FTL_REGROUP_EVERY is the tuning knob
    h->rg_every = h->sw.regroup_every > 0 ? (unsigned)h->sw.regroup_every : 4u;
    h->cus = 256;
    (void)hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device);
    FtlDevParams& P = h->P;
    P.n_envs = n_envs;
    P.R = 2 + cfg->n_bears;
    int off = 0, hmax = 1, rays = 0;
    auto width_of = [](const ftl_laser_cfg& l) { return l.count * (l.compas ? 5 : (l.pad_sectors ? 4 : 1)); };
    for (int k = 0; k < cfg->n_lasers; k++) {
        P.cfg.lasers[k].out_offset = off;
        off += cfg->lasers[k].history * width_of(cfg->lasers[k]);
        hmax = cfg->lasers[k].history > hmax ? cfg->lasers[k].history : hmax;
        rays += cfg->lasers[k].count;
    }
    for (int j = 0; j < cfg->n_aux; j++) {       // lidar / detector blocks follow the ray sensors' blocks
        ftl_aux_cfg& a = P.cfg.aux[j];
        a.out_len = a.kind == FTL_AUX_LIDAR ? (a.return_all_points ? 1 + a.n_angles * a.points_number * (a.return_only_distances ? 1 : 2) : a.n_angles * (a.return_only_distances ? 1 : 2))
                  : a.kind == FTL_AUX_TRACK_VECTOR ? 2 * a.seq_len : a.radar_sectors;
        a.out_offset = off; off += a.out_len;
    }
    P.lasers_len = off; P.total_rays = rays; P.hmax = hmax;
    {   // ray directions relative to the heading (glibc cos / sin, as the reference's np.cos(np.radians(.))) and the no-hit reading
        const double deg2rad = 3.141592653589793 / 180.0;
        bool miss_ok = true;
        const double span = (double)(cfg->width > cfg->height ? cfg->width : cfg->height);
        const double margin = 1e-11 * (span > 2048.0 ? span / 2048.0 : 1.0);
        for (int k = 0; k < cfg->n_lasers; k++) {
            const ftl_laser_cfg& l = cfg->lasers[k];
            // float64 |end - origin| = laser_length within 4e-13 (coordinates < 2048): float32(.) is float32(laser_length) unless a
            // rounding boundary of float32 lies that close
            miss_ok = miss_ok && (float)(l.length - margin) == (float)l.length && (float)(l.length + margin) == (float)l.length;
        }
        P.miss_const = miss_ok ? 1 : 0;
        int rb[2] = {0, 0};              // phase 3's per-sensor records; ray indices run over the sensors of one pass (before / after the tracker)
        for (int k = 0; k < cfg->n_lasers; k++) {
            const ftl_laser_cfg& l = cfg->lasers[k];
            FtlRaySensor& rs = P.ray_sens[k];
            const int which = l.after_tracker ? 1 : 0, ro = l.react_obstacles;
            rs.count = l.count; rs.rbase = rb[which];
            rs.reach2 = ((float)l.length + 2.0f) * ((float)l.length + 2.0f);
            rs.inv_step = (float)l.count * 0.15915494309189535f; rs.inv_count = 1.0f / (float)l.count;
            rs.off_u = (float)(l.angle_offset * deg2rad) * rs.inv_step;
            rs.slack = 0.022f + 0.01f * (float)l.count * 0.15915494f;   // 0.01 rad + 0.022 ray spacings (0.002 of them: the arc is scaled per sensor after it was
                                                                        // normalised in radians -- float32 roundings of values below 2 x count)
            rs.flags = ((ro == 1 || ro == 2) ? 1u : 0u) | ((ro == 1 || ro == 3) ? 2u : 0u) | (l.react_corridor ? 4u : 0u) | (l.react_green ? 8u : 0u)
                     | (l.explicit_angles ? 16u : 0u) | (which ? 32u : 0u) | (l.compas ? 64u : 0u);
            if (!l.compas) rb[which] += l.count;
        }
        P.inv_nrect_dyn = (65536u + (unsigned)(P.R - 1) - 1u) / (unsigned)(P.R - 1);
        // per-ray records of phase 2, rays in pass order: the sensors scanned before the tracker, then those scanned after it
        int g = 0;
        for (int which = 0; which < 2; which++) {
            P.pass_base[which] = g; P.pass_lmax[which] = 0.0f;
            for (int k = 0; k < cfg->n_lasers; k++) {
                const ftl_laser_cfg& l = cfg->lasers[k];
                if ((l.after_tracker ? 1 : 0) != which || l.compas) continue;
                P.pass_lmax[which] = fmaxf(P.pass_lmax[which], (float)l.length);
                for (int i = 0; i < l.count && g < FTL_MAX_RAYS; i++, g++) {
                    const double a = l.explicit_angles ? l.ray_angles[i & 7] : l.angle_offset + i * (360.0 / (double)l.count);
                    P.ray_dir[g].c = cos(a * deg2rad); P.ray_dir[g].s = sin(a * deg2rad); P.ray_dir[g].len = l.length;
                }
            }
            P.pass_rays[which] = g - P.pass_base[which];
            // phase 1's cull per segment class: the longest reach among the pass's sensors that react to the class -- the float32 value
            // whose square is rs.reach2 above -- or -1: no sensor of the pass sees the class.
            // FTL_RAYS_CLASS_CULL=0: one box of pass_lmax + 2 for every class (the table before the class cull)
            for (int q = 0; q < 4; q++) {
                float reach = -1.0f;
                for (int k = 0; k < cfg->n_lasers; k++) {
                    const ftl_laser_cfg& l = cfg->lasers[k];
                    if ((l.after_tracker ? 1 : 0) != which || l.compas || !((P.ray_sens[k].flags >> q) & 1u)) continue;
                    reach = fmaxf(reach, (float)l.length + 2.0f);
                }
                P.cls_reach[which][q] = h->sw.class_cull != 0 ? reach : P.pass_lmax[which] + 2.0f;
            }
        }
        // Every shipped config scans all its ray sensors on one side of the tracker: the other pass has nothing to do, and the kernels
        // compiled without the loop over the passes run the one that has.  FTL_RAYS_ONE_PASS=0/1 overrides (1 is the default where it applies).
        P.pass_single = P.pass_rays[0] > 0 && P.pass_rays[1] > 0 ? -1 : (P.pass_rays[1] > 0 ? 1 : 0);
        h->one_pass = P.pass_single >= 0 && h->sw.one_pass != 0;
        // pairs per window of the mask form's candidate list: all of it, or what FTL_DEBUG_PAIR_WINDOW asks for (tests of the multi-window path)
        P.pair_window = FTL_PAIR_CAP;
        if (const int v = h->sw.pair_window; v >= 16 && v <= FTL_PAIR_CAP && v % 16 == 0) P.pair_window = v;
    }
    if (rays > 1023) { delete h; return fail(FTL_E_INVALID, "more than 1023 rays per env (the candidate list of the ray kernel packs a ray index into 10 bits)"); }
    if (hmax * (P.R - 1) > FTL_WAVE) { delete h; return fail(FTL_E_INVALID, "max_prev_obs x (1 + bears) exceeds one wavefront of snapshot rects"); }
    {   // row width / common history of the fused sensorPrev output: the sensors wrappers.py:204, 214 select (in_policy_obs), in dict order
        int w = 0, hcommon = 0;
        for (int k = 0; k < cfg->n_lasers; k++) {
            P.pol_off[k] = -1;
            if (!cfg->lasers[k].in_policy_obs) continue;
            P.pol_off[k] = w; w += width_of(cfg->lasers[k]);
            if (hcommon == 0) hcommon = cfg->lasers[k].history;
            else if (cfg->lasers[k].history != hcommon) hcommon = -1;
        }
        P.pol_width = w; P.pol_h = hcommon;
    }
    // State layout.  The small fields of an env form one record (fields in the order below, the ray kernel's inputs first; 16-byte aligned
    // fields, a stride that is a multiple of 128 bytes); the long ones are [n_envs][per_env] arrays in 256-byte aligned regions.
    const size_t n = (size_t)n_envs;
    size_t per_env[FTL_N_FIELDS];
    per_env[F_rb_pos] = (size_t)P.R * 2; per_env[F_rb_dbl] = (size_t)P.R * FTL_RD_COUNT; per_env[F_rb_int] = (size_t)P.R * FTL_RI_COUNT;
    per_env[F_env_int] = FTL_EI_COUNT; per_env[F_env_dbl] = FTL_ED_COUNT; per_env[F_fol_cs] = 2;
    per_env[F_snap_rects] = (size_t)hmax * (P.R - 1) * 4; per_env[F_snap_win] = (size_t)hmax * 4;
    per_env[F_traj] = (size_t)cfg->traj_cap * 2; per_env[F_traj_bb] = (size_t)(cfg->traj_cap / FTL_TRAJ_BLOCK) * 4;
    per_env[F_hist] = (size_t)cfg->corr_cap * 2; per_env[F_corr] = (size_t)cfg->corr_cap * 4; per_env[F_corr32] = (size_t)cfg->corr_cap * 4;
    per_env[F_hist1] = (size_t)(cfg->has_tracker == 1 ? cfg->hist1_cap : 0) * 2; per_env[F_ep_stats] = FTL_N_METRICS;
    size_t ro = 0;
    for (int i : kRecOrder) {
        ro = align_up(ro, 16);
        h->fields[i] = Field{kFields[i].name, ro, per_env[i], kFields[i].dtype, 0};
        ro += per_env[i] * kFields[i].esz;
    }
    const size_t rec_stride = align_up(ro, 128);
    P.rec_stride = (int32_t)rec_stride;
    for (int i : kRecOrder) h->fields[i].stride = rec_stride;
    size_t cur = rec_stride * n;
    for (int i = 0; i < FTL_N_FIELDS; i++) {
        if (kFields[i].rec) continue;
        cur = align_up(cur, 256);
        h->fields[i] = Field{kFields[i].name, cur, per_env[i], kFields[i].dtype, per_env[i] * kFields[i].esz};
        cur += per_env[i] * kFields[i].esz * n;
    }
    h->state_bytes = align_up(cur, 256);
    {   // corridor ring (f32x4) + near rects (int4 + u32) + corridor refs (u32) + green caps (f32x4 + u32) + counters
        // + ray ends (double2) + per-(ray, snapshot) minima (u64 x HM) + miss readings (f64)
        const size_t rects = (size_t)cfg->n_static + hmax + (size_t)hmax * (P.R - 2 > 0 ? P.R - 2 : 0) + 1;
        // LDS copy of the corridor ring: up to 128 points (the windows of the snapshots span a few dozen; the ring itself is sized
        // for a crawling leader); FTL_DEBUG_CORR_LDS_CAP forces a smaller copy (tests of the unstaged path)
        P.corr_lds_cap = cfg->corr_cap < 128 ? cfg->corr_cap : 128;
        if (const int v = h->sw.corr_lds_cap; v >= 2 && v <= cfg->corr_cap && (v & (v - 1)) == 0) P.corr_lds_cap = v;
        // the float32 minima are sized by the EXPL rows of rays_inst(), which have the widest HM for any hmax (5 or FTL_HMAX accumulators
        // per ray), whichever instantiation the handle launches.  (The occupancy every profile was taken at depends on this size.)
        const int hm_lds = rays_inst(hmax, true, false, false, false, 0).hm;
        P.lds_rays = (int)((size_t)P.corr_lds_cap * 16 + rects * 20 + (size_t)2 * P.corr_lds_cap * 4 + (size_t)2 * hmax * 20 + 64
                           + (size_t)rays * 16 + (size_t)rays * hm_lds * 4 + (size_t)rays * 4
                           + rects * 8 + 32                   /* facing-edge list (u16 x 4 per rect) + edge counters */
                           + (size_t)FTL_PAIR_CAP * 2 + 16);  /* candidate list of phase 3 */
    }
    // The v2 tracker trims its window from a running length while that length stays exact in float64: the kernel drops it for a window
    // that reaches 2^10 px (no config bounds the longest segment: a seeded step is as long as the field allows), which a window trimmed to
    // a corridor_length of 2^10 or more always does.  FTL_TRK_RUNNING=0: the two full sums of every saving scan, no length kept.
    P.trk_running = (h->sw.trk_running != 0 && cfg->has_tracker == 2 && cfg->corridor_length > 0.0 && cfg->corridor_length < 1024.0) ? 1 : 0;
    P._pad_trk = 0;
    P.trk_band = h->sw.trk_band;
    P.lds_rays += h->sw.lds_pad_rays;      // diagnostic: occupancy of the ray kernel without touching the code
    if (cfg->traj_cap > 65535 || frames_max(*cfg) > 4095) { delete h; return fail(FTL_E_INVALID, "traj_cap above 65535 or more than 4095 frames per step"); }
    if (apply_plan(h, n_envs)) { delete h; return FTL_E_INVALID; }
    report_plan(h);
    if (P.lds_rays > 64 * 1024) { delete h; return fail(FTL_E_INVALID, "config needs more than 64 KiB of LDS per env"); }
    if (ftl_aux_lds_bytes(*cfg) > 64 * 1024) { delete h; return fail(FTL_E_INVALID, "the compas / lidar / radar sensors of this config need more than 64 KiB of LDS per env"); }
    *out = h;
    return FTL_OK;
}

void ftl_destroy(ftl_handle* h) {
    if (!h) return;
    if (h->dP || h->rg_mem || h->side || h->mt_mem || h->rs.scen_idx || h->ro_alive || h->bl_action) (void)hipSetDevice(h->device);
    if (h->rs.scen_idx) (void)hipFree(h->rs.scen_idx);
    if (h->ro_alive) (void)hipFree(h->ro_alive);
    if (h->bl_action) (void)hipFree(h->bl_action);
    if (h->dP) (void)hipFree(h->dP);
    if (h->mt_mem) (void)hipFree(h->mt_mem);
    for (hipEvent_t ev : h->tev) (void)hipEventDestroy(ev);
    if (h->rg_mem) (void)hipFree(h->rg_mem);
    if (h->side) { (void)hipStreamSynchronize(h->side); (void)hipStreamDestroy(h->side); }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    delete h;
}

int32_t ftl_lasers_len(const ftl_handle* h) { return h ? h->P.lasers_len : 0; }

int ftl_get_config(const ftl_handle* h, ftl_config* out) {
    if (!h || !out) return fail(FTL_E_INVALID, "null argument");
    *out = h->P.cfg;
    return FTL_OK;
}

size_t ftl_state_bytes(const ftl_handle* h) { return h ? h->state_bytes : 0; }

int ftl_state_field(const ftl_handle* h, const char* name, size_t* offset, size_t* per_env, int32_t* dtype, size_t* stride) {
    if (!h || !name) return fail(FTL_E_INVALID, "null argument");
    for (int i = 0; i < FTL_N_FIELDS; i++)
        if (!strcmp(h->fields[i].name, name)) {
            if (offset) *offset = h->fields[i].offset;
            if (per_env) *per_env = h->fields[i].per_env;
            if (dtype) *dtype = h->fields[i].dtype;
            if (stride) *stride = h->fields[i].stride;
            return FTL_OK;
        }
    return fail(FTL_E_INVALID, std::string("unknown state field ") + name);
}

int ftl_bind_state(ftl_handle* h, void* dev_state, size_t bytes) {
    if (!h || !dev_state) return fail(FTL_E_INVALID, "null argument");
    if (bytes < h->state_bytes) return fail(FTL_E_INVALID, "state buffer too small");
    if (((uintptr_t)dev_state) & 255) return fail(FTL_E_INVALID, "state buffer must be 256-byte aligned");
    for (int i = 0; i < FTL_N_FIELDS; i++) *(void**)((char*)&h->P + kFields[i].ptr) = (unsigned char*)dev_state + h->fields[i].offset;
    h->bound = true; h->dirty = true;
    return FTL_OK;
}

int ftl_load_scenarios(ftl_handle* h, const ftl_scenarios* pool) {
    if (!h || !pool) return fail(FTL_E_INVALID, "null argument");
    if (pool->n_scenarios <= 0) return fail(FTL_E_INVALID, "empty scenario pool");
    if (!pool->robot_pos || !pool->robot_dir || !pool->robot_rect || !pool->route || !pool->route_len ||
        !pool->init_traj || !pool->init_traj_len || (h->P.cfg.n_static > 0 && !pool->static_rects))
        return fail(FTL_E_INVALID, "scenario pool has null arrays");
    h->P.scen = *pool;
    h->have_scen = true; h->dirty = true;
    h->win_base = 0; h->win_count = pool->n_scenarios; h->win_stride = h->P.n_envs % pool->n_scenarios;
    return FTL_OK;
}

int ftl_set_reset_window(ftl_handle* h, int32_t base, int32_t count, int32_t stride) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (!h->have_scen) return fail(FTL_E_STATE, "ftl_load_scenarios has not been called");
    if (base < 0 || count <= 0 || base + count > h->P.scen.n_scenarios) return fail(FTL_E_INVALID, "reset window outside the scenario pool");
    h->win_base = base; h->win_count = count; h->win_stride = (stride > 0 ? stride : h->P.n_envs) % count;
    return FTL_OK;
}

int ftl_tune(ftl_handle* h, int32_t what, int32_t value) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (what == FTL_TUNE_COSCHEDULED_ENVS) {
        if (value < h->P.n_envs) return fail(FTL_E_INVALID, "co-scheduled envs below this handle's own");
        if (int rc = apply_plan(h, value)) return rc;
    } else if (what == FTL_TUNE_REGROUP_EVERY) {
        if (value < 1) return fail(FTL_E_INVALID, "regroup interval below 1");
        if (h->sw.regroup_every <= 0) h->rg_every = (unsigned)value;
    } else if (what == FTL_TUNE_TWO_STREAMS) {
        if (h->sw.split < 0) h->split = value != 0 && h->P.n_envs >= 8192 && h->P.cfg.has_tracker != 1;
    } else return fail(FTL_E_INVALID, "unknown tuning key");
    report_plan(h);
    return FTL_OK;
}

// device copy of the frozen parameters: (re)uploaded only after bind_state / load_scenarios, never on the steady-state step path
static int sync_params(ftl_handle* h) {
    hipError_t e;
    if (!h->dP) {
        e = hipMalloc((void**)&h->dP, sizeof(FtlDevParams));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(params): ") + hipGetErrorString(e));
        h->dirty = true;
    }
    if (h->dirty) {
        e = hipMemcpy(h->dP, &h->P, sizeof(FtlDevParams), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMemcpy(params): ") + hipGetErrorString(e));
        h->dirty = false;
    }
    return FTL_OK;
}

// The kernels of one pass (a step, a reset, a reset pass) on `stream`.  FTL_STEP_NO_SENSORS in call_in.flags leaves out the two sensor
// launches and nothing else; the kernels never see the bit.
static int launch(ftl_handle* h, const FtlCall& call_in, void* stream) {
    const bool sensors = !(call_in.flags & FTL_STEP_NO_SENSORS);
    FtlCall call = call_in; call.flags &= ~(uint32_t)FTL_STEP_NO_SENSORS;
    if (int rc = set_device(h)) return rc;
    if (h->sched.regroup && !h->rg_mem) {
        const size_t n = (size_t)h->P.n_envs, nb = (n + FTL_RG_BLOCK - 1) / FTL_RG_BLOCK;
        const size_t o_bh = align_up(n * 4, 256), o_rank = o_bh + align_up(nb * FTL_NKEYS * 4, 256), o_keys = o_rank + align_up(n * 2, 256), o_tot = o_keys + align_up(n, 256);
        hipError_t e = hipMalloc(&h->rg_mem, o_tot + 2 * FTL_NKEYS * sizeof(int));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(regroup): ") + hipGetErrorString(e));
        char* b = (char*)h->rg_mem;
        h->P.perm = (int32_t*)b; h->P.bh = (int32_t*)(b + o_bh); h->P.rank = (uint16_t*)(b + o_rank); h->P.keys = (uint8_t*)(b + o_keys);
        h->rg_tot = (int*)(b + o_tot); h->rg_parity = 0;
        e = hipMemsetAsync(h->rg_tot, 0, 2 * FTL_NKEYS * sizeof(int), (hipStream_t)stream);
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMemsetAsync(regroup): ") + hipGetErrorString(e));
        hipLaunchKernelGGL(ftl::ftl_perm_identity_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->P.perm, (int)n);
        h->dirty = true;
    }
    { int rc = sync_params(h); if (rc) return rc; }
    if (h->split && !h->side) {
        if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess)
            return fail(FTL_E_DEVICE, "cannot create the side stream / events");
    }
    // one slot range: frame loop (G lanes per env: 4 for <= 2 dynamic obstacles, else 8; configs with leader regimes or random
    // frame counts use the instantiations that carry that code), then the ray sensors of the same envs
    // (the halves are interleaved wavefront by wavefront, so both see the same mix of the cost-sorted slots)
    // optional per-kernel timing (ftl_kernel_timing): up to 512 steps of 4 events each, single-stream mode only
    hipEvent_t* tev = nullptr;
    if (h->timing && !h->split && call.mode == 0 && h->tev_used + 5 <= 5 * 512) {
        while (h->tev.size() < h->tev_used + 5) { hipEvent_t ev; if (hipEventCreate(&ev) != hipSuccess) return fail(FTL_E_DEVICE, "hipEventCreate"); h->tev.push_back(ev); }
        tev = h->tev.data() + h->tev_used; h->tev_used += 5;
    }
    const FtlKernel frames = h->k_frames[call_xr(call) ? 1 : 0];
    auto launch_range = [&](int part, int parts, hipStream_t s) {
        const int epw = h->sched.epw;
        const int n_groups = (h->P.n_envs + epw - 1) / epw;
        const int my_groups = (n_groups - part + parts - 1) / parts;
        FtlCall c2 = call; c2.part = part; c2.parts = parts; c2.epw = epw;
        if (tev) (void)hipEventRecord(tev[0], s);
        hipLaunchKernelGGL(frames, dim3(my_groups), dim3(FTL_WAVE), (size_t)h->P.fr_lds + h->sw.lds_pad, s, h->dP, c2);
        if (h->has_trk1 && part == 0)      // the v1 tracker's scan + snapshot bookkeeping for ALL envs (one thread per env)
            hipLaunchKernelGGL(ftl::ftl_tracker1_kernel, dim3((unsigned)((h->P.n_envs + 255) / 256)), dim3(256), 0, s, h->dP, c2);
        if (tev) (void)hipEventRecord(tev[1], s);
        // one block per slot of this launch (the tail of the last group may be idle)
        if (const FtlKernel rays = sensors ? h->k_rays[parts > 1 ? 1 : 0] : nullptr) hipLaunchKernelGGL(rays, dim3(my_groups * epw), dim3(FTL_WAVE), h->P.lds_rays, s, h->dP, c2);
        if (tev) (void)hipEventRecord(tev[2], s);
    };
    if (h->split) {
        (void)hipEventRecord(h->ev_fork, (hipStream_t)stream);              // everything the caller queued (actions, ...) happens first
        (void)hipStreamWaitEvent(h->side, h->ev_fork, 0);
        launch_range(0, 2, (hipStream_t)stream);
        launch_range(1, 2, h->side);
        (void)hipEventRecord(h->ev_join, h->side);
        (void)hipStreamWaitEvent((hipStream_t)stream, h->ev_join, 0);        // the caller's stream sees the whole step
    } else launch_range(0, 1, (hipStream_t)stream);
    // compas / lidar / leader-track detectors: one more launch, only for configs that have such a sensor
    if (h->has_aux && sensors) hipLaunchKernelGGL(ftl_aux_kernel, dim3((unsigned)h->P.n_envs), dim3(FTL_WAVE), ftl_aux_lds_bytes(h->P.cfg), (hipStream_t)stream, h->dP, call);
    if (tev) (void)hipEventRecord(tev[3], (hipStream_t)stream);
    // the frame kernel left every env's cost class for its next step: rebuild the slot -> env map.  The classes are stable
    // from step to step unless the frame count is random, so every second launch is enough then.  (The reset pass of ftl_step_final
    // follows a step that has just rebuilt or kept the map: the few envs it re-initialises move with the next rebuild.)
    if (h->sched.regroup && !(call.flags & FTL_CALL_FINISH) && (h->P.cfg.rand_fps_hi > 0 || call.mode == 1 || (h->rg_launches++ % h->rg_every) == 0)) {
        const unsigned nb = (unsigned)((h->P.n_envs + FTL_RG_BLOCK - 1) / FTL_RG_BLOCK);
        int* tot = h->rg_tot + (h->rg_parity & 1u) * FTL_NKEYS, *tot_next = h->rg_tot + ((h->rg_parity + 1u) & 1u) * FTL_NKEYS;
        h->rg_parity++;
        hipLaunchKernelGGL(ftl::ftl_regroup_count_kernel, dim3(nb), dim3(FTL_RG_BLOCK), 0, (hipStream_t)stream, h->dP, tot);
        hipLaunchKernelGGL(ftl::ftl_regroup_scatter_kernel, dim3(nb), dim3(FTL_RG_BLOCK), 0, (hipStream_t)stream, h->dP, (const int*)tot, tot_next);
    }
    if (tev) (void)hipEventRecord(tev[4], (hipStream_t)stream);
    return launched();
}

}  // extern "C"

// What a reset or a step needs before anything is launched: a bound state, a scenario pool, the output arrays and, with policy_obs, one
// history length on every ray sensor
// the arguments of a call that restarts nothing and asks for no masks
static FtlCall make_call(const ftl_handle* h, int mode, const ftl_outputs* out) {
    FtlCall c = {};
    c.mode = mode; c.out = *out; c.action_kind = FTL_ACTION_BOX2; c.win_base = h->win_base; c.win_count = h->win_count; c.win_stride = h->win_stride;
    return c;
}

static int check_ready(const ftl_handle* h, const ftl_outputs* out, bool policy_obs = true) {
    if (!h->bound) return fail(FTL_E_STATE, "ftl_bind_state has not been called");
    if (!h->have_scen) return fail(FTL_E_STATE, "ftl_load_scenarios has not been called");
    if (!out || !out->obs_num || !out->target || !out->reward || !out->done || !out->status || (h->P.lasers_len > 0 && !out->lasers))
        return fail(FTL_E_INVALID, "output arrays missing");
    if (policy_obs && out->policy_obs && h->P.pol_h <= 0) return fail(FTL_E_INVALID, "policy_obs needs the same max_prev_obs on every ray sensor");
    return FTL_OK;
}

#include "ftl_restart.hpp"       // what same-step, the queue and the sampler share: finish_step, start_chosen, the choosers' arguments
#include "ftl_queue.hpp"         // the episode queue (ftl_set_episode_queue, ftl_queue_start, FTL_STEP_QUEUE_RESET), same translation unit
#include "ftl_sampler.hpp"       // the scenario sampler (ftl_set_scenario_sampler, ftl_sampler_start, FTL_STEP_SAMPLE_RESET), same translation unit

extern "C" {

int ftl_reset(ftl_handle* h, const int32_t* scen_idx, const uint8_t* mask, const ftl_outputs* out, void* stream) {
    if (!h || !scen_idx) return fail(FTL_E_INVALID, "null argument");
    int rc = check_ready(h, out);
    if (rc) return rc;
    FtlCall call = make_call(h, 1, out);
    call.scen_idx = scen_idx; call.mask = mask;
    h->last_lasers = h->P.lasers_len > 0 ? out->lasers : nullptr;
    return launch(h, call, stream);
}

int ftl_step(ftl_handle* h, const double* action, const ftl_outputs* out, uint32_t flags, void* stream) {
    return ftl_step_encoded(h, action, FTL_ACTION_BOX2, out, flags, stream);
}

int ftl_step_encoded(ftl_handle* h, const void* action, int32_t encoding, const ftl_outputs* out, uint32_t flags, void* stream) {
    return ftl_step_final(h, action, encoding, out, nullptr, flags, stream);
}

int ftl_step_final(ftl_handle* h, const void* action, int32_t encoding, const ftl_outputs* out, const ftl_final_outputs* fin,
                   uint32_t flags, void* stream) {
    if (!h || !action) return fail(FTL_E_INVALID, "null argument");
    const uint32_t blind = flags & FTL_STEP_NO_SENSORS;     // every pass of this call goes without the sensor kernels (launch())
    flags &= FTL_STEP_AUTO_RESET | FTL_STEP_NEXT_RESET | FTL_STEP_QUEUE_RESET | FTL_STEP_SAMPLE_RESET;   // the reset bits (other bits were always ignored; the kernel's internal ones stay internal)
    if ((flags & FTL_STEP_AUTO_RESET) && (flags & FTL_STEP_NEXT_RESET)) return fail(FTL_E_INVALID, "FTL_STEP_AUTO_RESET and FTL_STEP_NEXT_RESET exclude each other");
    const bool queue = (flags & FTL_STEP_QUEUE_RESET) != 0;
    if (queue && flags != FTL_STEP_QUEUE_RESET) return fail(FTL_E_INVALID, "FTL_STEP_QUEUE_RESET excludes the other reset flags");
    const bool sample = (flags & FTL_STEP_SAMPLE_RESET) != 0;
    if (sample && flags != FTL_STEP_SAMPLE_RESET) return fail(FTL_E_INVALID, "FTL_STEP_SAMPLE_RESET excludes the other reset flags");
    if (encoding < FTL_ACTION_BOX2 || encoding > FTL_ACTION_TURN) return fail(FTL_E_INVALID, "unknown action encoding");
    if (sample && !h->sampler.attached) return fail(FTL_E_STATE, "FTL_STEP_SAMPLE_RESET without a scenario sampler (ftl_set_scenario_sampler)");
    if (queue && !h->queue.attached) return fail(FTL_E_STATE, "FTL_STEP_QUEUE_RESET without an episode queue (ftl_set_episode_queue)");
    int rc = check_ready(h, out);
    if (rc) return rc;
    const bool same_step = fin && (flags & (FTL_STEP_AUTO_RESET | FTL_STEP_QUEUE_RESET | FTL_STEP_SAMPLE_RESET));      // the terminal rows are copied
    if (fin && (!fin->ended || !fin->restarted)) return fail(FTL_E_INVALID, "ftl_final_outputs: ended / restarted missing");
    if (same_step && (!fin->obs_num || !fin->target || (h->P.lasers_len > 0 && !fin->lasers)))
        return fail(FTL_E_INVALID, "ftl_final_outputs: obs_num / lasers / target missing (needed under FTL_STEP_AUTO_RESET / FTL_STEP_QUEUE_RESET / FTL_STEP_SAMPLE_RESET)");
    if (same_step && fin->policy_obs && !out->policy_obs) return fail(FTL_E_INVALID, "ftl_final_outputs.policy_obs needs ftl_outputs.policy_obs");
    FtlCall call = make_call(h, 0, out);
    call.action = (const double*)action; call.action_kind = encoding; call.flags = flags | blind;
    if (fin) { call.ended = fin->ended; call.restarted = fin->restarted; }
    h->last_lasers = h->P.lasers_len > 0 ? out->lasers : nullptr;
    if (queue || sample) {   // a plain step, then the chooser's kernel and the reset pass of the slots it restarts (ftl_restart.hpp)
        if (sample) { rc = ftl_sampler_check_window(h); if (rc) return rc; }
        call.flags = blind; call.ended = nullptr; call.restarted = nullptr;
        rc = launch(h, call, stream);
        if (rc) return rc;
        ftlrs::Args a;
        rc = (queue ? ftl_queue_choose : ftl_sampler_choose)(h, out, fin, ftlrs::MODE_STEP, stream, a);
        return rc ? rc : finish_step(h, call, out, fin, a.scen_idx, a.restarted, stream);
    }
    if (!same_step) return launch(h, call, stream);
    // same-step: the step defers the reset of the envs that finish (their terminal state gets the usual sensor scans), their terminal rows
    // go to `fin`, then a reset pass over fin->ended re-initialises them as the in-kernel auto-reset would have -- all on `stream`, after
    // the step's join when the handle runs two streams
    call.flags = (flags & ~(uint32_t)FTL_STEP_AUTO_RESET) | FTL_CALL_DEFER_RESET | blind;
    rc = launch(h, call, stream);
    return rc ? rc : finish_step(h, call, out, fin, nullptr, fin->ended, stream);
}

int ftl_scan(ftl_handle* h, const ftl_outputs* out, void* stream) {
    if (!h || !out) return fail(FTL_E_INVALID, "null argument");
    if (int rc = check_ready(h, out)) return rc;
    if (int rc = set_device(h)) return rc;
    if (int rc = sync_params(h)) return rc;
    h->last_lasers = h->P.lasers_len > 0 ? out->lasers : nullptr;
    // the sensor launches of a step (mode 0, no flags) with the kernels a step of this handle runs; a two-stream handle's two halves go
    // one after the other on the caller's stream (every env is scanned once either way)
    FtlCall call = make_call(h, 0, out);
    const int parts = h->split ? 2 : 1, epw = h->sched.epw, n_groups = (h->P.n_envs + epw - 1) / epw;
    if (const FtlKernel rays = h->k_rays[parts > 1 ? 1 : 0])
        for (int part = 0; part < parts; part++) {
            const int my_groups = (n_groups - part + parts - 1) / parts;
            call.part = part; call.parts = parts; call.epw = epw;
            if (my_groups > 0) hipLaunchKernelGGL(rays, dim3(my_groups * epw), dim3(FTL_WAVE), h->P.lds_rays, (hipStream_t)stream, h->dP, call);
        }
    call.part = call.parts = call.epw = 0;      // (as launch() hands the call to the aux kernel)
    if (h->has_aux) hipLaunchKernelGGL(ftl_aux_kernel, dim3((unsigned)h->P.n_envs), dim3(FTL_WAVE), ftl_aux_lds_bytes(h->P.cfg), (hipStream_t)stream, h->dP, call);
    return launched();
}

int ftl_kernel_timing(ftl_handle* h, int32_t enable) {
    if (!h) return fail(FTL_E_INVALID, "null argument");
    if (enable && h->split) return fail(FTL_E_UNSUPPORTED, "per-kernel timing is not available in the two-stream mode");
    h->timing = enable != 0; h->tev_used = 0;
    return FTL_OK;
}

int ftl_kernel_times(ftl_handle* h, double* ms, int32_t* n_steps) {
    if (!h || !ms || !n_steps) return fail(FTL_E_INVALID, "null argument");
    if (h->split) return fail(FTL_E_UNSUPPORTED, "per-kernel timing is not available in the two-stream mode");
    ms[0] = ms[1] = ms[2] = ms[3] = 0.0; *n_steps = 0;
    if (h->tev_used == 0) return FTL_OK;
    (void)hipSetDevice(h->device);
    hipError_t e = hipEventSynchronize(h->tev[h->tev_used - 1]);
    if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
    for (size_t i = 0; i + 5 <= h->tev_used; i += 5) {
        for (int k = 0; k < 4; k++) {
            float t = 0.0f;
            e = hipEventElapsedTime(&t, h->tev[i + k], h->tev[i + k + 1]);
            if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipEventElapsedTime: ") + hipGetErrorString(e));
            ms[k] += (double)t;
        }
        *n_steps += 1;
    }
    h->tev_used = 0;
    return FTL_OK;
}

int ftl_episode_metrics(ftl_handle* h, double* dev_metrics, int32_t* dev_errors, uint32_t flags, void* stream) {
    if (!h || !dev_metrics) return fail(FTL_E_INVALID, "null argument");
    if (!h->bound) return fail(FTL_E_STATE, "ftl_bind_state has not been called");
    if (int rc = set_device(h)) return rc;
    const int nb = (h->P.n_envs + FTL_MT_BLOCK - 1) / FTL_MT_BLOCK;
    const size_t o_err = align_up((size_t)nb * FTL_N_METRICS * sizeof(double), 256);
    if (!h->mt_mem) {
        hipError_t e = hipMalloc(&h->mt_mem, o_err + (size_t)nb * 2 * sizeof(int));
        if (e != hipSuccess) return fail(FTL_E_DEVICE, std::string("hipMalloc(metrics): ") + hipGetErrorString(e));
    }
    { int rc = sync_params(h); if (rc) return rc; }
    double* part = (double*)h->mt_mem; int* epart = (int*)((char*)h->mt_mem + o_err);
    hipLaunchKernelGGL(ftl::ftl_metrics_partial_kernel, dim3((unsigned)nb), dim3(FTL_MT_THREADS), 0, (hipStream_t)stream, h->dP, part, epart, (flags & FTL_METRICS_CLEAR) ? 1 : 0);
    hipLaunchKernelGGL(ftl::ftl_metrics_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)part, (const int*)epart, nb, dev_metrics, dev_errors);
    return launched();
}

}  // extern "C"

#include "ftl_gazebo.hpp"      // follower-relative tracker / ray sensors (include/ftl_gazebo.h), same translation unit
#include "ftl_scenario_dev.hpp"  // the scenario generator on the GPU (ftl_generate_scenarios_device), same translation unit
#include "ftl_render.hpp"        // batched top-down RGB frames (ftl_render), same translation unit
#include "ftl_snapshot.hpp"      // snapshot / clone / restore of env rows (ftl_pack_envs, ftl_unpack_envs), same translation unit
#include "ftl_rollout.hpp"       // T blind steps of an action sequence and their discounted return (ftl_rollout), same translation unit
#include "ftl_baseline.hpp"      // the reference's way-point chase as a policy and as closed-loop rollouts (ftl_baseline_act, ftl_rollout_baseline), same translation unit
#include "ftl_mlp.hpp"           // a dense feed-forward policy population on policy_obs: the forward pass and closed-loop rollouts (ftl_mlp_act, ftl_rollout_mlp), same translation unit
#include "ftl_collect.hpp"       // T recorded stochastic closed-loop steps through episode boundaries and their advantages (ftl_collect_mlp, ftl_gae), same translation unit
#include "ftl_rnn.hpp"           // a recurrent policy population (dense trunk, LSTM cell, linear head): decisions, rollouts, trajectories (ftl_rnn_act, ftl_rollout_rnn, ftl_collect_rnn), same translation unit
#include "ftl_ppo.hpp"           // the PPO loss head on recorded rows: dhead, dvalue, d log_std and statistics per weight set (ftl_ppo_head), same translation unit
#include "ftl_search.hpp"        // K candidate action sequences per env on clones in a second handle (ftl_search), same translation unit
#include "ftl_guided.hpp"        // the search over residuals on the baseline follower with a closed-loop tail (ftl_search_guided), same translation unit

#ifdef FTL_WAVE_TIMES
extern "C" int ftl_debug_wave_timeline(unsigned long long* times, unsigned int* info) {
    hipDeviceSynchronize();
    return hipMemcpyFromSymbol(times, HIP_SYMBOL(ftl::g_wt), sizeof(unsigned long long) * 2 * 8192) != hipSuccess ||
           hipMemcpyFromSymbol(info, HIP_SYMBOL(ftl::g_wi), sizeof(unsigned int) * 8192) != hipSuccess;
}
#endif
#ifdef FTL_PROFILE_PATHS
extern "C" int ftl_debug_heavy(unsigned long long* out, int clear) {      // [17] section cycles of the long wavefronts + their number
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ftl::g_cyc_heavy), sizeof(unsigned long long) * 17) != hipSuccess) return 1;
    if (clear) { unsigned long long z[17] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(ftl::g_cyc_heavy), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
extern "C" int ftl_debug_wave_times(unsigned long long* out) {
    hipDeviceSynchronize();
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ftl::g_wave_t), sizeof(unsigned long long) * 2 * 8192) != hipSuccess;
}
extern "C" int ftl_debug_whist(unsigned int* out, int clear) {
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ftl::g_whist), sizeof(unsigned int) * 128) != hipSuccess) return 1;
    if (clear) { unsigned int z[128] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(ftl::g_whist), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
extern "C" int ftl_debug_prof(unsigned long long* out, int clear) {
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ftl::g_prof), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out + 16, HIP_SYMBOL(ftl::g_cyc), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
#ifdef FTL_PROFILE_RAYS
    if (hipMemcpyFromSymbol(out + 32, HIP_SYMBOL(g_rcyc), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
    if (clear) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_rcyc), z, sizeof(z)) != hipSuccess) return 1; }
#endif
    if (clear) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(ftl::g_prof), z, sizeof(z)) != hipSuccess) return 1;
                 if (hipMemcpyToSymbol(HIP_SYMBOL(ftl::g_cyc), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
#endif
