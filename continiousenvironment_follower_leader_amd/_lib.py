"""Build + load the HIP shared library (``libftl_hip.so``) that implements ``include/ftl.h``.

The product has no CPU fallback: if the library is missing or cannot be loaded, importing the
batched env raises."""
import ctypes as C
import os
import subprocess

from . import abi

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
SO_PATH = os.path.join(_PKG, "libftl_hip.so")
SOURCES = [os.path.join(_PKG, "csrc", "ftl_abi.hip"), os.path.join(_PKG, "csrc", "ftl_device.hpp"),
           os.path.join(_PKG, "csrc", "ftl_raymask.hpp"),
           os.path.join(_PKG, "csrc", "ftl_frames_group.hpp"), os.path.join(_PKG, "csrc", "ftl_aux.hpp"), os.path.join(_PKG, "csrc", "ftl_gazebo.hpp"), os.path.join(_ROOT, "include", "ftl_gazebo.h"), os.path.join(_PKG, "csrc", "ftl_scenario.cpp"),
           os.path.join(_PKG, "csrc", "ftl_scenario_dev.hpp"),
           os.path.join(_PKG, "csrc", "ftl_scenario_core.hpp"),
           os.path.join(_PKG, "csrc", "ftl_crmath.hpp"),
           os.path.join(_PKG, "csrc", "ftl_trktrim.hpp"),
           os.path.join(_PKG, "csrc", "ftl_render.hpp"),
           os.path.join(_PKG, "csrc", "ftl_snapshot.hpp"),
           os.path.join(_PKG, "csrc", "ftl_restart.hpp"),
           os.path.join(_PKG, "csrc", "ftl_queue.hpp"),
           os.path.join(_PKG, "csrc", "ftl_sampler.hpp"),
           os.path.join(_PKG, "csrc", "ftl_rollout.hpp"),
           os.path.join(_PKG, "csrc", "ftl_baseline.hpp"),
           os.path.join(_PKG, "csrc", "ftl_mlp.hpp"),
           os.path.join(_PKG, "csrc", "ftl_collect.hpp"),
           os.path.join(_PKG, "csrc", "ftl_rnn.hpp"),
           os.path.join(_PKG, "csrc", "ftl_rnn_math.hpp"),
           os.path.join(_PKG, "csrc", "ftl_ppo.hpp"),
           os.path.join(_PKG, "csrc", "ftl_ppo_math.hpp"),
           os.path.join(_PKG, "csrc", "ftl_search.hpp"),
           os.path.join(_PKG, "csrc", "ftl_guided.hpp"),
           os.path.join(_ROOT, "include", "ftl.h")]
# translation units: the device code + C-ABI, and the host-only scenario generator (reset-time, no GPU code)
UNITS = [os.path.join(_PKG, "csrc", "ftl_abi.hip"), os.path.join(_PKG, "csrc", "ftl_scenario.cpp")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -ffp-contract=off: the arithmetic must follow the reference operation by operation (no implicit FMA)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17"]

_LIB = None


def build(force=False, verbose=False):
    """Compile the HIP library in-tree for gfx950 (works without a GPU: hipcc cross-compiles)."""
    stale = (not os.path.exists(SO_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(SO_PATH) for s in SOURCES)
    if force or stale:
        cmd = [HIPCC] + HIPCC_FLAGS + ["-pthread", "-o", SO_PATH] + UNITS
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, cwd=os.path.join(_PKG, "csrc"))
    return SO_PATH


class FtlError(RuntimeError):
    pass


def load():
    """dlopen the library and declare every entry point of include/ftl.h."""
    global _LIB
    if _LIB is not None:
        return _LIB
    so_path = os.environ.get("FTL_LIB", SO_PATH)     # A/B builds of the same sources (tuning only)
    if not os.path.exists(so_path):
        raise FtlError("libftl_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                       "there is no CPU fallback")
    # PyTorch-ROCm bundles its own HIP runtime; it must be the one already loaded when our library is opened so
    # that both resolve to the SAME libamdhip64 (two runtimes in one process do not see the device).
    import torch  # noqa: F401
    lib = C.CDLL(so_path)
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    lib.ftl_last_error.restype = C.c_char_p
    lib.ftl_create.argtypes = [C.POINTER(abi.Config), i32, i32, C.POINTER(vp)]
    lib.ftl_create.restype = C.c_int
    lib.ftl_destroy.argtypes = [vp]
    lib.ftl_destroy.restype = None
    lib.ftl_lasers_len.argtypes = [vp]
    lib.ftl_lasers_len.restype = i32
    lib.ftl_get_config.argtypes = [vp, C.POINTER(abi.Config)]
    lib.ftl_state_bytes.argtypes = [vp]
    lib.ftl_state_bytes.restype = C.c_size_t
    lib.ftl_bind_state.argtypes = [vp, vp, C.c_size_t]
    lib.ftl_state_field.argtypes = [vp, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(i32), C.POINTER(C.c_size_t)]
    lib.ftl_load_scenarios.argtypes = [vp, C.POINTER(abi.Scenarios)]
    lib.ftl_set_reset_window.argtypes = [vp, i32, i32, i32]
    lib.ftl_tune.argtypes = [vp, i32, i32]
    lib.ftl_reset.argtypes = [vp, vp, vp, C.POINTER(abi.Outputs), vp]
    lib.ftl_step.argtypes = [vp, vp, C.POINTER(abi.Outputs), u32, vp]
    lib.ftl_step_encoded.argtypes = [vp, vp, i32, C.POINTER(abi.Outputs), u32, vp]
    lib.ftl_step_final.argtypes = [vp, vp, i32, C.POINTER(abi.Outputs), C.POINTER(abi.FinalOutputs), u32, vp]
    lib.ftl_scan.argtypes = [vp, C.POINTER(abi.Outputs), vp]
    lib.ftl_scan.restype = C.c_int
    lib.ftl_sizeof_rollout_outputs.restype = C.c_size_t
    lib.ftl_rollout.argtypes = [vp, vp, C.c_int64, i32, i32, C.c_double, C.POINTER(abi.Outputs), C.POINTER(abi.RolloutOutputs), u32, vp]
    lib.ftl_rollout.restype = C.c_int
    lib.ftl_baseline_bytes.argtypes = [vp, i32]
    lib.ftl_baseline_bytes.restype = C.c_size_t
    lib.ftl_baseline_act.argtypes = [vp, C.POINTER(abi.Outputs), vp, C.c_size_t, i32, vp, vp]
    lib.ftl_baseline_act.restype = C.c_int
    lib.ftl_rollout_baseline.argtypes = [vp, i32, C.c_double, C.POINTER(abi.Outputs), C.POINTER(abi.RolloutOutputs), vp, C.c_size_t, i32,
                                         vp, C.c_int64, u32, vp]
    lib.ftl_rollout_baseline.restype = C.c_int
    lib.ftl_kernel_timing.argtypes = [vp, i32]
    lib.ftl_kernel_times.argtypes = [vp, C.POINTER(C.c_double * 4), C.POINTER(i32)]
    lib.ftl_episode_metrics.argtypes = [vp, vp, vp, u32, vp]
    lib.ftl_episode_metrics.restype = C.c_int
    lib.ftl_generate_scenarios.argtypes = [C.POINTER(abi.Config), C.POINTER(abi.ScenParams), vp, i32, i32,
                                           C.POINTER(abi.Scenarios), vp]
    lib.ftl_generate_scenarios.restype = C.c_int
    lib.ftl_sizeof_scen_params.restype = C.c_size_t
    lib.ftl_generate_scenarios_device_workspace.argtypes = [C.POINTER(abi.Config), C.POINTER(abi.ScenParams), i32, C.POINTER(C.c_size_t)]
    lib.ftl_generate_scenarios_device_workspace.restype = C.c_int
    lib.ftl_generate_scenarios_device.argtypes = [C.POINTER(abi.Config), C.POINTER(abi.ScenParams), vp, i32, C.POINTER(abi.Scenarios), vp,
                                                  vp, C.c_size_t, vp]
    lib.ftl_generate_scenarios_device.restype = C.c_int
    lib.ftl_sizeof_render_params.restype = C.c_size_t
    lib.ftl_render_workspace.argtypes = [vp, i32, C.POINTER(C.c_size_t)]
    lib.ftl_render_workspace.restype = C.c_int
    lib.ftl_render.argtypes = [vp, vp, i32, C.POINTER(abi.RenderParams), vp, C.c_size_t, vp, vp]
    lib.ftl_render.restype = C.c_int
    lib.ftl_env_bytes.argtypes = [vp]
    lib.ftl_env_bytes.restype = C.c_size_t
    lib.ftl_env_layout_id.argtypes = [vp]
    lib.ftl_env_layout_id.restype = C.c_uint64
    lib.ftl_pack_envs.argtypes = [vp, vp, i32, vp, vp]
    lib.ftl_pack_envs.restype = C.c_int
    lib.ftl_unpack_envs.argtypes = [vp, vp, vp, i32, u32, vp]
    lib.ftl_unpack_envs.restype = C.c_int
    lib.ftl_unpack_envs_from.argtypes = [vp, vp, vp, vp, i32, u32, vp]
    lib.ftl_unpack_envs_from.restype = C.c_int
    lib.ftl_sizeof_search_params.restype = C.c_size_t
    lib.ftl_sizeof_search_buffers.restype = C.c_size_t
    lib.ftl_search_begin.argtypes = [vp, vp, i32, i32, C.c_uint64, i32, vp, vp]
    lib.ftl_search_begin.restype = C.c_int
    lib.ftl_search_sample.argtypes = [vp, vp, i32, C.POINTER(abi.SearchParams), C.c_uint64, i32, C.c_double, vp, vp, vp]
    lib.ftl_search_sample.restype = C.c_int
    lib.ftl_search_select.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.ftl_search_select.restype = C.c_int
    lib.ftl_search.argtypes = [vp, vp, C.POINTER(abi.SearchParams), C.c_uint64, i32, C.POINTER(abi.SearchBuffers), vp]
    lib.ftl_search.restype = C.c_int
    lib.ftl_sizeof_guided_buffers.restype = C.c_size_t
    lib.ftl_baseline_act_guided.argtypes = [vp, C.POINTER(abi.Outputs), vp, C.c_size_t, i32, vp, vp, vp]
    lib.ftl_baseline_act_guided.restype = C.c_int
    lib.ftl_rollout_guided.argtypes = [vp, i32, i32, C.c_double, C.POINTER(abi.Outputs), C.POINTER(abi.RolloutOutputs), vp, C.c_size_t, i32,
                                       vp, C.c_int64, vp, C.c_int64, u32, vp]
    lib.ftl_rollout_guided.restype = C.c_int
    lib.ftl_guided_fanout.argtypes = [vp, vp, i32, C.POINTER(abi.Outputs), C.POINTER(abi.Outputs), vp, C.c_size_t, vp, C.c_size_t, i32, vp]
    lib.ftl_guided_fanout.restype = C.c_int
    lib.ftl_search_guided.argtypes = [vp, vp, C.POINTER(abi.SearchParams), C.c_uint64, i32, i32, C.POINTER(abi.GuidedBuffers), vp]
    lib.ftl_search_guided.restype = C.c_int
    lib.ftl_sizeof_mlp.restype = C.c_size_t
    lib.ftl_mlp_param_count.argtypes = [C.POINTER(i32), i32]
    lib.ftl_mlp_param_count.restype = C.c_int64
    lib.ftl_mlp_act.argtypes = [vp, C.POINTER(abi.Outputs), C.POINTER(abi.Mlp), vp, vp]
    lib.ftl_mlp_act.restype = C.c_int
    lib.ftl_rollout_mlp.argtypes = [vp, i32, C.c_double, C.POINTER(abi.Outputs), C.POINTER(abi.RolloutOutputs), C.POINTER(abi.Mlp), vp, C.c_int64,
                                    u32, vp]
    lib.ftl_rollout_mlp.restype = C.c_int
    lib.ftl_sizeof_collect_buffers.restype = C.c_size_t
    lib.ftl_mlp_sample.argtypes = [vp, C.POINTER(abi.Outputs), C.POINTER(abi.Mlp), vp, vp, vp, vp, vp, vp]
    lib.ftl_mlp_sample.restype = C.c_int
    lib.ftl_collect_mlp.argtypes = [vp, i32, C.POINTER(abi.Outputs), C.POINTER(abi.Mlp), C.POINTER(abi.CollectBuffers), u32, vp]
    lib.ftl_collect_mlp.restype = C.c_int
    lib.ftl_gae.argtypes = [vp, i32, i32, vp, C.c_int64, vp, C.c_int64, vp, C.c_double, C.c_double, vp, vp, vp]
    lib.ftl_gae.restype = C.c_int
    lib.ftl_mlp_forward.argtypes = [vp, C.POINTER(abi.Mlp), i32, i32, vp, C.c_int64, vp, C.c_int64, vp]
    lib.ftl_mlp_forward.restype = C.c_int
    lib.ftl_mlp_backward.argtypes = [vp, C.POINTER(abi.Mlp), i32, i32, vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int64, vp]
    lib.ftl_mlp_backward.restype = C.c_int
    lib.ftl_sizeof_mlp_backward_workspace.argtypes = [C.POINTER(abi.Mlp), i32, i32]
    lib.ftl_sizeof_mlp_backward_workspace.restype = C.c_int64
    lib.ftl_sizeof_rnn.restype = C.c_size_t
    lib.ftl_sizeof_rnn_collect_buffers.restype = C.c_size_t
    lib.ftl_rnn_param_count.argtypes = [C.POINTER(i32), i32, i32, u32]
    lib.ftl_rnn_param_count.restype = C.c_int64
    lib.ftl_rnn_act.argtypes = [vp, C.POINTER(abi.Outputs), C.POINTER(abi.Rnn), vp, vp, vp, vp, vp, vp, u32, vp]
    lib.ftl_rnn_act.restype = C.c_int
    lib.ftl_rollout_rnn.argtypes = [vp, i32, C.c_double, C.POINTER(abi.Outputs), C.POINTER(abi.RolloutOutputs), C.POINTER(abi.Rnn), vp, C.c_int64,
                                    u32, vp]
    lib.ftl_rollout_rnn.restype = C.c_int
    lib.ftl_collect_rnn.argtypes = [vp, i32, C.POINTER(abi.Outputs), C.POINTER(abi.Rnn), C.POINTER(abi.RnnCollectBuffers), u32, vp]
    lib.ftl_collect_rnn.restype = C.c_int
    lib.ftl_sizeof_rnn_sequence.restype = C.c_size_t
    lib.ftl_rnn_forward.argtypes = [vp, C.POINTER(abi.Rnn), i32, i32, C.POINTER(abi.RnnSequence), vp]
    lib.ftl_rnn_forward.restype = C.c_int
    lib.ftl_sizeof_rnn_gradient.restype = C.c_size_t
    lib.ftl_sizeof_rnn_backward_workspace.argtypes = [C.POINTER(abi.Rnn), i32, i32]
    lib.ftl_sizeof_rnn_backward_workspace.restype = C.c_int64
    lib.ftl_rnn_backward.argtypes = [vp, C.POINTER(abi.Rnn), i32, i32, C.POINTER(abi.RnnSequence), C.POINTER(abi.RnnGradient), vp]
    lib.ftl_rnn_backward.restype = C.c_int
    lib.ftl_sizeof_ppo_head_args.restype = C.c_size_t
    lib.ftl_sizeof_ppo_head_workspace.argtypes = [i32, i32, i32]
    lib.ftl_sizeof_ppo_head_workspace.restype = C.c_int64
    lib.ftl_ppo_head.argtypes = [vp, C.POINTER(abi.PpoHeadArgs), vp]
    lib.ftl_ppo_head.restype = C.c_int
    lib.ftl_sizeof_episode_record.restype = C.c_size_t
    lib.ftl_sizeof_episode_queue.restype = C.c_size_t
    lib.ftl_set_episode_queue.argtypes = [vp, C.POINTER(abi.EpisodeQueueC)]
    lib.ftl_set_episode_queue.restype = C.c_int
    lib.ftl_queue_start.argtypes = [vp, C.POINTER(abi.Outputs), vp]
    lib.ftl_queue_start.restype = C.c_int
    lib.ftl_sizeof_scenario_sampler.restype = C.c_size_t
    lib.ftl_set_scenario_sampler.argtypes = [vp, C.POINTER(abi.ScenarioSamplerC)]
    lib.ftl_set_scenario_sampler.restype = C.c_int
    lib.ftl_sampler_refresh.argtypes = [vp, vp]
    lib.ftl_sampler_refresh.restype = C.c_int
    lib.ftl_sampler_start.argtypes = [vp, C.POINTER(abi.Outputs), vp]
    lib.ftl_sampler_start.restype = C.c_int
    # include/ftl_gazebo.h
    lib.ftl_gz_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    lib.ftl_gz_destroy.argtypes = [vp]
    lib.ftl_gz_destroy.restype = None
    lib.ftl_gz_state_bytes.argtypes = [vp]
    lib.ftl_gz_state_bytes.restype = C.c_size_t
    lib.ftl_gz_bind_state.argtypes = [vp, vp, C.c_size_t]
    lib.ftl_gz_lasers_len.argtypes = [vp]
    lib.ftl_gz_lasers_len.restype = i32
    lib.ftl_gz_reset.argtypes = [vp, vp, vp]
    lib.ftl_gz_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ftl_gz_state_field.argtypes = [vp, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(i32)]
    for n in ("ftl_sizeof_config", "ftl_sizeof_scenarios", "ftl_sizeof_outputs", "ftl_sizeof_final_outputs"):
        getattr(lib, n).restype = C.c_size_t
    _LIB = lib
    return lib


EXPORTS = ("ftl_create", "ftl_destroy", "ftl_lasers_len", "ftl_get_config", "ftl_state_bytes", "ftl_bind_state",
           "ftl_state_field", "ftl_load_scenarios", "ftl_set_reset_window", "ftl_tune", "ftl_reset", "ftl_step", "ftl_step_encoded", "ftl_step_final", "ftl_last_error", "ftl_generate_scenarios",
           "ftl_generate_scenarios_device_workspace", "ftl_generate_scenarios_device",
           "ftl_episode_metrics", "ftl_kernel_timing", "ftl_kernel_times",
           "ftl_sizeof_render_params", "ftl_render_workspace", "ftl_render",
           "ftl_env_bytes", "ftl_env_layout_id", "ftl_pack_envs", "ftl_unpack_envs",
           "ftl_sizeof_episode_record", "ftl_sizeof_episode_queue", "ftl_set_episode_queue", "ftl_queue_start",
           "ftl_sizeof_scenario_sampler", "ftl_set_scenario_sampler", "ftl_sampler_refresh", "ftl_sampler_start",
           "ftl_scan", "ftl_sizeof_rollout_outputs", "ftl_rollout",
           "ftl_baseline_bytes", "ftl_baseline_act", "ftl_rollout_baseline",
           "ftl_unpack_envs_from", "ftl_sizeof_search_params", "ftl_sizeof_search_buffers", "ftl_search_begin", "ftl_search_sample",
           "ftl_search_select", "ftl_search",
           "ftl_sizeof_guided_buffers", "ftl_baseline_act_guided", "ftl_rollout_guided", "ftl_guided_fanout", "ftl_search_guided",
           "ftl_sizeof_mlp", "ftl_mlp_param_count", "ftl_mlp_act", "ftl_rollout_mlp",
           "ftl_sizeof_collect_buffers", "ftl_mlp_sample", "ftl_collect_mlp", "ftl_gae", "ftl_mlp_forward", "ftl_mlp_backward", "ftl_sizeof_mlp_backward_workspace",
           "ftl_sizeof_rnn", "ftl_sizeof_rnn_collect_buffers", "ftl_rnn_param_count", "ftl_rnn_act", "ftl_rollout_rnn", "ftl_collect_rnn",
           "ftl_sizeof_rnn_sequence", "ftl_rnn_forward", "ftl_sizeof_rnn_gradient", "ftl_sizeof_rnn_backward_workspace", "ftl_rnn_backward",
           "ftl_sizeof_ppo_head_args", "ftl_sizeof_ppo_head_workspace", "ftl_ppo_head",
           "ftl_gz_create", "ftl_gz_destroy", "ftl_gz_state_bytes", "ftl_gz_bind_state", "ftl_gz_lasers_len", "ftl_gz_reset", "ftl_gz_step",
           "ftl_gz_state_field")


def check(rc, lib=None):
    if rc != 0:
        lib = lib or load()
        msg = lib.ftl_last_error().decode("utf-8", "replace")
        if rc == abi.FTL_E_INVALID:
            raise ValueError(msg)
        if rc == abi.FTL_E_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise FtlError("ftl error %d: %s" % (rc, msg))
