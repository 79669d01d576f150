"""ctypes binding of the C ABI in include/minppo_hip.h.

The product path loads exactly one library, `minppo_amd/libminppo_hip.so` (hand-written HIP for
gfx950, built by `__graft_entry__.build()` / `minppo_amd/build.py`), and raises if it is missing:
there is no CPU fallback.  (cffi, which the north star names, is not installed on the target
image; ctypes ABI mode is the same boundary.)

`Lib(path)` is also what the test-suite uses to bind the same ABI to the CPU SIMT-emulator
build of the kernel sources (tests/emu/), with NumPy arrays standing in for device memory.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

HERE = Path(__file__).resolve().parent
HIP_LIB_PATH = HERE / "libminppo_hip.so"

c_f = C.c_float
c_i32 = C.c_int32
c_u64 = C.c_uint64
c_sz = C.c_size_t
c_vp = C.c_void_p


class NativeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[mppo error {code}] {msg}")
        self.code = code


class ModelDims(C.Structure):
    _fields_ = [(n, c_i32) for n in ("nq", "nv", "nu", "nbody", "njnt", "ncon", "nlimit", "nefc", "obs_dim", "obs_pad",
                                     "rec_dim", "lds_bytes")] + [("timestep", c_f)]


class RewardCfg(C.Structure):
    _fields_ = [(n, c_f) for n in ("height_min_z", "height_max_z", "exp_coefficient", "subtraction_factor", "max_diff_norm",
                                   "w_ctrl_cost", "w_original_pos", "w_is_healthy", "w_velocity")]


class EnvMetrics(C.Structure):
    _fields_ = [(n, c_vp) for n in ("episode_returns", "episode_lengths", "returned_episode_returns",
                                    "returned_episode_lengths", "timestep", "returned_episode")]


class ForwardProbe(C.Structure):
    _fields_ = [(n, c_vp) for n in ("qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qacc_smooth", "efc_J", "efc_D",
                                    "efc_aref", "qacc", "cinert", "cvel", "subtree_com1", "xpos", "qacc_euler",
                                    "solver_niter")]


class Net(C.Structure):
    _fields_ = [(n, c_i32) for n in ("O", "OP", "A", "H", "use_tanh", "bf16", "num_layers")]  # num_layers 0 = 2 (the reference default)


class Batch(C.Structure):
    _fields_ = [("obs", c_vp), ("obs_ld", c_i32), ("action", c_vp), ("act_ld", c_i32), ("value", c_vp), ("log_prob", c_vp),
                ("adv", c_vp), ("target", c_vp)]


class GemmDesc(C.Structure):
    _fields_ = [(n, c_vp) for n in ("A", "B", "C", "bias", "aux", "gather", "bias_out")] + [(n, c_i32) for n in ("M", "N", "K", "lda", "ldb", "ldc", "ldaux", "act")]


class LossCfg(C.Structure):
    _fields_ = [("clip_eps", c_f), ("vf_coef", c_f), ("ent_coef", c_f)]


class AdamCfg(C.Structure):
    _fields_ = [("lr", c_f), ("max_grad_norm", c_f), ("b1", c_f), ("b2", c_f), ("eps", c_f), ("anneal", c_i32),
                ("sched_div", c_i32), ("num_updates", c_i32)]


class EngineCfg(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_steps", c_i32), ("num_minibatches", c_i32), ("update_epochs", c_i32),
                ("n_frames", c_i32), ("num_updates", c_i32), ("world_size", c_i32), ("rank", c_i32), ("gamma", c_f),
                ("gae_lambda", c_f), ("loss", LossCfg), ("adam", AdamCfg), ("reward", RewardCfg), ("net", Net),
                ("seed", c_u64), ("use_graph", c_i32), ("external_random", c_i32), ("rng_impl", c_i32), ("reserved0", c_i32)]


class EvalCfg(C.Structure):
    _fields_ = [("N", c_i32), ("K", c_i32), ("n_frames", c_i32), ("deterministic", c_i32), ("record_envs", c_i32), ("reset_noise_scale", c_f),
                ("seed", c_u64), ("reward", RewardCfg)]


class EvalResultRaw(C.Structure):  # mppo_eval_result_t (minppo_amd.evaluate.EvalResult is what callers see)
    _fields_ = [(n, C.c_int64) for n in ("episodes", "len_sum", "len_min", "len_max", "survivors", "steps")] + [
        (n, C.c_double) for n in ("ret_sum", "ret_sumsq", "ret_min", "ret_max", "survivor_ret_sum", "reward_sum")]


class PushCfg(C.Structure):  # mppo_push_cfg_t: random pushes (force 0: off)
    _fields_ = [("body", c_i32), ("interval", c_i32), ("duration", c_i32), ("rank", c_i32), ("force", c_f), ("seed", c_u64)]


class TimeLimitCfg(C.Structure):  # mppo_time_limit_cfg_t: the episode time limit of one mppo_env_time_limit launch (length >= 1)
    _fields_ = [("length", c_i32), ("stagger", c_i32), ("rank", c_i32), ("reserved", c_i32), ("seed", c_u64)]


class EvalLimitResultRaw(C.Structure):  # mppo_eval_limit_result_t
    _fields_ = [("truncated_episodes", C.c_int64), ("fallen_envs", C.c_int64)]


class DomainCfg(C.Structure):  # mppo_domain_cfg_t: domain randomisation (every range at its identity - 1 .. 1, 1 .. 1, 0 .. 0: off)
    _fields_ = [(n, c_f) for n in ("friction_min", "friction_max", "actuator_min", "actuator_max", "mass_min", "mass_max")] + [
        ("mass_body", c_i32), ("seed", c_u64), ("rank", c_i32)]


class ObsNoiseCfg(C.Structure):  # mppo_obs_noise_cfg_t: the stream of the sensor noise (the half-widths are a table of their own)
    _fields_ = [("seed", c_u64), ("rank", c_i32), ("reserved", c_i32)]


class ActionDelayCfg(C.Structure):  # mppo_action_delay_cfg_t: actuation latency in env steps (0 / 0: off)
    _fields_ = [("min", c_i32), ("max", c_i32), ("rank", c_i32), ("reserved", c_i32), ("seed", c_u64)]


class SceneDims(C.Structure):
    _fields_ = [(n, c_i32) for n in ("nq", "nbody", "ngeom", "ncam", "has_plane")]


class RenderOut(C.Structure):  # mppo_render_out_t: device pointers, any may be null
    _fields_ = [(n, c_vp) for n in ("rgb", "depth", "geom_id", "geom_pose")]


EVAL_ACC_SLOTS = 10  # include/minppo_hip.h: the accumulators of mppo_eval_accumulate / _reduce are 10 * N 8-byte words

P = C.POINTER
ABI_VERSION = 7  # include/minppo_hip.h: MPPO_ABI_VERSION

# name -> (restype, argtypes); restype c_i32 functions are checked and raise NativeError
SIGNATURES = {
    "mppo_last_error": (C.c_char_p, []),
    "mppo_abi_version": (c_i32, []),
    "mppo_model_open": (c_i32, [c_vp, c_sz, c_vp, P(c_vp)]),
    "mppo_model_close": (c_i32, [c_vp]),
    "mppo_model_get_dims": (c_i32, [c_vp, P(ModelDims)]),
    "mppo_model_is_specialized": (c_i32, [c_vp, P(c_i32)]),
    "mppo_model_scratch_bytes": (c_i32, [c_vp, c_i32, P(c_sz)]),
    "mppo_model_attach_kernel": (c_i32, [c_vp, c_vp, c_sz, P(C.c_char_p), c_i32, P(c_i32)]),
    "mppo_env_reset": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, P(EnvMetrics), c_vp]),
    "mppo_env_step": (c_i32, [c_vp, c_i32, c_i32, P(RewardCfg), c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp,
                              P(EnvMetrics), c_vp]),
    "mppo_env_reinit": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_f, c_i32, c_u64, c_i32, c_vp, c_vp, c_i32, c_vp]),
    "mppo_physics_forward": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, P(ForwardProbe), c_vp]),
    "mppo_env_step_xfrc": (c_i32, [c_vp, c_i32, c_i32, P(RewardCfg), c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp,
                                   P(EnvMetrics), c_i32, c_vp, c_vp]),
    "mppo_physics_forward_xfrc": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, P(ForwardProbe), c_i32, c_vp, c_vp]),
    "mppo_push_fill": (c_i32, [P(PushCfg), c_i32, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "mppo_env_time_limit": (c_i32, [c_vp, c_i32, P(TimeLimitCfg), c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, P(EnvMetrics), c_vp]),
    "mppo_gae_truncated": (c_i32, [c_i32, c_i32, c_f, c_f, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mppo_domain_fill": (c_i32, [P(DomainCfg), c_i32, c_vp, c_vp]),
    "mppo_env_reset_domain": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, P(EnvMetrics), c_vp, c_vp, c_i32, c_f, c_i32, c_u64, c_i32, c_vp, c_vp,
                                      c_i32, c_vp]),
    "mppo_env_step_domain": (c_i32, [c_vp, c_i32, c_i32, P(RewardCfg), c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, P(EnvMetrics), c_i32, c_vp, c_vp,
                                     c_i32, c_vp]),
    "mppo_physics_forward_domain": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, P(ForwardProbe), c_i32, c_vp, c_vp, c_i32, c_vp]),
    "mppo_obs_noise_apply": (c_i32, [P(ObsNoiseCfg), c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp]),
    "mppo_action_delay_fill": (c_i32, [P(ActionDelayCfg), c_i32, c_vp, c_vp]),
    "mppo_action_delay_apply": (c_i32, [P(ActionDelayCfg), c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp]),
    "mppo_param_count": (c_sz, [P(Net)]),
    "mppo_policy_ws_bytes": (c_sz, [P(Net), c_i32]),
    "mppo_policy_forward": (c_i32, [P(Net), c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mppo_gemm_batch": (c_i32, [P(GemmDesc), c_i32, c_i32, c_i32, c_sz, c_i32, c_vp]),
    "mppo_gae": (c_i32, [c_i32, c_i32, c_f, c_f, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mppo_grad_ws_bytes": (c_sz, [P(Net), c_i32]),
    "mppo_minibatch_path": (c_i32, [P(Net), P(Batch), P(c_i32)]),
    "mppo_minibatch_rows_per_workgroup": (c_i32, [P(Net), c_i32, c_i32, P(c_i32)]),
    "mppo_minibatch_grad": (c_i32, [P(Net), c_vp, P(Batch), c_vp, c_i32, c_vp, c_f, P(LossCfg), c_vp, c_vp, c_vp, c_sz,
                                    c_vp]),
    "mppo_minibatch_rowpass": (c_i32, [P(Net), c_vp, P(Batch), c_vp, c_i32, c_vp, c_f, P(LossCfg), c_vp, c_sz, c_vp]),
    "mppo_adv_sums": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "mppo_adv_stats_finalize": (c_i32, [c_vp, c_i32, C.c_double, c_vp, c_vp]),
    "mppo_adam_ws_bytes": (c_sz, [c_sz]),
    "mppo_clip_adam": (c_i32, [c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, P(AdamCfg), c_vp, c_sz, c_vp]),
    "mppo_shadow_refresh": (c_i32, [P(Net), c_vp, c_i32, c_vp, c_sz, c_vp]),
    "mppo_minibatch_rowpass_shadow": (c_i32, [P(Net), c_vp, P(Batch), c_vp, c_i32, c_vp, c_f, P(LossCfg), c_vp, c_sz, c_vp]),
    "mppo_minibatch_grad_shadow": (c_i32, [P(Net), c_vp, P(Batch), c_vp, c_i32, c_vp, c_f, P(LossCfg), c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mppo_clip_adam_shadow": (c_i32, [P(Net), c_i32, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, P(AdamCfg), c_vp, c_sz, c_vp]),
    "mppo_gather_rows": (c_i32, [P(Net), P(Batch), c_vp, c_i32, c_vp, c_sz, c_i32, c_vp]),
    "mppo_minibatch_rowpass_pre": (c_i32, [P(Net), c_vp, P(Batch), c_vp, c_vp, c_i32, c_vp, c_f, P(LossCfg), c_vp, c_sz, c_i32, c_vp]),
    "mppo_minibatch_grad_pre": (c_i32, [P(Net), c_vp, P(Batch), c_vp, c_vp, c_i32, c_vp, c_f, P(LossCfg), c_vp, c_vp, c_vp, c_sz, c_i32, c_vp]),
    "mppo_normal_fill": (c_i32, [c_u64, c_u64, c_sz, c_vp, c_vp]),
    "mppo_permutation_ws_bytes": (c_sz, [c_i32]),
    "mppo_permutation": (c_i32, [c_u64, c_u64, c_i32, c_vp, c_vp, c_sz, c_vp]),
    "mppo_threefry_normal": (c_i32, [c_vp, c_sz, c_vp, c_vp]),
    "mppo_threefry_bits": (c_i32, [c_vp, c_sz, c_vp, c_vp]),
    "mppo_threefry_update_keys": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "mppo_threefry_update_keys_step": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "mppo_threefry_permutation": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_sz, c_vp]),
    "mppo_obs_norm_partials": (c_i32, [c_i32]),
    "mppo_obs_norm_apply": (c_i32, [c_i32, c_i32, c_vp, c_i32, c_vp, c_i32, c_f, c_vp, c_vp]),
    "mppo_obs_norm_update": (c_i32, [c_i32, c_i32, C.c_int64, c_vp, c_vp, c_f, c_vp, c_i32, c_vp]),
    "mppo_obs_norm_rank_sums": (c_i32, [c_i32, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "mppo_reward_norm_partials": (c_i32, [c_i32]),
    "mppo_reward_norm_apply": (c_i32, [c_i32, c_i32, c_f, c_vp, c_vp, c_vp, c_vp, c_f, c_vp, c_vp, c_vp]),
    "mppo_engine_arena_bytes": (c_i32, [c_vp, P(EngineCfg), P(c_sz)]),
    "mppo_engine_create": (c_i32, [c_vp, P(EngineCfg), c_vp, c_sz, P(c_vp)]),
    "mppo_engine_destroy": (c_i32, [c_vp]),
    "mppo_engine_region": (c_i32, [c_vp, C.c_char_p, P(c_sz), P(c_sz)]),
    "mppo_comm_unique_id": (c_i32, [c_vp]),
    "mppo_engine_comm_init": (c_i32, [c_vp, c_vp]),
    "mppo_engine_peer_export": (c_i32, [c_vp, c_vp]),
    "mppo_engine_peer_connect": (c_i32, [c_vp, c_vp, c_i32]),
    "mppo_engine_comm_mode": (c_i32, [c_vp, P(c_i32)]),
    "mppo_engine_peer_status": (c_i32, [c_vp, P(c_i32), P(c_i32)]),
    "mppo_engine_peer_selftest": (c_i32, [c_vp, c_vp, P(c_i32)]),
    "mppo_engine_peer_latency": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, P(C.c_double)]),
    "mppo_engine_peer_disable": (c_i32, [c_vp]),
    "mppo_engine_reset": (c_i32, [c_vp, c_vp]),
    "mppo_engine_set_reset_noise": (c_i32, [c_vp, c_f]),
    "mppo_engine_set_obs_norm": (c_i32, [c_vp, c_i32, c_f, c_f]),
    "mppo_engine_set_reward_norm": (c_i32, [c_vp, c_i32, c_f, c_f]),
    "mppo_engine_set_push": (c_i32, [c_vp, P(PushCfg)]),
    "mppo_engine_set_time_limit": (c_i32, [c_vp, c_i32, c_i32]),
    "mppo_engine_set_domain": (c_i32, [c_vp, P(DomainCfg)]),
    "mppo_engine_set_obs_noise": (c_i32, [c_vp, c_vp]),
    "mppo_engine_set_action_delay": (c_i32, [c_vp, c_i32, c_i32]),
    "mppo_engine_update": (c_i32, [c_vp, c_vp]),
    "mppo_engine_prepare": (c_i32, [c_vp, c_vp]),
    "mppo_engine_graph_active": (c_i32, [c_vp, P(c_i32)]),
    "mppo_engine_rollout": (c_i32, [c_vp, c_vp]),
    "mppo_engine_learn": (c_i32, [c_vp, c_vp]),
    "mppo_eval_ws_bytes": (c_sz, [c_vp, P(Net), P(EvalCfg)]),
    "mppo_evaluate": (c_i32, [c_vp, P(Net), c_vp, P(EvalCfg), c_vp, c_sz, c_vp, c_vp, c_vp]),
    "mppo_evaluate_obs_norm": (c_i32, [c_vp, P(Net), c_vp, P(EvalCfg), c_vp, c_sz, c_vp, c_f, c_vp, c_vp, c_vp]),
    "mppo_evaluate_push": (c_i32, [c_vp, P(Net), c_vp, P(EvalCfg), c_vp, c_sz, c_vp, c_f, P(PushCfg), c_vp, c_vp, c_vp]),
    "mppo_eval_accumulate": (c_i32, [c_i32, c_i32, c_vp, c_vp, P(EnvMetrics), c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mppo_eval_reduce": (c_i32, [c_i32, c_i32, c_vp, c_vp, c_vp]),
    "mppo_eval_limit_ws_bytes": (c_sz, [c_vp, P(Net), P(EvalCfg)]),
    "mppo_evaluate_limit": (c_i32, [c_vp, P(Net), c_vp, P(EvalCfg), c_vp, c_sz, c_vp, c_f, P(PushCfg), c_i32, c_vp, c_vp, c_vp, c_vp]),
    "mppo_eval_limit_count": (c_i32, [c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "mppo_eval_limit_reduce": (c_i32, [c_i32, c_vp, c_vp, c_vp]),
    "mppo_eval_domain_ws_bytes": (c_sz, [c_vp, P(Net), P(EvalCfg)]),
    "mppo_evaluate_domain": (c_i32, [c_vp, P(Net), c_vp, P(EvalCfg), c_vp, c_sz, c_vp, c_f, P(PushCfg), c_i32, P(DomainCfg), c_vp, c_vp, c_vp, c_vp]),
    "mppo_eval_sensors_ws_bytes": (c_sz, [c_vp, P(Net), P(EvalCfg)]),
    "mppo_evaluate_sensors": (c_i32, [c_vp, P(Net), c_vp, P(EvalCfg), c_vp, c_sz, c_vp, c_f, P(PushCfg), c_i32, P(DomainCfg), c_vp, P(ActionDelayCfg), c_vp, c_vp, c_vp,
                                      c_vp, c_vp]),
    "mppo_scene_open": (c_i32, [c_vp, c_sz, c_vp, P(c_vp)]),
    "mppo_scene_close": (c_i32, [c_vp]),
    "mppo_scene_get_dims": (c_i32, [c_vp, P(SceneDims)]),
    "mppo_render": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, P(RenderOut), c_vp]),
}

UNCHECKED = {"mppo_last_error", "mppo_abi_version", "mppo_param_count", "mppo_policy_ws_bytes", "mppo_grad_ws_bytes",
             "mppo_adam_ws_bytes", "mppo_permutation_ws_bytes", "mppo_eval_ws_bytes", "mppo_eval_limit_ws_bytes", "mppo_eval_domain_ws_bytes", "mppo_eval_sensors_ws_bytes", "mppo_obs_norm_partials",
             "mppo_reward_norm_partials"}


class Lib:
    """One loaded instance of the C ABI."""

    def __init__(self, path: os.PathLike | str):
        self.path = str(path)
        # RTLD_LOCAL (the default): the test-suite's emulator build exports the same C++ symbols; with global visibility whichever
        # library came first would serve the other's internal calls
        self._dll = C.CDLL(self.path)
        self._fn = {}
        for name, (res, args) in SIGNATURES.items():
            try:
                f = getattr(self._dll, name)
            except AttributeError:
                continue
            f.restype = res
            f.argtypes = args
            self._fn[name] = f

    def has(self, name: str) -> bool:
        return name in self._fn

    def exported(self):
        return sorted(self._fn)

    def last_error(self) -> str:
        return self._fn["mppo_last_error"]().decode("utf-8", "replace")

    def __getattr__(self, name: str):
        key = "mppo_" + name
        fn = self.__dict__.get("_fn", {}).get(key)
        if fn is None:
            raise AttributeError(f"{self.path} does not export {key}")
        if key in UNCHECKED:
            return fn

        def checked(*a):
            rc = fn(*a)
            if rc != 0:
                raise NativeError(rc, self.last_error())
            return rc

        return checked


_LIB: Optional[Lib] = None


def load() -> Lib:
    """Loads the HIP engine.  Raises if it has not been built: no CPU fallback exists."""
    global _LIB
    if _LIB is None:
        if not HIP_LIB_PATH.exists():
            raise ImportError(
                f"{HIP_LIB_PATH} is missing: build the gfx950 engine first (python -c 'import __graft_entry__ as g; "
                f"g.build()' or python -m minppo_amd.build). minppo_amd has no CPU fallback."
            )
        # torch ships its own HIP runtime / RCCL with the same SONAMEs; import it first so that the
        # engine binds to the runtime instance that owns torch's streams and allocations.
        import torch  # noqa: F401

        _LIB = Lib(HIP_LIB_PATH)
        if _LIB.abi_version() != ABI_VERSION:
            raise ImportError(f"{HIP_LIB_PATH}: ABI version {_LIB.abi_version()} != {ABI_VERSION} (rebuild: python -m minppo_amd.build)")
    return _LIB


def ptr(x) -> int:
    """Device (torch) or host (numpy) array -> raw address."""
    if x is None:
        return 0
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return x.ctypes.data
