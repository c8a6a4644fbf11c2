"""ctypes binding of include/carl_amd.h (libcarl_amd.so).

There is NO CPU fallback: if the HIP library is missing the import of the engine
fails loudly.  ``torch`` is imported first so that the library binds to the HIP
runtime PyTorch-ROCm already loaded (same ``libamdhip64.so.7``), which is what makes
``tensor.data_ptr()`` and ``torch.cuda.current_stream().cuda_stream`` valid on the
other side of the C ABI.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

from carl_amd import build as _build

CARL_ABI_VERSION = 9
CARL_MAX_CTX_OBS = 32

# carl_family_t
CARTPOLE, PENDULUM, ACROBOT, MOUNTAINCAR, MOUNTAINCAR_CONT = range(5)
CARL_N_FAMILIES = 5
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2  # CARL_ERR_* (include/carl_amd.h)
# carl_selector_t
SEL_STATIC, SEL_ROUND_ROBIN, SEL_RANDOM, SEL_HOST = range(4)
FLAG_AUTORESET = 1
FLAG_CARTPOLE_RECOMPUTE = 2
FLAG_ACROBOT_FP32 = 4
FLAG_AUTORESET_FIRST_STATE = 8
FLAG_ROLLOUT_DIRECT = 16
FLAG_BRAX_GENERIC = 32
FLAG_BRAX_FP32 = 64  # opt-in: float32 pose algebra in the substeps (include/carl_amd.h: CARL_FLAG_BRAX_FP32)
ROLLOUT_STAGED, ROLLOUT_DIRECT_SHAPE, ROLLOUT_DIRECT_FLAG = range(3)
ACTION_I32, ACTION_I64, ACTION_F32, ACTION_U8, ACTION_F16, ACTION_BF16 = range(6)

_vp = C.c_void_p


class FamilyInfo(C.Structure):
    _fields_ = [
        ("state_dim", C.c_int32), ("obs_dim", C.c_int32), ("n_features", C.c_int32),
        ("action_dim", C.c_int32), ("action_is_discrete", C.c_int32), ("n_actions", C.c_int32),
        ("max_episode_steps", C.c_int32), ("reserved", C.c_int32),
        ("action_low", C.c_float), ("action_high", C.c_float),
    ]


class Batch(C.Structure):
    _fields_ = [
        ("family", C.c_int32), ("n_lanes", C.c_int32), ("n_contexts", C.c_int32),
        ("ctx_stride", C.c_int32), ("max_episode_steps", C.c_int32), ("selector", C.c_int32),
        ("selector_stride", C.c_int32), ("flags", C.c_int32),
        ("lane_offset", C.c_int64), ("seed", C.c_uint64),
        ("state", _vp), ("elapsed", _vp), ("ctx_idx", _vp), ("episode", _vp), ("n_calls", _vp),
        ("ep_return", _vp),
        ("ctx_table", _vp), ("ctx_obs", _vp),
        ("n_ctx_obs", C.c_int32), ("ctx_obs_feat", C.c_int32 * CARL_MAX_CTX_OBS),
        ("fin_capacity", C.c_int32),
        ("last_return", _vp), ("last_length", _vp), ("episodes_done", _vp),
        ("fin_count", _vp), ("fin_lane", _vp), ("fin_return", _vp), ("fin_length", _vp),
        ("goal_pos", _vp), ("success", _vp), ("first_state", _vp),
    ]


class StepIO(C.Structure):
    _fields_ = [
        ("action", _vp), ("action_dtype", C.c_int32), ("row_pitch", C.c_int32),
        ("obs", _vp), ("reward", _vp), ("terminated", _vp), ("truncated", _vp), ("final_obs", _vp), ("done", _vp),
        ("branch_sig", _vp),
    ]


class RolloutPlan(C.Structure):
    """carl_rollout_plan_t: which kernel instance a launch takes (carl_rollout_plan_io; host logic, no GPU needed)"""
    _fields_ = [(k, C.c_int32) for k in ("variant", "lean", "unsupported", "ak", "plain", "ldsctx", "moves", "fin", "ar",
                                          "deep", "has_staged_kernel", "use_lds_ctx", "step_block", "acrobot_fp32")] + [
        ("lds_bytes", C.c_int64)]


EXPORTS = {
    "carl_abi_version": (C.c_int, []),
    "carl_last_error": (C.c_char_p, []),
    "carl_family_info": (C.c_int, [C.c_int, C.POINTER(FamilyInfo)]),
    "carl_reset": (C.c_int, [C.POINTER(Batch), _vp, _vp, _vp]),
    "carl_reset_indexed": (C.c_int, [C.POINTER(Batch), _vp, _vp, _vp, _vp]),
    "carl_step": (C.c_int, [C.POINTER(Batch), C.POINTER(StepIO), _vp]),
    "carl_rollout": (C.c_int, [C.POINTER(Batch), C.POINTER(StepIO), C.c_int32, _vp]),
    "carl_rollout_pair": (C.c_int, [C.POINTER(Batch), C.POINTER(StepIO), C.POINTER(Batch), C.POINTER(StepIO), C.c_int32, _vp]),
    "carl_rollout_variant": (C.c_int, [C.POINTER(Batch)]),
    "carl_rollout_variant_io": (C.c_int, [C.POINTER(Batch), C.POINTER(StepIO)]),
    "carl_rollout_plan_io": (C.c_int, [C.POINTER(Batch), C.POINTER(StepIO), C.POINTER(RolloutPlan)]),
    "carl_rollout_pitch": (C.c_int32, [C.c_int32]),
    "carl_done_compact": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp]),
    "carl_done_compact_scratch_elems": (C.c_int32, [C.c_int32]),
}


class CarlHipError(RuntimeError):
    pass


_lib = None


def lib_path() -> str:
    return _build.LIB_PATH


def load() -> C.CDLL:
    """Load libcarl_amd.so (building it in-tree first if hipcc is here and the
    sources are newer).  Raises if the library cannot be produced or loaded."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    override = os.environ.get("CARL_AMD_LIB_PATH")  # kernel experiments: load another build
    if override:
        path = override
    elif os.environ.get("CARL_AMD_NO_BUILD", "0") != "1":
        try:
            path = _build.build()
        except Exception as e:  # hipcc absent / compile error
            if not os.path.exists(path):
                raise CarlHipError(
                    f"libcarl_amd.so is missing and could not be built ({e}); the engine has "
                    "no CPU fallback -- run `python -m carl_amd.build` on a machine with hipcc"
                ) from e
    if not os.path.exists(path):
        raise CarlHipError(f"{path} not found; run `python -m carl_amd.build`")
    lib = C.CDLL(path)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)  # AttributeError = ABI drift, fail loudly
        fn.restype = res
        fn.argtypes = args
    v = lib.carl_abi_version()
    if v != CARL_ABI_VERSION:
        raise CarlHipError(f"libcarl_amd ABI version {v} != binding {CARL_ABI_VERSION}")
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != 0:
        msg = load().carl_last_error()
        raise CarlHipError(f"libcarl_amd call failed ({code}): {msg.decode() if msg else ''}")


def family_info(family: int) -> FamilyInfo:
    info = FamilyInfo()
    check(load().carl_family_info(family, C.byref(info)))
    return info


# ---- Brax-locomotion families (carl_brax_sys_t, include/carl_amd.h) ----------------------
BRAX_MAX_LINKS, BRAX_MAX_DOF, BRAX_MAX_Q, BRAX_MAX_ACT, BRAX_MAX_COLL, BRAX_MAX_CTX_MASS = 16, 24, 32, 24, 32, 16
BRAX_MAX_PAIR = 8
(BRAX_ANT, BRAX_HALFCHEETAH, BRAX_HUMANOID, BRAX_HOPPER, BRAX_WALKER2D, BRAX_INVERTED_PENDULUM, BRAX_HUMANOIDSTANDUP, BRAX_INVERTED_DOUBLE_PENDULUM,
 BRAX_REACHER, BRAX_PUSHER) = range(10)
BRAX_LINK_STATE = 13
BRAX_LINK_RECORD = 20  # floats per (env, link) in HBM: pose head 7 | pose tail 7 | velocities 6 (include/carl_amd.h, ABI 8)
_f, _i = C.c_float, C.c_int32


class BraxCtxMap(C.Structure):
    _fields_ = [
        ("gravity", _i), ("friction", _i), ("elasticity", _i), ("ang_damping", _i),
        ("joint_stiffness_scale", _i), ("target_distance", _i), ("target_direction", _i), ("target_radius", _i),
        ("n_mass", _i),
        ("mass_row", _i * BRAX_MAX_CTX_MASS), ("mass_link", _i * BRAX_MAX_CTX_MASS),
        ("mass_nominal", _f * BRAX_MAX_CTX_MASS), ("mass_ratio_floor", _f * BRAX_MAX_CTX_MASS),
        ("mass_ratio_floor_multi", _f * BRAX_MAX_CTX_MASS),
        ("goal_position", _i * 3),
    ]


class BraxSys(C.Structure):
    _fields_ = [
        ("env_kind", _i), ("n_links", _i), ("n_q", _i), ("n_dof", _i), ("n_act", _i), ("n_coll", _i),
        ("n_frames", _i), ("obs_dim", _i), ("max_episode_steps", _i), ("terminate_when_unhealthy", _i),
        ("exclude_current_positions", _i), ("reserved", _i),
        ("dt", _f), ("gravity_z", _f), ("vel_damping", _f), ("ang_damping", _f), ("baumgarte_erp", _f),
        ("elasticity", _f), ("friction", _f),
        ("healthy_z_lo", _f), ("healthy_z_hi", _f), ("healthy_reward", _f), ("ctrl_cost_weight", _f),
        ("forward_reward_weight", _f), ("reset_noise_scale", _f), ("reset_vel_scale", _f),
        ("parent", _i * BRAX_MAX_LINKS), ("n_link_dof", _i * BRAX_MAX_LINKS),
        ("q_start", _i * BRAX_MAX_LINKS), ("dof_start", _i * BRAX_MAX_LINKS),
        ("link_pos", (_f * 3) * BRAX_MAX_LINKS), ("link_rot", (_f * 4) * BRAX_MAX_LINKS),
        ("joint_pos", (_f * 3) * BRAX_MAX_LINKS), ("joint_rot", (_f * 4) * BRAX_MAX_LINKS),
        ("com", (_f * 3) * BRAX_MAX_LINKS), ("mass", _f * BRAX_MAX_LINKS),
        ("inv_inertia", (_f * 3) * BRAX_MAX_LINKS),
        ("k_pos", _f * BRAX_MAX_LINKS), ("k_vel", _f * BRAX_MAX_LINKS),
        ("k_limit", _f * BRAX_MAX_LINKS), ("k_ang_damp", _f * BRAX_MAX_LINKS),
        ("dof_lo", _f * BRAX_MAX_DOF), ("dof_hi", _f * BRAX_MAX_DOF),
        ("dof_damping", _f * BRAX_MAX_DOF), ("dof_stiffness", _f * BRAX_MAX_DOF),
        ("act_dof", _i * BRAX_MAX_ACT), ("act_gear", _f * BRAX_MAX_ACT),
        ("act_lo", _f * BRAX_MAX_ACT), ("act_hi", _f * BRAX_MAX_ACT),
        ("coll_link", _i * BRAX_MAX_COLL), ("coll_pos", (_f * 3) * BRAX_MAX_COLL),
        ("coll_radius", _f * BRAX_MAX_COLL),
        ("init_q", _f * BRAX_MAX_Q),
        ("goal_mode", _i), ("goal_obs_idx", _i * 2), ("goal_dt", _f),
        ("n_slide", _i * BRAX_MAX_LINKS), ("dof_sign3", _f * BRAX_MAX_LINKS),
        ("reset_vel_uniform", _i), ("reward_on_com", _i), ("obs_extended", _i), ("healthy_q_index", _i),
        ("healthy_q_lo", _f), ("healthy_q_hi", _f), ("obs_qd_clip", _f), ("lanes_per_env", _i),
        ("reward_height", _i), ("obs_trig_from", _i),
        ("tip_link", _i), ("tip_offset", _f * 3), ("tip_x_weight", _f), ("tip_height", _f), ("tip_min_height", _f),
        ("tip_vel_weight", _f * 2), ("tip_vel_dof", _i * 2),
        ("target_link", _i), ("target_max_dist", _f),
        ("push_link", _i), ("push_goal", _f * 3), ("push_near_weight", _f), ("push_min_dist", _f),
        ("push_lo", _f * 2), ("push_hi", _f * 2),
        ("n_pair", _i), ("pair_link", _i), ("pair_pos", (_f * 3) * BRAX_MAX_PAIR), ("pair_radius", _f * BRAX_MAX_PAIR),
        ("pair_obj_radius", _f), ("pair_obj_half", _f), ("pair_k", _f), ("pair_c", _f),
        ("pair_ct", _f), ("plane_z", _f), ("obj_support", _i), ("reserved2", _i),
        ("slide_axis", ((_f * 3) * 2) * BRAX_MAX_LINKS),
        ("ctx", BraxCtxMap),
    ]


EXPORTS.update({
    "carl_brax_reset": (C.c_int, [C.POINTER(Batch), _vp, C.POINTER(BraxSys), _vp, _vp, _vp]),
    "carl_brax_step": (C.c_int, [C.POINTER(Batch), _vp, C.POINTER(BraxSys), C.POINTER(StepIO), _vp]),
    "carl_brax_rollout": (C.c_int, [C.POINTER(Batch), _vp, C.POINTER(BraxSys), C.POINTER(StepIO), C.c_int32, _vp]),
    "carl_brax_lane_widths": (C.c_int, [C.POINTER(BraxSys), C.c_uint32, _vp, C.c_int32]),
    "carl_brax_model_is_planar": (C.c_int, [C.POINTER(BraxSys)]),
    "carl_brax_fragment_plan": (C.c_int, [C.c_int32] * 6 + [_vp, C.c_int32]),
})


# ---- context sets on the device (include/carl_amd.h: carl_feature_spec_t) --------------------
MAX_CHOICES = 32
FEAT_CONSTANT, FEAT_UNIFORM_FLOAT, FEAT_NORMAL_FLOAT, FEAT_UNIFORM_INT, FEAT_CATEGORICAL = range(5)


class FeatureSpec(C.Structure):
    _fields_ = [
        ("kind", _i), ("n_choices", _i), ("log_scale", _i), ("reserved", _i),
        ("lower", _f), ("upper", _f), ("mu", _f), ("sigma", _f), ("value", _f), ("reserved_f", _f),
        ("choices", _f * MAX_CHOICES),
    ]


EXPORTS.update({
    "carl_sample_contexts": (C.c_int, [_vp, C.POINTER(FeatureSpec), C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                       C.c_uint64, _vp, _vp]),
    "carl_verify_contexts": (C.c_int, [_vp, C.POINTER(FeatureSpec), C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
})


# ---- closed-loop rollout: a policy network on the device (include/carl_amd.h: carl_policy_t) ------------------
POLICY_MAX_IN, POLICY_MAX_HIDDEN, POLICY_MAX_WIDTH = 32, 2, 64
POLICY_IDENTITY, POLICY_TANH, POLICY_RELU = range(3)
POLICY_HEAD_ARGMAX, POLICY_HEAD_BOX = range(2)


class Policy(C.Structure):
    _fields_ = [
        ("n_in", _i), ("n_ctx", _i), ("ctx_rows", _i * POLICY_MAX_IN), ("n_hidden", _i),
        ("width", _i * POLICY_MAX_HIDDEN), ("n_out", _i), ("activation", _i), ("head", _i), ("n_sets", _i),
        ("lanes_per_set", _i), ("reserved", _i), ("params", _vp),
    ]


class PolicySummary(C.Structure):
    _fields_ = [("episodes", _vp), ("return_sum", _vp), ("length_sum", _vp)]


class PolicyEpisodes(C.Structure):
    _fields_ = [("episodes", _vp), ("steps", _vp), ("ret", _vp), ("length", _vp), ("context_id", _vp),
                ("terminated", _vp)]


class PolicySampling(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("log_std", _vp), ("log_prob", _vp)]


EXPORTS.update({
    "carl_rollout_policy": (C.c_int, [C.POINTER(Batch), C.POINTER(Policy), C.POINTER(StepIO), C.c_int32,
                                      C.POINTER(PolicySummary), _vp]),
    "carl_rollout_policy_sampled": (C.c_int, [C.POINTER(Batch), C.POINTER(Policy), C.POINTER(PolicySampling),
                                              C.POINTER(StepIO), C.c_int32, C.POINTER(PolicySummary), _vp]),
    "carl_evaluate_policy_sampled": (C.c_int, [C.POINTER(Batch), C.POINTER(Policy), C.POINTER(PolicySampling), C.c_int32,
                                               C.c_int32, C.POINTER(PolicyEpisodes), _vp]),
    "carl_policy_lane_quantum": (C.c_int32, []),
    "carl_policy_set_floats": (C.c_int32, [C.POINTER(Policy)]),
    "carl_evaluate_policy": (C.c_int, [C.POINTER(Batch), C.POINTER(Policy), C.c_int32, C.c_int32,
                                       C.POINTER(PolicyEpisodes), _vp]),
})


# ---- closed-loop rollout of the Brax families (include/carl_amd.h: carl_brax_rollout_policy) ------------------------
class BraxLaunchShape(C.Structure):
    """carl_brax_launch_shape_t: the shape of a carl_brax_rollout_policy launch (carl_brax_policy_launch_shape; host logic)"""
    _fields_ = [("grid", _i), ("waves_per_workgroup", _i), ("lanes_per_env", _i), ("reserved", _i),
                ("lds_bytes", C.c_int64)]


EXPORTS.update({
    "carl_brax_rollout_policy": (C.c_int, [C.POINTER(Batch), _vp, C.POINTER(BraxSys), _vp, C.POINTER(Policy),
                                           C.POINTER(StepIO), C.c_int32, C.POINTER(PolicySummary), _vp]),
    "carl_brax_rollout_policy_sampled": (C.c_int, [C.POINTER(Batch), _vp, C.POINTER(BraxSys), _vp, C.POINTER(Policy),
                                                   C.POINTER(PolicySampling), C.POINTER(StepIO), C.c_int32,
                                                   C.POINTER(PolicySummary), _vp]),
    "carl_brax_evaluate_policy": (C.c_int, [C.POINTER(Batch), _vp, C.POINTER(BraxSys), _vp, C.POINTER(Policy), C.c_int32,
                                            C.c_int32, C.POINTER(PolicyEpisodes), _vp]),
    "carl_brax_policy_set_floats": (C.c_int32, [C.POINTER(Policy)]),
    "carl_brax_policy_launch_shape": (C.c_int, [C.POINTER(Batch), C.POINTER(BraxSys), C.POINTER(Policy), C.c_int32,
                                                C.POINTER(BraxLaunchShape)]),
    "carl_brax_launch_shape": (C.c_int, [C.POINTER(Batch), C.POINTER(BraxSys), C.c_int32, C.c_int32,
                                         C.POINTER(BraxLaunchShape)]),
})


# ---- a critic in the closed-loop launch, and GAE (include/carl_amd.h: carl_policy_value_t, carl_gae_t) ----------
class PolicyValue(C.Structure):
    _fields_ = [("value", _vp), ("last_value", _vp), ("boot_value", _vp)]


class Gae(C.Structure):
    _fields_ = [("n_lanes", _i), ("n_steps", _i), ("row_pitch", _i), ("gamma", C.c_float), ("lam", C.c_float),
                ("reserved", _i), ("reward", _vp), ("value", _vp), ("boot_value", _vp), ("last_value", _vp),
                ("terminated", _vp), ("truncated", _vp), ("advantage", _vp), ("ret", _vp)]


EXPORTS.update({
    "carl_rollout_policy_valued": (C.c_int, [C.POINTER(Batch), C.POINTER(Policy), C.POINTER(Policy),
                                             C.POINTER(PolicySampling), C.POINTER(StepIO), C.c_int32,
                                             C.POINTER(PolicySummary), C.POINTER(PolicyValue), _vp]),
    "carl_gae": (C.c_int, [C.POINTER(Gae), _vp]),
    "carl_brax_rollout_policy_valued": (C.c_int, [C.POINTER(Batch), _vp, C.POINTER(BraxSys), _vp, C.POINTER(Policy),
                                                  C.POINTER(Policy), C.POINTER(PolicySampling), C.POINTER(StepIO),
                                                  C.c_int32, C.POINTER(PolicySummary), C.POINTER(PolicyValue), _vp]),
})


# ---- evolution strategies on the device (include/carl_amd.h: carl_es_t) ---------------------------------------
class Es(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("generation", C.c_uint32), ("n_pairs", _i), ("set_floats", _i), ("n_noisy", _i),
                ("sigma", C.c_float), ("reserved", _i)]


EXPORTS.update({
    "carl_es_perturb": (C.c_int, [C.POINTER(Es), _vp, _vp, _vp, _vp]),
    "carl_es_gradient": (C.c_int, [C.POINTER(Es), _vp, _vp, _vp]),
    "carl_es_slice_pairs": (C.c_int32, []),
})


# ---- input statistics inside the episodes launch (include/carl_amd.h: carl_policy_stats_t) --------------------
class PolicyStats(C.Structure):
    _fields_ = [("partial", _vp), ("partial_capacity", _i)]


class PolicyRunningStats(C.Structure):
    _fields_ = [("count", _vp), ("mean", _vp), ("m2", _vp)]


EXPORTS.update({
    "carl_policy_stats_workgroups": (C.c_int32, [C.c_int32]),
    "carl_evaluate_policy_stats": (C.c_int, [C.POINTER(Batch), C.POINTER(Policy), C.POINTER(PolicySampling), C.c_int32,
                                             C.c_int32, C.POINTER(PolicyEpisodes), C.POINTER(PolicyStats), _vp]),
    "carl_policy_stats_merge": (C.c_int, [C.POINTER(Policy), C.POINTER(PolicyStats), C.c_int32, _vp, C.c_int32,
                                          C.POINTER(PolicyRunningStats), C.c_double, C.c_double, _vp, C.c_int32, _vp]),
    # the Brax families' (carl_brax_evaluate_policy gathering the sums; one slab per wavefront of the launch)
    "carl_brax_policy_stats_slabs": (C.c_int32, [C.POINTER(Batch), C.POINTER(BraxSys), C.POINTER(Policy), C.c_int32]),
    "carl_brax_evaluate_policy_stats": (C.c_int, [C.POINTER(Batch), _vp, C.POINTER(BraxSys), _vp, C.POINTER(Policy), C.c_int32,
                                                  C.c_int32, C.POINTER(PolicyEpisodes), C.POINTER(PolicyStats), _vp]),
    "carl_brax_policy_stats_merge": (C.c_int, [C.POINTER(Policy), C.POINTER(PolicyStats), C.c_int32, _vp, C.c_int32,
                                               C.POINTER(PolicyRunningStats), C.c_double, C.c_double, _vp, C.c_int32, _vp]),
})


# ---- the PPO update on the device (include/carl_amd.h: carl_policy_context_trace, carl_ppo_batch_t) ---------------
class PpoBatch(C.Structure):
    _fields_ = [("family", _i), ("n_lanes", _i), ("n_steps", _i), ("row_pitch", _i), ("obs_dim", _i), ("n_contexts", _i),
                ("ctx_stride", _i), ("action_dtype", _i), ("n_samples", _i), ("reserved", _i),
                ("clip_range", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float), ("reserved2", _i),
                ("obs0", _vp), ("obs", _vp), ("context_id", _vp), ("ctx_table", _vp), ("action", _vp), ("log_prob", _vp),
                ("advantage", _vp), ("ret", _vp), ("idx", _vp), ("adv_norm", _vp)]


class PpoOut(C.Structure):
    _fields_ = [("grad_actor", _vp), ("grad_critic", _vp), ("grad_log_std", _vp), ("stats", _vp), ("new_log_prob", _vp),
                ("new_value", _vp), ("workspace", _vp), ("workspace_floats", C.c_int64)]


EXPORTS.update({
    "carl_policy_context_trace": (C.c_int, [C.POINTER(Batch), _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _vp]),
    "carl_ppo_tile": (C.c_int32, []),
    "carl_ppo_grad_workgroups": (C.c_int32, [C.c_int32]),
    "carl_ppo_workspace_floats": (C.c_int64, [C.POINTER(Policy), C.POINTER(Policy), C.c_int32]),
    "carl_ppo_grad": (C.c_int, [C.POINTER(PpoBatch), C.POINTER(Policy), C.POINTER(Policy), _vp, C.POINTER(PpoOut), _vp]),
    # the Brax families' (dense rows; a joint Gaussian over the model's actuators: carl_brax_ppo_grad)
    "carl_brax_policy_context_trace": (C.c_int, [C.POINTER(Batch), _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "carl_brax_ppo_tile": (C.c_int32, []),
    "carl_brax_ppo_grad_workgroups": (C.c_int32, [C.c_int32]),
    "carl_brax_ppo_workspace_floats": (C.c_int64, [C.POINTER(Policy), C.POINTER(Policy), C.c_int32]),
    "carl_brax_ppo_grad": (C.c_int, [C.POINTER(PpoBatch), C.POINTER(BraxSys), C.POINTER(Policy), C.POINTER(Policy), _vp,
                                     C.POINTER(PpoOut), _vp]),
})


# ---- PPO's running normalisation (include/carl_amd.h: carl_ppo_input_stats, carl_ppo_return_stats_t) ----------------
class PpoReturnStats(C.Structure):
    _fields_ = [("n_lanes", _i), ("n_steps", _i), ("row_pitch", _i), ("gamma", C.c_float), ("reward", _vp),
                ("terminated", _vp), ("truncated", _vp), ("ret", _vp), ("ret_rows", _vp), ("partial", _vp),
                ("partial_capacity", _i), ("reserved", _i)]


EXPORTS.update({
    "carl_ppo_input_stats_slabs": (C.c_int32, [C.c_int32, C.c_int32]),
    "carl_ppo_input_stats": (C.c_int, [C.POINTER(PpoBatch), C.POINTER(Policy), C.POINTER(PolicyStats), _vp]),
    "carl_brax_ppo_input_stats": (C.c_int, [C.POINTER(PpoBatch), C.POINTER(Policy), C.POINTER(PolicyStats), _vp]),
    "carl_ppo_return_stats_slabs": (C.c_int32, [C.c_int32]),
    "carl_ppo_return_stats": (C.c_int, [C.POINTER(PpoReturnStats), _vp]),
    "carl_ppo_return_merge": (C.c_int, [_vp, C.c_int32, C.c_int64, C.POINTER(PolicyRunningStats), C.c_double, _vp, _vp]),
})


# ---- PPO's minibatch step (include/carl_amd.h: carl_ppo_adv_stats_t, carl_adam_t) -----------------------------------
ADAM_MAX_TENSORS = 4


class PpoAdvStats(C.Structure):
    _fields_ = [("advantage", _vp), ("idx", _vp), ("adv_norm", _vp), ("storage_floats", C.c_int64), ("n_total", _i),
                ("batch_size", _i), ("eps", C.c_double)]


class Adam(C.Structure):
    _fields_ = [("n_tensors", _i), ("reserved", _i), ("n", C.c_int64 * ADAM_MAX_TENSORS),
                ("param", _vp * ADAM_MAX_TENSORS), ("grad", _vp * ADAM_MAX_TENSORS), ("m", _vp * ADAM_MAX_TENSORS),
                ("v", _vp * ADAM_MAX_TENSORS), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("max_grad_norm", C.c_double), ("step", _vp), ("beta_pow", _vp), ("norm_out", _vp)]


EXPORTS.update({
    "carl_ppo_adv_stats_rows": (C.c_int32, [C.c_int32, C.c_int32]),
    "carl_ppo_adv_stats": (C.c_int, [C.POINTER(PpoAdvStats), _vp]),
    "carl_adam_step_max_floats": (C.c_int64, []),
    "carl_adam_step": (C.c_int, [C.POINTER(Adam), _vp]),
})


# ---- a population of PPO learners (include/carl_amd.h: carl_ppo_sets_t, carl_ppo_grad_sets) ------------------------------
PPO_HYPER = 5
PPO_HYPER_LR, PPO_HYPER_CLIP_RANGE, PPO_HYPER_VF_COEF, PPO_HYPER_ENT_COEF, PPO_HYPER_MAX_GRAD_NORM = range(5)
PPO_HYPER_NAMES = ("lr", "clip_range", "vf_coef", "ent_coef", "max_grad_norm")  # the columns of a hyper row, in order


class PpoSets(C.Structure):
    _fields_ = [("hyper", _vp), ("idx", _vp), ("adv_norm", _vp), ("idx_set_stride", C.c_int64),
                ("adv_norm_set_stride", C.c_int64)]


EXPORTS.update({
    "carl_ppo_sets_workspace_floats": (C.c_int64, [C.POINTER(Policy), C.POINTER(Policy), C.c_int32]),
    "carl_ppo_grad_sets": (C.c_int, [C.POINTER(PpoBatch), C.POINTER(Policy), C.POINTER(Policy), _vp, C.POINTER(PpoSets),
                                     C.POINTER(PpoOut), _vp]),
    "carl_ppo_adv_stats_sets": (C.c_int, [C.POINTER(PpoAdvStats), C.c_int32, C.c_int64, _vp]),
    "carl_adam_step_sets": (C.c_int, [C.POINTER(Adam), C.c_int32, _vp, _vp]),
})
