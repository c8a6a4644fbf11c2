"""One representative model per Brax kernel class, and the lane-group widths the library must list for it.

carl_brax.hip's `kBraxKernels` instantiates `brax_kernel<MODE, MULTI, K, TASK, PLANAR, F32>` per (class, width K);
`carl_brax_lane_widths(sys, flags)` lists the widths a step / rollout launch of a model can take (one lane per link or
wider), and `carl_brax_sys_t::lanes_per_env` pins one of them.  `CASES` below names, for every kernel class, a model
and batch flags that select it, and the widths it must list.  Together they reach every entry of `kBraxKernels`:
tests/test_brax_kernel_table.py holds the table against the library and its source (a kernel without a case fails
there), and tests/test_gpu_brax_kernel_matrix.py runs every (case, width) against the float64 oracle.

Reset never takes the planar substep or the float32 pose algebra (carl_brax.hip: brax_class), so the reset kernels
follow from the same cases: Hopper resets through the lean kernels, every float32 case through its float64 class.

The lean class has one shipped model, Ant, whose 9 links put its narrowest width at 9; `one_leg_ant_sys` keeps the
torso and the first leg (3 links), which reaches the lean widths 4, 7 and 8 too.
"""
import numpy as np

from carl_amd import _lib

FP32, GENERIC = _lib.FLAG_BRAX_FP32, _lib.FLAG_BRAX_GENERIC

# kernel class as carl_brax.hip's BraxClass spells it: (multi, task, planar, f32)
LEAN, MULTI, TASK, PLANAR = (False, False, False, False), (True, False, False, False), (True, True, False, False), \
    (False, False, True, False)
LEAN_F32, MULTI_F32, PLANAR_F32 = (False, False, False, True), (True, False, False, True), (False, False, True, True)


def one_leg_ant_sys(feature_names=None):
    """Ant cut down to the torso (free root) and its first leg (hip and ankle hinges): 3 links, q 9, qd 8, 2 motors,
    obs 15.  The collision spheres kept are the torso's, the far end of the first aux capsule, and the two ends of the
    hip and of the ankle capsule -- the first six of ant_sys's list.  A lean model (free root, single hinges), not
    planar."""
    from carl_amd.envs.brax.models import ant_sys

    s = ant_sys(feature_names)
    s.n_links, s.n_q, s.n_dof, s.n_act, s.obs_dim = 3, 9, 8, 2, 15
    s.act_dof[0], s.act_dof[1] = 6, 7  # hip_1, ankle_1 (ant_sys drives hip_4 / ankle_4 first)
    s.n_coll = 6
    return s


def back_half_cheetah_sys(feature_names=None):
    """Halfcheetah cut down to the torso (root on two slides and a hinge) and its back leg (thigh, shin, foot): 4 links,
    q 6, qd 6, 3 motors, obs 11, the torso's and the back leg's ten collision spheres.  A planar model whose joint
    anchors sit off their parent's z axis: Hopper's do not (a vertical chain), so there the planar substep's x-offset
    terms multiply zeros."""
    from carl_amd.envs.brax.models import halfcheetah_sys

    s = halfcheetah_sys(feature_names)
    s.n_links, s.n_q, s.n_dof, s.n_act, s.obs_dim = 4, 6, 6, 3, 11
    s.n_coll = 10
    return s


def _model(name):
    """(sys table builder, CARL class) of a model name"""
    from carl_amd import envs as E
    from carl_amd.envs.brax.models import SYSTEMS

    cls = {"one_leg_ant": E.CARLBraxAnt, "ant": E.CARLBraxAnt, "hopper": E.CARLBraxHopper,
           "back_half_cheetah": E.CARLBraxHalfcheetah, "inverted_pendulum": E.CARLBraxInvertedPendulum,
           "reacher": E.CARLBraxReacher, "humanoid": E.CARLBraxHumanoid}[name]
    fn = {"one_leg_ant": one_leg_ant_sys, "back_half_cheetah": back_half_cheetah_sys}.get(name, SYSTEMS[cls.env_name])
    return fn, cls


def build(name):
    """-> (sys table, context feature names, default context row) of a model"""
    fn, cls = _model(name)
    # (the cut-down models keep the mass features of the links they keep)
    feats = {k: f for k, f in cls.get_context_features().items() if not (name == "back_half_cheetah" and k[:6] == "mass_f")}
    names = list(feats)
    return fn(names), names, np.array([float(f.default_value) for f in feats.values()])


class Case:
    def __init__(self, label, model, flags, step_class, reset_class, widths):
        self.label, self.model, self.flags = label, model, flags
        self.step_class, self.reset_class, self.widths = step_class, reset_class, list(widths)

    def __repr__(self):
        return self.label


# label, model, batch flags, step kernel class, reset kernel class, widths carl_brax_lane_widths must list
CASES = [
    Case("lean", "one_leg_ant", 0, LEAN, LEAN, [4, 7, 8, 9, 16]),
    Case("planar", "hopper", 0, PLANAR, LEAN, [4, 7, 8, 9, 16]),
    Case("multi", "inverted_pendulum", 0, MULTI, MULTI, [2, 11, 16]),
    Case("task", "reacher", 0, TASK, TASK, [4, 8, 16]),
    Case("lean_f32", "one_leg_ant", FP32, LEAN_F32, LEAN, [4, 7, 8, 9, 16]),
    Case("planar_f32", "hopper", FP32, PLANAR_F32, LEAN, [4, 7, 8, 9, 16]),
    Case("multi_f32", "inverted_pendulum", FP32, MULTI_F32, MULTI, [2, 11, 16]),
    Case("generic_f32", "hopper", GENERIC | FP32, MULTI_F32, LEAN, [11, 16]),
]

# beside the representatives: the planar kernels again on a model with horizontal joint offsets, and the float32 shapes
# bench.py times (also.config4_fp32: Ant at 9 lanes per env; config5_fp32: Humanoid at 11)
EXTRA_CASES = [
    Case("cheetah_half", "back_half_cheetah", 0, PLANAR, LEAN, [4, 7, 8, 9, 16]),
    Case("cheetah_half_f32", "back_half_cheetah", FP32, PLANAR_F32, LEAN, [4, 7, 8, 9, 16]),
    Case("ant_f32", "ant", FP32, LEAN_F32, LEAN, [9, 16]),
    Case("humanoid_f32", "humanoid", FP32, MULTI_F32, MULTI, [11, 16]),
]


def lane_widths(sys_table, flags):
    import ctypes as C

    out = (C.c_int32 * 16)()
    n = _lib.load().carl_brax_lane_widths(C.byref(sys_table), int(flags), out, 16)
    return [int(out[i]) for i in range(n)]
