"""Inputs of the Brax closed-loop rollout tests (test_brax_policy_abi.py on the host, test_gpu_brax_policy.py on the GPU):
the models, derived the way brax_kernel_cases.py derives its cases -- a model table, its batch flags, and every lane width
`carl_brax_lane_widths` lists for it -- the three network shapes, and the host reference of a policy with up to
CARL_BRAX_MAX_ACT outputs.  A plain module: importing it allocates nothing and touches no device."""
import ctypes as C

import numpy as np

from brax_kernel_cases import lane_widths, one_leg_ant_sys
from carl_amd import _lib

# kernel class (multi, task, planar) of each model's step launch, as carl_brax.hip's BraxClass spells it without f32.
# One shipped model per class and more, plus the cut-down Ant and the inverted pendulum: the only models narrow enough for
# the lean widths 4, 7, 8 and the multi-hinge width 2.
MODELS = {
    "ant": (False, False, False), "one_leg_ant": (False, False, False), "halfcheetah": (False, False, True),
    "hopper": (False, False, True), "inverted_double_pendulum": (True, False, False),
    "inverted_pendulum": (True, False, False), "reacher": (True, True, False),
}
GROUND = {"ant", "one_leg_ant", "halfcheetah", "hopper"}  # models that stand on the ground from reset on
# (hidden widths, activation): 2 x 64 tanh, 1 x 32 relu, a linear identity network
NETWORKS = [((64, 64), "tanh"), ((32,), "relu"), ((), "identity")]


def build_model(name):
    """-> (sys table, context feature names, default context row)"""
    from carl_amd import envs as E
    from carl_amd.envs.brax.models import SYSTEMS

    cls = {"ant": E.CARLBraxAnt, "one_leg_ant": E.CARLBraxAnt, "halfcheetah": E.CARLBraxHalfcheetah,
           "hopper": E.CARLBraxHopper, "inverted_double_pendulum": E.CARLBraxInvertedDoublePendulum,
           "inverted_pendulum": E.CARLBraxInvertedPendulum, "reacher": E.CARLBraxReacher,
           "humanoid": E.CARLBraxHumanoid}[name]
    feats = cls.get_context_features()
    names = list(feats)
    fn = one_leg_ant_sys if name == "one_leg_ant" else SYSTEMS[cls.env_name]
    return fn(names), names, np.array([float(f.default_value) for f in feats.values()])


def model_widths(name):
    return lane_widths(build_model(name)[0], 0)


def instance_cases():
    """every (model, width) of MODELS: together every instantiated (class, width) of the closed-loop kernels"""
    return [(m, w) for m in MODELS for w in model_widths(m)]


def context_rows(rng, n_ctx, default, names):
    rows = np.tile(default, (n_ctx, 1))
    rows[:, names.index("gravity")] = rng.uniform(-15, -5, n_ctx)
    rows[:, names.index("friction")] = rng.uniform(0.3, 1.5, n_ctx)
    return rows.astype(np.float32).astype(np.float64)


def make_layers(rng, n_in, widths, n_out, gain=0.5):
    """random (W, b) per layer; the head scaled so that the actions spread over the actuators' [-1, 1] and beyond"""
    dims = [n_in, *widths, n_out]
    layers = []
    for k, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        scale = gain if k == len(dims) - 2 else 1.0 / np.sqrt(i)
        layers.append(((rng.normal(size=(o, i)) * scale).astype(np.float32), (rng.normal(size=o) * 0.1).astype(np.float32)))
    return layers


def transform(rng, n_in):
    """(shift, scale, clip): a VecNormalize-like input transform that is not the identity"""
    return (rng.normal(size=n_in) * 0.1).astype(np.float32), rng.uniform(0.5, 1.5, n_in).astype(np.float32), 5.0


def pack(layers, shift, scale, clip):
    """one packed weight set (include/carl_amd.h), written out independently of carl_amd.policy"""
    parts = []
    for W, b in layers:
        parts += [np.asarray(W, np.float32).reshape(-1), np.asarray(b, np.float32)]
    parts += [np.asarray(shift, np.float32), np.asarray(scale, np.float32), np.array([clip], np.float32)]
    flat = np.concatenate(parts)
    return np.concatenate([flat, np.zeros((-flat.size) % 4, np.float32)])


def reference_actions(pol, x, sets=None):
    """oracle.policy_forward of a policy with any head width on inputs x [M, n_in]; sets [M]: each row's weight set.
    The oracle takes at most 4 outputs: the head is evaluated in row slices of at most 4, each slice packed as a policy
    of its own (the same hidden layers and transform).  -> (y32, y64, bound), each [M, n_out]"""
    from oracle import oracle as O

    n_sets = pol.params.shape[0]
    per_set = []
    for k in range(n_sets):  # the layers of set k, read back from its packed block
        flat, off, layers = pol.params[k], 0, []
        for W, b in pol.layers:
            layers.append((flat[off: off + W.size].reshape(W.shape), flat[off + W.size: off + W.size + b.size]))
            off += W.size + b.size
        n = pol.n_in
        per_set.append((layers, flat[off: off + n], flat[off + n: off + 2 * n], flat[off + 2 * n]))
    outs = []
    for lo in range(0, pol.n_out, 4):
        hi = min(lo + 4, pol.n_out)
        params = np.stack([pack(L[:-1] + [(L[-1][0][lo:hi], L[-1][1][lo:hi])], sh, sc, cl) for L, sh, sc, cl in per_set])
        outs.append(O.policy_forward(params, pol.n_in, pol.widths, hi - lo, pol.activation, x, sets))
    return tuple(np.concatenate([getattr(r, f) for r in outs], axis=1) for f in ("y32", "y64", "bound"))


def launch_shape(batch, sys_table, policy_struct, n_steps):
    out = _lib.BraxLaunchShape()
    code = _lib.load().carl_brax_policy_launch_shape(C.byref(batch), C.byref(sys_table), C.byref(policy_struct), n_steps,
                                                     C.byref(out))
    return code, out


def open_launch_shape(batch, sys_table, step, n_steps):
    """the shape of the carl_brax_reset (step False) or carl_brax_step / carl_brax_rollout launch of this batch"""
    out = _lib.BraxLaunchShape()
    code = _lib.load().carl_brax_launch_shape(C.byref(batch), C.byref(sys_table), int(step), n_steps, C.byref(out))
    return code, out


def fragments(shape, n_lanes, n_steps):
    """every fragment of the launch `shape` as (workgroup, wave, group, t_lo, t_hi, wait_head, signal_head)"""
    lib = _lib.load()
    n_groups = -(-n_lanes // (64 // shape.lanes_per_env))
    buf = (C.c_int32 * (5 * 64))()
    frags = []
    for wg in range(min(shape.grid, n_groups)):
        for wave in range(shape.waves_per_workgroup):
            k = lib.carl_brax_fragment_plan(n_groups, shape.grid, shape.waves_per_workgroup, n_steps, wg, wave, buf, 64)
            assert 0 <= k <= 64
            frags += [(wg, wave, *buf[5 * i: 5 * i + 5]) for i in range(k)]
    return frags
