"""One representative model per Brax kernel class, and the lane-group widths the library must list for it.

carl_brax.hip's `kBraxKernels` instantiates `brax_kernel<MODE, MULTI, K, TASK, PLANAR, F32>` per (class, width K);
`carl_brax_lane_widths(sys, flags)` lists the widths a step / rollout launch of a model can take (one lane per link or
wider), and `carl_brax_sys_t::lanes_per_env` pins one of them.  `CASES` below names, for every kernel class, a model
and batch flags that select it, and the widths it must list.  Together they reach every entry of `kBraxKernels`:
tests/test_brax_kernel_table.py holds the table against the library and its source (a kernel without a case fails
there), and tests/test_gpu_brax_kernel_matrix.py runs every (case, width) against the float64 oracle.  The second half
of this file holds the inputs of tests/test_gpu_brax_context_matrix.py: context rows that move every physics column and
every link mass through the stability clamp's regimes, under a selector that changes an env's context at each reset.

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
           "reacher": E.CARLBraxReacher, "humanoid": E.CARLBraxHumanoid,
           "back_half_cheetah_stiffness": E.CARLBraxHalfcheetahStiffness,
           "humanoid_stiffness": E.CARLBraxHumanoidStiffness}[name]
    fn = {"one_leg_ant": one_leg_ant_sys, "back_half_cheetah": back_half_cheetah_sys,
          "back_half_cheetah_stiffness": back_half_cheetah_sys}.get(name, SYSTEMS[cls.env_name])
    return fn, cls


def build(name):
    """-> (sys table, context feature names, default context row) of a model"""
    fn, cls = _model(name)
    # (the cut-down models keep the mass features of the links they keep)
    feats = {k: f for k, f in cls.get_context_features().items()
             if not (name.startswith("back_half_cheetah") and k[:6] == "mass_f")}
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


# ---- per-env context application: the inputs of tests/test_gpu_brax_context_matrix.py ----------------------------------
# (held on the host, with the float64 oracle alone, by tests/test_brax_kernel_table.py)

# the two models that declare the `joint_stiffness` column (the ...Stiffness classes' feature tables); not part of the
# kernel-instance table above: Humanoid is pinned to the width bench.py's config5_fp32 runs
STIFFNESS_CASES = [
    Case("cheetah_half_stiff", "back_half_cheetah_stiffness", 0, PLANAR, LEAN, [4, 7, 8, 9, 16]),
    Case("humanoid_stiff_f32", "humanoid_stiffness", FP32, MULTI_F32, MULTI, [11]),
]
CTX_CASES = CASES + EXTRA_CASES + STIFFNESS_CASES
CTX_N, CTX_STEPS, CTX_TIME_LIMIT, CTX_N_CTX, CTX_STRIDE = 815, 9, 4, 37, 3
# models that stand on the ground from reset on (the others have no collision spheres: elasticity and friction move nothing)
GROUND_CONTACT = {"one_leg_ant", "hopper", "back_half_cheetah", "ant", "humanoid", "back_half_cheetah_stiffness",
                  "humanoid_stiffness"}
# ranges of the physics columns: gravity and friction as the kernel matrix draws them.  None had to be narrowed: every row
# of every case stays finite and below 1e4 over the window, and the share of edge-prone lane-steps stays under a third of
# the GPU cap (worst: cheetah_half 2.7e-4 of 3.3e-4) -- test_context_matrix_rows_are_stable_and_not_edge_prone.
CTX_RANGES = {"gravity": (-15.0, -5.0), "friction": (0.3, 1.5), "elasticity": (0.0, 0.5), "ang_damping": (-0.5, 0.0),
              "joint_stiffness": (0.5, 2.0)}
LIGHT = 0.5        # regimes (c) and (d): this multiple of the feature's single floor
B_MARGIN = 0.01    # regime (b) draws from [floor + margin, 0.95]: float32 rounding must not put it under the floor


def wire_floors(sys_table, names, env_name):
    """`carl_brax_ctx_map_t::mass_ratio_floor` / `_multi` as `CARLBraxEnv.__init__` fills them (the env calls the same
    function)"""
    from carl_amd.envs.brax.models import wire_mass_floors

    wire_mass_floors(sys_table, names, env_name)


def build_clamped(case):
    """`build(case.model)` with the model's stability floors wired: (sys, names, default row)"""
    s, names, default = build(case.model)
    wire_floors(s, names, _model(case.model)[1].env_name)
    return s, names, default


def _row_plan(n_mass, n_ctx):
    """Which regime every mass feature takes in every row: a list of n_ctx dicts {feature k: "b" | "c" | "d"} (features
    not named: regime (a)).  One pass is an all-(a) row, (c) alone and (b) alone for every feature, and the (d) rows: the
    features in pairs at the end of the first pass, every feature at once after the (a) row of the later ones.  A model
    with one mass feature has no (d): two light links need two features.  The passes are laid along the order in which a
    lane visits the rows (`CTX_STRIDE` apart), so that a lane never meets the same (c) or (d) masses, which are
    constants, twice in a row."""
    seq, p = [], 0
    while len(seq) < n_ctx:
        d = [] if n_mass < 2 else [{k: "d" for k in range(n_mass)}] if p else \
            [{k: "d", (k + 1) % n_mass: "d"} for k in range(0, n_mass, 2)]
        alone = [{k: "c"} for k in range(n_mass)] + [{k: "b"} for k in range(n_mass)]
        seq += [{}] + (d + alone if p else alone + d)
        assert len(seq) <= n_ctx or p > 0, "too few rows for every feature to see every regime"
        p += 1
    plan = [None] * n_ctx
    for j in range(n_ctx):
        plan[(CTX_STRIDE * j) % n_ctx] = seq[j]
    assert None not in plan
    return plan


def context_matrix_rows(case, rng, n_ctx):
    """float32-exact context rows [n_ctx, F] that vary every physics column the case's model declares (CTX_RANGES; goal
    columns at their defaults) and take every `mass_<link>` column through the clamp's four regimes (`_row_plan`):
    (a) ratio U(1, 3); (b) ratio in [floor, 0.95], the env's only light link; (c) 0.5 x floor, alone: the single floor;
    (d) two or more links at 0.5 x their floor: the combined floor.  Every feature sees each regime in at least two rows
    where 37 rows allow it: a feature is alone in its (b) and (c) rows, so Humanoid's eleven features need 29 rows for one
    pass -- there every feature has (a) and (d) twice, six of them (c) twice, and (b) comes once."""
    s, names, default = build_clamped(case)
    cm = s.ctx
    rows = np.tile(default, (n_ctx, 1))
    for name, (lo, hi) in CTX_RANGES.items():
        if name in names:
            rows[:, names.index(name)] = rng.uniform(lo, hi, n_ctx)
    for r, regimes in enumerate(_row_plan(cm.n_mass, n_ctx)):
        for k in range(cm.n_mass):
            floor = float(cm.mass_ratio_floor[k])
            ratio = {"a": rng.uniform(1.0, 3.0), "b": rng.uniform(floor + B_MARGIN, 0.95), "c": LIGHT * floor,
                     "d": LIGHT * floor}[regimes.get(k, "a")]
            rows[r, cm.mass_row[k]] = ratio * float(cm.mass_nominal[k])
    return rows.astype(np.float32).astype(np.float64)


def mass_ratios(s, rows):
    """-> (sampled ratio, effective ratio, n_light) per (row, mass feature), by `load_ctx`'s rule in float32"""
    cm = s.ctx
    K = range(cm.n_mass)
    ratio = np.stack([rows[:, cm.mass_row[k]].astype(np.float32) / np.float32(cm.mass_nominal[k]) for k in K], axis=1)
    n_light = (ratio < np.float32(0.999)).sum(1)
    single = np.array([cm.mass_ratio_floor[k] for k in K], np.float32)
    multi = np.array([cm.mass_ratio_floor_multi[k] for k in K], np.float32)
    return ratio, np.maximum(ratio, np.where(n_light[:, None] >= 2, multi, single)), n_light


def mass_regimes(s, rows):
    """The regime of every (row, mass feature), read off the rows alone: [n_ctx, n_mass] of "a" / "b" / "c" / "d" ("-":
    none of them)"""
    cm = s.ctx
    ratio, _, n_light = mass_ratios(s, rows)
    out = np.full(ratio.shape, "-", dtype="<U1")
    for k in range(cm.n_mass):
        floor = np.float32(cm.mass_ratio_floor[k])
        r = ratio[:, k]
        out[r >= 1.0, k] = "a"
        out[(r >= floor) & (r <= np.float32(0.95)) & (n_light == 1), k] = "b"
        out[(r < floor) & (n_light == 1), k] = "c"
        out[(r < floor) & (n_light >= 2), k] = "d"
    return out


def touch_down(s, st):
    """Lower every even env of a model that stands on the ground until its lowest collision sphere is 5 mm deep; `st` is
    the float64 state [N, L, 13] (position 3, rotation (w, x, y, z), velocities), changed in place.  Hopper and Humanoid
    start above the ground and need longer than a TimeLimit of 4 to reach it; this puts the contact path into the window
    (the odd envs keep their reset pose, and the envs that auto-reset start from the reset pose)."""
    link = np.array(s.coll_link[: s.n_coll])
    # a sphere's offset from its link's centre of mass, in the link frame (the state holds the COM)
    off = np.array([[s.coll_pos[k][j] - s.com[s.coll_link[k]][j] for j in range(3)] for k in range(s.n_coll)], np.float64)
    rad = np.array(s.coll_radius[: s.n_coll], np.float64)
    p, q = st[:, link, :3], st[:, link, 3:7]
    w, u = q[..., 0], q[..., 1:]  # sphere centre = p + R off, R off = off + 2 w (u x off) + 2 u x (u x off)
    uxo = np.cross(u, np.broadcast_to(off, u.shape))
    z = p[..., 2] + off[:, 2] + 2 * (w * uxo[..., 2] + np.cross(u, uxo)[..., 2])
    gap = (z - rad).min(1) - float(s.plane_z)  # [N]: height of the lowest sphere's bottom above the ground
    st[0::2, :, 2] -= (gap[0::2] + 0.005)[:, None]
    return st


class CtxInputs:
    """What one case of the context matrix runs on, the same on the host and on the GPU, at every width"""

    def __init__(self, case, n=CTX_N, steps=CTX_STEPS, time_limit=CTX_TIME_LIMIT, seed_base=4000):
        from oracle import oracle as O

        self.case, self.n, self.steps, self.time_limit = case, n, steps, time_limit
        self.seed = seed_base + 100 * CTX_CASES.index(case)
        rng = np.random.default_rng(self.seed)
        self.sys, self.names, self.default = build_clamped(case)
        self.rows = context_matrix_rows(case, rng, CTX_N_CTX)
        s = self.sys
        self.lo, self.hi = float(min(s.act_lo[: s.n_act])), float(max(s.act_hi[: s.n_act]))
        self.acts = rng.uniform(self.lo, self.hi, (steps, n, s.n_act)).astype(np.float32)
        self.selector = dict(selector=O.SEL_ROUND_ROBIN, selector_stride=CTX_STRIDE, seed=self.seed)
        self.touch = case.model in GROUND_CONTACT

    def pinned(self, width):
        """a copy of the model table pinned to `width` lanes per env"""
        s = type(self.sys).from_buffer_copy(self.sys)
        s.lanes_per_env = width
        return s

    def oracle(self, sys_table=None, rows=None):
        from oracle import brax as B

        return B.Engine(self.sys if sys_table is None else sys_table, self.rows if rows is None else rows, self.n,
                        max_steps=self.time_limit, **self.selector)


_INPUTS = {}


def ctx_inputs(case):
    if case.label not in _INPUTS:
        _INPUTS[case.label] = CtxInputs(case)
    return _INPUTS[case.label]


# ---- the float64 oracle alone on those inputs (host checks) ------------------------------------------------------------
_BOOK = ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done", "goal_pos", "last_return",
         "last_length", "obs")


def snapshot(ora):
    return {k: getattr(ora, k).copy() for k in _BOOK}


def restep(inp, snap, action, *, sys_table=None, rows=None, state=None, ctx_idx=None):
    """One oracle step from a snapshot, with the model table, context rows, start state or context index replaced.
    -> (per-lane observation (the terminal one on a done step) [N, D], reward, terminated, contact hash, engine)"""
    ora = inp.oracle(sys_table, rows)
    for k, v in snap.items():
        getattr(ora, k)[...] = v
    if state is not None:
        ora.state[...] = state
    if ctx_idx is not None:
        ora.ctx_idx[...] = ctx_idx
    out = ora.step(action)
    done = (out.terminated != 0) | (out.truncated != 0)
    return np.where(done[:, None], out.final_obs, out.obs), out.reward, out.terminated != 0, ora.branch_sig[:, 0].copy(), ora


def oracle_trajectory(inp, touched, rows=None):
    """The window of the GPU tests on the oracle alone: reset (and the touched-down start where `touched`), then
    `inp.steps` steps.  -> list of (snapshot before the step, action, obs (the terminal one on a done step), reward,
    terminated, contact hash, ctx_idx after the step, done)"""
    ora = inp.oracle(rows=rows)
    ora.reset()
    if touched:
        L = inp.sys.n_links
        ora.state[...] = touch_down(inp.sys, ora.state.reshape(inp.n, L, 13).copy()).reshape(inp.n, -1)
    traj = []
    for t in range(inp.steps):
        snap = snapshot(ora)
        out = ora.step(inp.acts[t])
        done = (out.terminated != 0) | (out.truncated != 0)
        traj.append((snap, inp.acts[t], np.where(done[:, None], out.final_obs, out.obs), out.reward, out.terminated != 0,
                     ora.branch_sig[:, 0].copy(), ora.ctx_idx.copy(), done))
    return traj


def moved(obs_a, rew_a, obs_b, rew_b):
    """per-lane distance of two transitions, in the measure of tests/brax_parity_util.py: rel_err"""
    def rel(got, want):
        return np.abs(np.float64(got) - np.float64(want)) / (1.0 + np.abs(np.float64(want)))
    return np.maximum(rel(obs_a, obs_b).max(1), rel(rew_a, rew_b))


# ---- bars of the GPU comparison on these inputs ---------------------------------------------------------------------------
F64_BAR = (1e-5, None, 1e-3)   # (max, p99, excluded share): north_star's, as tests/test_gpu_brax_kernel_matrix.py holds them
F32_BAR = (2e-4, 1e-4, 5e-3)   # measured on nominal masses (profiles/r06_brax_fp32_deviation.txt)
# Float32 allowance on clamped-light links, from the oracle alone: the oracle's one-step output deviation caused by
# rounding its start state to float32, over the window of the GPU test (the touched-down start where the model stands on
# the ground; lane-steps whose contact hash and `terminated` agree), on the rows above and on the same rows with every
# mass ratio set to 1.  R = (new rows) / (nominal masses) at (p99, max); the GPU bars on these inputs are the existing
# ones x max(1, R).  tests/test_brax_kernel_table.py measures R again and holds these constants to it within 20 %.
F32_LIGHT_MASS_AMPLIFICATION = {
    "lean_f32": (1.01, 1.27), "planar_f32": (1.12, 1.32), "multi_f32": (0.91, 0.78), "generic_f32": (1.08, 1.21),
    "cheetah_half_f32": (0.97, 0.95), "ant_f32": (0.99, 0.83), "humanoid_f32": (1.28, 1.44),
    "humanoid_stiff_f32": (1.37, 1.43),
}


def ctx_bars(case):
    """-> (max, p99 or None, excluded share) the GPU comparison holds `case` to on the context-matrix inputs"""
    if not case.flags & FP32:
        return F64_BAR
    r99, rmax = F32_LIGHT_MASS_AMPLIFICATION[case.label]
    return F32_BAR[0] * max(1.0, rmax), F32_BAR[1] * max(1.0, r99), F32_BAR[2]


def f32_start_deviation(inp, rows):
    """The oracle stepped once from every state of the window and once from the same state rounded to float32, on context
    rows `rows`: -> (p99, max of the deviation over the agreeing lane-steps, share of lane-steps whose contact hash or
    `terminated` differs)"""
    dev, edge = [], 0
    for snap, act, obs, rew, term, sig, _, _ in oracle_trajectory(inp, inp.touch, rows):
        o, r, te, h, _ = restep(inp, snap, act, rows=rows, state=snap["state"].astype(np.float32).astype(np.float64))
        agree = (h == sig) & (te == term)
        edge += int((~agree).sum())
        dev.append(moved(o, r, obs, rew)[agree])
    dev = np.concatenate(dev)
    return float(np.percentile(dev, 99)), float(dev.max()), edge / (inp.n * inp.steps)


def nominal_mass_rows(inp):
    """the case's rows with every mass ratio set to 1"""
    cm, rows = inp.sys.ctx, inp.rows.copy()
    for k in range(cm.n_mass):
        rows[:, cm.mass_row[k]] = np.float32(cm.mass_nominal[k])
    return rows
