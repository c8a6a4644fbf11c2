"""Model tables (``carl_brax_sys_t``) of the Brax locomotion systems CARL wraps.

The reference loads these with ``brax.io.mjcf.load`` from XML assets shipped INSIDE the brax
wheel (``envs/assets/ant.xml`` ...; carl/envs/brax/carl_ant.py:16) -- neither brax nor its
assets are in the reference tree or installable here, so geometry, joint ranges, gears and
the spring-backend constants below are restated from upstream memory [upstream-memory] of
brax 0.12.1's ``ant.xml`` (a Gym-Ant derivative with brax ``<custom>`` numerics) and
``brax/envs/ant.py``.  PARITY UNPINNED against brax itself.

Spring backend conventions restated here: ``spring_mass_scale = spring_inertia_scale = 1``
in the asset, i.e. the pipeline runs every link with effective mass ``m**(1-1) = 1`` and
identity inertia (what keeps its stiff joint springs stable at dt = 0.005).  Hence upstream a
``mass_<link>`` context would NOT move the spring dynamics even with the reference's Quirk B1
fixed; scaling the effective mass RELATIVE to CARL's default (``mass_torso`` 10 -> factor 1) is an
EXTENSION of this build (north_star asks for per-instance mass), like ``joint_stiffness`` --
clamped per env at the measured stability floor (``carl_brax_ctx_map_t::mass_ratio_floor``).
"""
from __future__ import annotations

import math

import numpy as np

from carl_amd import _lib
from carl_amd.envs.brax.feature_tables import (COMBINED_FLOOR_SCALE, DEFAULT_MASS_RATIO_FLOOR, MASS_RATIO_FLOOR,
                                               masses)


def _axis_quat(axis) -> tuple[float, float, float, float]:
    """shortest-arc rotation taking e_x onto ``axis`` (the joint frame's x axis is the hinge)"""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    d = float(u[0])
    if d < -1 + 1e-12:
        return (0.0, 0.0, 0.0, 1.0)
    c = np.cross([1.0, 0.0, 0.0], u)
    q = np.array([1.0 + d, c[0], c[1], c[2]])
    q /= np.linalg.norm(q)
    return tuple(float(x) for x in q)


def _set3(dst, i, v):
    for k in range(len(v)):
        dst[i][k] = float(v[k])


def ant_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """Ant: torso (free root) + 4 x (hip link, ankle link); q 15, qd 14, 8 motors, obs 27.

    ``feature_names``: the CARL class's context-feature order, to wire context columns to
    physics parameters (carl/envs/brax/carl_brax_env.py:255-292 in its intended form);
    ``reference_compat=True`` leaves every physics parameter at the asset's value, which is
    what the reference effectively simulates (SURVEY.md Quirk B1)."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_ANT
    s.healthy_q_index = -1
    s.n_links, s.n_q, s.n_dof, s.n_act = 9, 15, 14, 8
    s.n_frames, s.obs_dim = 10, 27
    s.max_episode_steps = 1000
    s.terminate_when_unhealthy = 1
    s.exclude_current_positions = 2  # obs = q[2:] ++ qd
    s.dt = 0.005
    s.gravity_z, s.vel_damping, s.ang_damping = -9.81, 0.0, 0.0
    s.baumgarte_erp, s.elasticity, s.friction = 0.1, 0.0, 1.0
    s.healthy_z_lo, s.healthy_z_hi, s.healthy_reward = 0.2, 1.0, 1.0
    s.ctrl_cost_weight, s.forward_reward_weight = 0.5, 1.0
    s.reset_noise_scale, s.reset_vel_scale = 0.1, 0.1

    ident = (1.0, 0.0, 0.0, 0.0)
    dirs = [(1, 1), (-1, 1), (-1, -1), (1, -1)]
    ankle_axis = [(-1, 1, 0), (1, 1, 0), (-1, 1, 0), (1, 1, 0)]
    ankle_range = [(30, 70), (-70, -30), (-70, -30), (30, 70)]
    # link 0: torso
    s.parent[0], s.n_link_dof[0], s.q_start[0], s.dof_start[0] = -1, 6, 0, 0
    _set3(s.link_rot, 0, ident)
    _set3(s.joint_rot, 0, ident)
    coll = [(0, (0.0, 0.0, 0.0), 0.25)]
    li, qi, di = 1, 7, 6
    joint_dof = {}
    for k, (dx, dy) in enumerate(dirs):
        coll.append((0, (0.2 * dx, 0.2 * dy, 0.0), 0.08))  # far end of the aux capsule on the torso
        hip = li
        s.parent[hip], s.n_link_dof[hip], s.q_start[hip], s.dof_start[hip] = 0, 1, qi, di
        _set3(s.link_pos, hip, (0.2 * dx, 0.2 * dy, 0.0))
        _set3(s.link_rot, hip, ident)
        _set3(s.joint_rot, hip, _axis_quat((0, 0, 1)))
        _set3(s.com, hip, (0.1 * dx, 0.1 * dy, 0.0))
        s.dof_lo[di], s.dof_hi[di] = math.radians(-30), math.radians(30)
        joint_dof[f"hip_{k + 1}"] = di
        coll += [(hip, (0.0, 0.0, 0.0), 0.08), (hip, (0.2 * dx, 0.2 * dy, 0.0), 0.08)]
        ank = li + 1
        s.parent[ank], s.n_link_dof[ank], s.q_start[ank], s.dof_start[ank] = hip, 1, qi + 1, di + 1
        _set3(s.link_pos, ank, (0.2 * dx, 0.2 * dy, 0.0))
        _set3(s.link_rot, ank, ident)
        _set3(s.joint_rot, ank, _axis_quat(ankle_axis[k]))
        _set3(s.com, ank, (0.2 * dx, 0.2 * dy, 0.0))
        lo, hi = ankle_range[k]
        s.dof_lo[di + 1], s.dof_hi[di + 1] = math.radians(lo), math.radians(hi)
        joint_dof[f"ankle_{k + 1}"] = di + 1
        coll += [(ank, (0.0, 0.0, 0.0), 0.08), (ank, (0.4 * dx, 0.4 * dy, 0.0), 0.08)]
        li, qi, di = li + 2, qi + 2, di + 2
    for i in range(s.n_links):
        s.mass[i] = 1.0          # m ** (1 - spring_mass_scale), spring_mass_scale = 1
        _set3(s.inv_inertia, i, (1.0, 1.0, 1.0))
        s.k_pos[i], s.k_vel[i], s.k_limit[i], s.k_ang_damp[i] = 4000.0, 20.0, 1000.0, 10.0
    for d in range(6, s.n_dof):
        s.dof_damping[d], s.dof_stiffness[d] = 1.0, 0.0
    for k, name in enumerate(["hip_4", "ankle_4", "hip_1", "ankle_1", "hip_2", "ankle_2", "hip_3", "ankle_3"]):
        s.act_dof[k], s.act_gear[k], s.act_lo[k], s.act_hi[k] = joint_dof[name], 150.0, -1.0, 1.0
    s.n_coll = len(coll)
    for k, (link, pos, rad) in enumerate(coll):
        s.coll_link[k], s.coll_radius[k] = link, rad
        _set3(s.coll_pos, k, pos)
    init_q = [0.0, 0.0, 0.55, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0, -1.0, 0.0, 1.0]
    for i, v in enumerate(init_q):
        s.init_q[i] = v
    _wire_context(s, feature_names, reference_compat, {"torso": 0}, {"mass_torso": 10.0})
    # goal mode constants: STATE_INDICES["ant"] (brax_walker_goal_wrapper.py:7) and the raw MJCF
    # `opt.timestep` of ant.xml the wrapper integrates with (:109-111, Quirk B3)
    s.goal_obs_idx[0], s.goal_obs_idx[1], s.goal_dt = 13, 14, 0.01
    return s


def _wire_context(s, feature_names, reference_compat, link_ids, mass_defaults):
    m = s.ctx
    m.gravity = m.friction = m.elasticity = m.ang_damping = m.joint_stiffness_scale = -1
    m.target_distance = m.target_direction = m.target_radius = -1
    m.n_mass = 0
    for k in range(3):
        m.goal_position[k] = -1
    if not feature_names:
        return
    col = {n: i for i, n in enumerate(feature_names)}
    # goal features are read by the goal-reward epilogue whatever the physics mode
    m.target_distance = col.get("target_distance", -1)
    m.target_direction = col.get("target_direction", -1)
    m.target_radius = col.get("target_radius", -1)
    if reference_compat:
        return
    m.gravity = col.get("gravity", -1)
    m.friction = col.get("friction", -1)
    m.elasticity = col.get("elasticity", -1)
    m.ang_damping = col.get("ang_damping", -1)
    m.joint_stiffness_scale = col.get("joint_stiffness", -1)
    for k, axis in enumerate("xyz"):  # push task (carl_pusher.py:91-103 hands them to the env as its goal)
        m.goal_position[k] = col.get(f"goal_position_{axis}", -1)
    for name, i in col.items():
        if name.startswith("mass_"):
            link = name.split("_", 1)[-1]
            if link not in link_ids:
                # same failure as the reference's _set_masses (carl_brax_env.py:70-73)
                raise RuntimeError(
                    f"Link {link} not in available link names {list(link_ids)}. Probably "
                    "something went wrong during context creation.")
            k = m.n_mass
            m.mass_row[k], m.mass_link[k], m.mass_nominal[k] = i, link_ids[link], float(mass_defaults[name])
            m.n_mass = k + 1


def wire_mass_floors(s, feature_names, env_name: str) -> None:
    """The per-env clamp of the effective mass ratio (``carl_brax_ctx_map_t::mass_ratio_floor`` / ``_multi``): every mass
    feature's measured single floor (``feature_tables.MASS_RATIO_FLOOR``; ``DEFAULT_MASS_RATIO_FLOOR`` where none was
    measured), and for an env with two or more light links that floor times the family's ``COMBINED_FLOOR_SCALE``, capped
    at the default mass."""
    floors = MASS_RATIO_FLOOR.get(env_name, {})
    scale = COMBINED_FLOOR_SCALE.get(env_name, 2.0)
    cm = s.ctx
    for k in range(cm.n_mass):
        cm.mass_ratio_floor[k] = floors.get(feature_names[cm.mass_row[k]], DEFAULT_MASS_RATIO_FLOOR)
        cm.mass_ratio_floor_multi[k] = min(1.0, scale * cm.mass_ratio_floor[k])


def apply_viscosity_rule(s, feature_names, rule: str) -> None:
    """What the ``viscosity`` context does to the physics.  ``"observed"`` (default): nothing -- it only appears in
    ``obs["context"]`` (Quirk B2: its intended semantics are unclear; fluid forces are not modelled).  ``"reference"``:
    the LITERAL rule of the reference's ``_update_context`` -- ``sys.replace(ang_damping=context["viscosity"])`` AFTER
    the ``ang_damping`` line (carl/envs/brax/carl_brax_env.py:276-279), i.e. the viscosity column is what the angular
    damping reads and the ``ang_damping`` column is overwritten.  (In the reference itself neither reaches the jitted
    step: Quirk B1.)"""
    if rule not in ("observed", "reference"):
        raise ValueError("viscosity rule must be 'observed' or 'reference'")
    if rule == "reference" and feature_names and "viscosity" in feature_names and s.ctx.ang_damping >= 0:
        s.ctx.ang_damping = list(feature_names).index("viscosity")


def _capsule_ends(pos, theta_y, half):
    """ends of a capsule given MJCF `pos`, `axisangle="0 1 0 theta"` and half-length (local z axis)"""
    d = np.array([math.sin(theta_y), 0.0, math.cos(theta_y)])
    p = np.asarray(pos, dtype=np.float64)
    return p - half * d, p + half * d


def halfcheetah_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """Halfcheetah: planar torso (slide x, slide z, hinge y against the world) + 6 hinge links;
    q 9, qd 9, 6 motors, obs 17 (q[1:] ++ qd).  Geometry, joint ranges / stiffness / damping
    and gears restated from upstream memory of brax's ``half_cheetah.xml`` (a Gym HalfCheetah
    derivative) and ``brax/envs/half_cheetah.py`` (spring backend: dt 0.003125 x 16 frames);
    the spring-constraint constants are this build's choice (CARL's legacy docs list
    joint_stiffness 15000 for Halfcheetah).  PARITY UNPINNED."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_HALFCHEETAH
    s.healthy_q_index = -1
    s.n_links, s.n_q, s.n_dof, s.n_act = 7, 9, 9, 6
    s.n_frames, s.obs_dim = 16, 17
    s.max_episode_steps = 1000
    s.terminate_when_unhealthy = 0
    s.exclude_current_positions = 1
    s.dt = 0.003125
    s.gravity_z, s.vel_damping, s.ang_damping = -9.81, 0.0, 0.0
    s.baumgarte_erp, s.elasticity, s.friction = 0.1, 0.0, 0.4
    s.healthy_z_lo, s.healthy_z_hi, s.healthy_reward = -1e9, 1e9, 0.0
    s.ctrl_cost_weight, s.forward_reward_weight = 0.1, 1.0
    s.reset_noise_scale, s.reset_vel_scale = 0.1, 0.1
    ident = (1.0, 0.0, 0.0, 0.0)
    hinge_y = _axis_quat((0, 1, 0))
    r = 0.046
    # (name, parent, body pos, range, stiffness, damping, geoms[(pos, theta, half)])
    links = [
        ("torso", -1, (0.0, 0.0, 0.7), None, 0.0, 0.0, [((0.0, 0, 0.0), math.pi / 2, 0.5), ((0.6, 0, 0.1), 0.87, 0.15)]),
        ("bthigh", 0, (-0.5, 0, 0), (-0.52, 1.05), 240.0, 6.0, [((0.1, 0, -0.13), -3.8, 0.145)]),
        ("bshin", 1, (0.16, 0, -0.25), (-0.785, 0.785), 180.0, 4.5, [((-0.14, 0, -0.07), -2.03, 0.15)]),
        ("bfoot", 2, (-0.28, 0, -0.14), (-0.4, 0.785), 120.0, 3.0, [((0.03, 0, -0.097), -0.27, 0.094)]),
        ("fthigh", 0, (0.5, 0, 0), (-1.0, 0.7), 180.0, 4.5, [((-0.07, 0, -0.12), 0.52, 0.133)]),
        ("fshin", 4, (-0.14, 0, -0.24), (-1.2, 0.87), 120.0, 3.0, [((0.065, 0, -0.09), -0.6, 0.106)]),
        ("ffoot", 5, (0.13, 0, -0.18), (-0.5, 0.5), 60.0, 1.5, [((0.045, 0, -0.07), -0.6, 0.07)]),
    ]
    coll = []
    qi = di = 0
    link_ids, joint_dof = {}, {}
    for i, (name, parent, pos, rng, stiff, damp, geoms) in enumerate(links):
        link_ids[name] = i
        s.parent[i] = parent
        _set3(s.link_pos, i, pos)
        _set3(s.link_rot, i, ident)
        _set3(s.joint_rot, i, hinge_y)
        ns = 2 if parent < 0 else 0
        s.n_slide[i], s.n_link_dof[i] = ns, ns + 1
        s.q_start[i], s.dof_start[i] = qi, di
        if ns:
            for k, ax in enumerate([(1.0, 0.0, 0.0), (0.0, 0.0, 1.0)]):
                for c in range(3):
                    s.slide_axis[i][k][c] = ax[c]
            lo, hi = -1e9, 1e9  # rooty is unlimited
            for k in range(ns):  # ... and so are the root slides
                s.dof_lo[di + k], s.dof_hi[di + k] = -1e9, 1e9
        else:
            lo, hi = rng
        d = di + ns
        s.dof_lo[d], s.dof_hi[d] = lo, hi
        s.dof_stiffness[d], s.dof_damping[d] = stiff, damp
        joint_dof[name] = d
        # centre of mass: capsule-volume weighted mean of the geom centres
        vols, ctrs = [], []
        for gpos, th, half in geoms:
            vols.append(math.pi * r * r * 2 * half + 4.0 / 3.0 * math.pi * r**3)
            ctrs.append(np.asarray(gpos, dtype=np.float64))
            e0, e1 = _capsule_ends(gpos, th, half)
            coll += [(i, e0, r), (i, e1, r)]
        com = sum(v * c for v, c in zip(vols, ctrs)) / sum(vols)
        _set3(s.com, i, com)
        s.mass[i] = 1.0
        _set3(s.inv_inertia, i, (1.0, 1.0, 1.0))
        s.k_pos[i], s.k_vel[i], s.k_limit[i], s.k_ang_damp[i] = 15000.0, 100.0, 1000.0, 20.0
        qi, di = qi + ns + 1, di + ns + 1
    # gears: half_cheetah.py's spring-backend branch replaces the MJCF's (120, 90, 60, 120, 60, 30) with
    # [120, 90, 60, 120, 100, 100] together with the timestep / n_frames above [upstream-memory]; applied since round 6
    # (rounds 1-5 kept the MJCF's front shin / foot gears: DESIGN.md section 7, provenance ledger)
    for k, (name, gear) in enumerate([("bthigh", 120.0), ("bshin", 90.0), ("bfoot", 60.0), ("fthigh", 120.0),
                                      ("fshin", 100.0), ("ffoot", 100.0)]):
        s.act_dof[k], s.act_gear[k], s.act_lo[k], s.act_hi[k] = joint_dof[name], gear, -1.0, 1.0
    s.n_coll = len(coll)
    for k, (link, pos, rad) in enumerate(coll):
        s.coll_link[k], s.coll_radius[k] = link, rad
        _set3(s.coll_pos, k, pos)
    for i in range(s.n_q):
        s.init_q[i] = 0.0
    _wire_context(s, feature_names, reference_compat, link_ids,
                  {"mass_torso": 10.0, "mass_bthigh": 1.5435146, "mass_bshin": 1.5874476, "mass_bfoot": 1.0953975,
                   "mass_fthigh": 1.4380753, "mass_fshin": 1.2008368, "mass_ffoot": 0.8845188})
    # STATE_INDICES["halfcheetah"] = [14, 15] (brax_walker_goal_wrapper.py:9; Quirk B3: these are not
    # the root x/y velocities of the 17-dim obs -- replicated as written), half_cheetah.xml timestep 0.01
    s.goal_obs_idx[0], s.goal_obs_idx[1], s.goal_dt = 14, 15, 0.01
    return s


def _frame_quat(a0, a1) -> tuple[float, float, float, float]:
    """quaternion of the joint frame whose x / y axes are the (orthogonal) hinge axes a0 / a1"""
    x = np.asarray(a0, dtype=np.float64)
    x = x / np.linalg.norm(x)
    y = np.asarray(a1, dtype=np.float64)
    y = y - x * float(x @ y)
    y = y / np.linalg.norm(y)
    z = np.cross(x, y)
    R = np.stack([x, y, z], axis=1)
    # Shepperd's method
    t = np.trace(R)
    if t > 0:
        w = math.sqrt(1.0 + t) / 2
        q = (w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w))
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        r = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        v = [0.0, 0.0, 0.0]
        v[i] = r / 2
        v[j] = (R[j, i] + R[i, j]) / (2 * r)
        v[k] = (R[k, i] + R[i, k]) / (2 * r)
        q = ((R[k, j] - R[j, k]) / (2 * r), v[0], v[1], v[2])
    n = math.sqrt(sum(c * c for c in q))
    return tuple(float(c / n) for c in q)


def _vol(kind, a, b, r):
    if kind == "sphere":
        return 4.0 / 3.0 * math.pi * r**3
    return math.pi * r * r * float(np.linalg.norm(np.subtract(b, a))) + 4.0 / 3.0 * math.pi * r**3


HUMANOID_MASSES = masses("humanoid")  # mass_<link> -> CARL default (feature_tables.py)


def humanoid_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """Humanoid: torso (free root) + lwaist (2 hinges), pelvis (1), 2 x (thigh: 3 hinges, shin: 1),
    2 x (upper arm: 2 hinges, lower arm: 1); q 24, qd 23, 17 motors, obs 244 =
    q[2:] (22) ++ qd (23) ++ com inertia (11 x 10) ++ com velocity (11 x 6) ++ qfrc_actuator (23).

    Geometry, joint axes / ranges / stiffness, gears and env constants restated from upstream
    memory of brax's ``humanoid.xml`` (a Gym-Humanoid derivative) and ``brax/envs/humanoid.py``
    (spring backend: dt 0.0015 x 10 frames; forward weight 1.25 on the whole-body COM velocity,
    healthy reward 5 while z in [1, 2], ctrl cost 0.1, reset noise U(+-0.01) on q AND qd).
    Multi-dof joints stack intrinsically in MJCF joint order about the joint frame's x, y, +-z
    (``dof_sign3``); the spring-constraint constants are this build's choice.  PARITY UNPINNED against brax itself;
    the GEOMETRY is pinned: the capsule / sphere volumes of every link reproduce the masses the reference holds as
    context defaults (tests/test_brax_model_tables.py, via an independent MJCF reader in the test infrastructure, which
    also compares every field of this table -- round 4: that comparison moved the knees' joint stiffness 1 -> 0
    (the asset gives none) and the left hip's y range -110 -> -120 degrees)."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_HUMANOID
    s.healthy_q_index = -1
    s.n_links, s.n_q, s.n_dof, s.n_act = 11, 24, 23, 17
    s.n_frames = 10
    s.max_episode_steps = 1000
    s.terminate_when_unhealthy = 1
    s.exclude_current_positions = 2
    s.obs_extended, s.reset_vel_uniform, s.reward_on_com = 1, 1, 1
    s.obs_dim = (s.n_q - 2) + s.n_dof + 16 * s.n_links + s.n_dof  # 244
    s.dt = 0.0015
    s.gravity_z, s.vel_damping, s.ang_damping = -9.81, 0.0, 0.0
    s.baumgarte_erp, s.elasticity, s.friction = 0.1, 0.0, 1.0
    s.healthy_z_lo, s.healthy_z_hi, s.healthy_reward = 1.0, 2.0, 5.0
    s.ctrl_cost_weight, s.forward_reward_weight = 0.1, 1.25
    s.reset_noise_scale, s.reset_vel_scale = 0.01, 0.01
    ident = (1.0, 0.0, 0.0, 0.0)
    tilt = (1.0, 0.0, -0.002, 0.0)
    X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    cap, sph = "capsule", "sphere"
    # (name, parent, body pos, body quat, joint pos, joints[(name, axis, (lo, hi) deg, stiffness, damping)], geoms)
    links = [
        ("torso", -1, (0, 0, 1.4), ident, (0, 0, 0), None,
         [(cap, (0, -0.07, 0), (0, 0.07, 0), 0.07), (sph, (0, 0, 0.19), None, 0.09),
          (cap, (-0.01, -0.06, -0.12), (-0.01, 0.06, -0.12), 0.06)]),
        ("lwaist", 0, (-0.01, 0, -0.26), tilt, (0, 0, 0.065),
         [("abdomen_z", Z, (-45, 45), 20, 5), ("abdomen_y", Y, (-75, 30), 10, 5)],
         [(cap, (0, -0.06, 0), (0, 0.06, 0), 0.06)]),
        ("pelvis", 1, (0, 0, -0.165), tilt, (0, 0, 0.1), [("abdomen_x", X, (-35, 35), 10, 5)],
         [(cap, (-0.02, -0.07, 0), (-0.02, 0.07, 0), 0.09)]),
        ("right_thigh", 2, (0, -0.1, -0.04), ident, (0, 0, 0),
         [("right_hip_x", X, (-25, 5), 10, 5), ("right_hip_z", Z, (-60, 35), 10, 5),
          ("right_hip_y", Y, (-110, 20), 20, 5)],
         [(cap, (0, 0, 0), (0, 0.01, -0.34), 0.06)]),
        ("right_shin", 3, (0, 0.01, -0.403), ident, (0, 0, 0.02), [("right_knee", (0, -1, 0), (-160, -2), 0, 1)],
         [(cap, (0, 0, 0), (0, 0, -0.3), 0.049), (sph, (0, 0, -0.35), None, 0.075)]),
        ("left_thigh", 2, (0, 0.1, -0.04), ident, (0, 0, 0),
         [("left_hip_x", (-1, 0, 0), (-25, 5), 10, 5), ("left_hip_z", (0, 0, -1), (-60, 35), 10, 5),
          ("left_hip_y", Y, (-120, 20), 20, 5)],  # (the asset's asymmetry: right -110, left -120)
         [(cap, (0, 0, 0), (0, -0.01, -0.34), 0.06)]),
        ("left_shin", 5, (0, -0.01, -0.403), ident, (0, 0, 0.02), [("left_knee", (0, -1, 0), (-160, -2), 0, 1)],
         [(cap, (0, 0, 0), (0, 0, -0.3), 0.049), (sph, (0, 0, -0.35), None, 0.075)]),
        ("right_upper_arm", 0, (0, -0.17, 0.06), ident, (0, 0, 0),
         [("right_shoulder1", (2, 1, 1), (-85, 60), 1, 1), ("right_shoulder2", (0, -1, 1), (-85, 60), 1, 1)],
         [(cap, (0, 0, 0), (0.16, -0.16, -0.16), 0.04)]),
        ("right_lower_arm", 7, (0.18, -0.18, -0.18), ident, (0, 0, 0),
         [("right_elbow", (0, -1, 1), (-90, 50), 0, 1)],
         [(cap, (0.01, 0.01, 0.01), (0.17, 0.17, 0.17), 0.031), (sph, (0.18, 0.18, 0.18), None, 0.04)]),
        ("left_upper_arm", 0, (0, 0.17, 0.06), ident, (0, 0, 0),
         [("left_shoulder1", (2, -1, 1), (-60, 85), 1, 1), ("left_shoulder2", (0, 1, 1), (-60, 85), 1, 1)],
         [(cap, (0, 0, 0), (0.16, 0.16, -0.16), 0.04)]),
        ("left_lower_arm", 9, (0.18, 0.18, -0.18), ident, (0, 0, 0),
         [("left_elbow", (0, -1, -1), (-90, 50), 0, 1)],
         [(cap, (0.01, -0.01, 0.01), (0.17, -0.17, 0.17), 0.031), (sph, (0.18, -0.18, 0.18), None, 0.04)]),
    ]
    coll, link_ids, joint_dof = [], {}, {}
    qi = di = 0
    for i, (name, parent, pos, quat, jpos, joints, geoms) in enumerate(links):
        link_ids[name] = i
        s.parent[i] = parent
        _set3(s.link_pos, i, pos)
        qn = np.asarray(quat, dtype=np.float64)
        _set3(s.link_rot, i, qn / np.linalg.norm(qn))
        _set3(s.joint_pos, i, jpos)
        s.q_start[i], s.dof_start[i] = qi, di
        s.n_slide[i] = 0
        s.dof_sign3[i] = 1.0
        if joints is None:
            s.n_link_dof[i] = 6
            _set3(s.joint_rot, i, ident)
            qi, di = qi + 7, di + 6
        else:
            nr = len(joints)
            s.n_link_dof[i] = nr
            axes = [np.asarray(j[1], dtype=np.float64) / np.linalg.norm(j[1]) for j in joints]
            if nr == 1:
                _set3(s.joint_rot, i, _axis_quat(axes[0]))
            else:
                assert abs(float(axes[0] @ axes[1])) < 1e-12
                _set3(s.joint_rot, i, _frame_quat(axes[0], axes[1]))
                if nr == 3:
                    sg = float(np.cross(axes[0], axes[1]) @ axes[2])
                    assert abs(abs(sg) - 1.0) < 1e-12
                    s.dof_sign3[i] = 1.0 if sg > 0 else -1.0
            for k, (jn, _ax, (lo, hi), stiff, damp) in enumerate(joints):
                d = di + k
                joint_dof[jn] = d
                s.dof_lo[d], s.dof_hi[d] = math.radians(lo), math.radians(hi)
                s.dof_stiffness[d], s.dof_damping[d] = float(stiff), float(damp)
            qi, di = qi + nr, di + nr
        vols, ctrs = [], []
        for kind, a, b, r in geoms:
            vols.append(_vol(kind, a, b, r))
            if kind == "sphere":
                ctrs.append(np.asarray(a, dtype=np.float64))
                coll.append((i, a, r))
            else:
                ctrs.append((np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64)) / 2)
                coll += [(i, a, r), (i, b, r)]
        _set3(s.com, i, sum(v * c for v, c in zip(vols, ctrs)) / sum(vols))
        s.mass[i] = 1.0
        _set3(s.inv_inertia, i, (1.0, 1.0, 1.0))
        # spring-constraint constants: rounds 1-5 used this build's own (20 000 / 100 / 1 000 / 20).  Under the spring
        # branch's actuator gears (below) HumanoidStandup -- which never terminates -- then blew up in 37 of 16 384 envs within
        # 1 000 steps of full-range random actions (tools/diag_standup_sweep.py, profiles/r06_standup_gear_stability.txt);
        # the set remembered from humanoid.xml's `<custom>` numerics (constraint_stiffness 27 000, constraint_vel_damping
        # 80, constraint_limit_stiffness 2 500, constraint_ang_damping 30) [upstream-memory, medium confidence] is stable
        # with them (0 of 16 384) -- gears and constants are tuned together upstream.  Adopted in round 6.
        s.k_pos[i], s.k_vel[i], s.k_limit[i], s.k_ang_damp[i] = 27000.0, 80.0, 2500.0, 30.0
    assert qi == s.n_q and di == s.n_dof
    # gears: humanoid.py / humanoidstandup.py replace the MJCF's (100 / 300 / 200 on torso and legs, 25 on the arms) with
    # [350] * 11 + [100] * 6 in the same `backend in ['spring', 'positional']` branch that sets timestep 0.0015 and
    # n_frames 10 [upstream-memory]; CARLBraxEnv always asks for "spring" (carl_brax_env.py:117,163-167).  Applied since
    # round 6 (rounds 1-5 took the timestep half of that branch and kept the MJCF gears)
    motors = [("abdomen_y", 350), ("abdomen_z", 350), ("abdomen_x", 350), ("right_hip_x", 350), ("right_hip_z", 350),
              ("right_hip_y", 350), ("right_knee", 350), ("left_hip_x", 350), ("left_hip_z", 350), ("left_hip_y", 350),
              ("left_knee", 350), ("right_shoulder1", 100), ("right_shoulder2", 100), ("right_elbow", 100),
              ("left_shoulder1", 100), ("left_shoulder2", 100), ("left_elbow", 100)]
    for k, (jn, gear) in enumerate(motors):
        s.act_dof[k], s.act_gear[k], s.act_lo[k], s.act_hi[k] = joint_dof[jn], float(gear), -0.4, 0.4
    s.n_coll = len(coll)
    assert s.n_coll <= _lib.BRAX_MAX_COLL
    for k, (link, pos, rad) in enumerate(coll):
        s.coll_link[k], s.coll_radius[k] = link, rad
        _set3(s.coll_pos, k, pos)
    init_q = [0.0, 0.0, 1.4, 1.0, 0.0, 0.0, 0.0] + [0.0] * 17
    for i, v in enumerate(init_q):
        s.init_q[i] = v
    _wire_context(s, feature_names, reference_compat, link_ids, HUMANOID_MASSES)
    # STATE_INDICES["humanoid"] = [22, 23] (brax_walker_goal_wrapper.py:8) on the 244-dim obs
    # (= qd[0], qd[1], the root's world x / y velocity); humanoid.xml timestep 0.003 (Quirk B3)
    s.goal_obs_idx[0], s.goal_obs_idx[1], s.goal_dt = 22, 23, 0.003
    return s

def _planar_chain(s, links, *, k_pos, k_vel, k_limit, k_ang_damp):
    """Fill link / joint / collider arrays of a planar (x-z) model: the first link is jointed to the
    world by slides along x and z plus a hinge about y (MuJoCo's rootx / rootz / rooty), every other
    link by one hinge.  ``links``: (name, parent, body pos, hinge axis, (lo, hi) rad, stiffness,
    damping, geoms[(end0, end1, radius)]) with capsule ends in the link frame."""
    ident = (1.0, 0.0, 0.0, 0.0)
    coll, link_ids, joint_dof = [], {}, {}
    qi = di = 0
    for i, (name, parent, pos, axis, rng, stiff, damp, geoms) in enumerate(links):
        link_ids[name] = i
        s.parent[i] = parent
        _set3(s.link_pos, i, pos)
        _set3(s.link_rot, i, ident)
        _set3(s.joint_rot, i, _axis_quat(axis))
        ns = 2 if parent < 0 else 0
        s.n_slide[i], s.n_link_dof[i] = ns, ns + 1
        s.q_start[i], s.dof_start[i] = qi, di
        s.dof_sign3[i] = 1.0
        if ns:
            for k, ax in enumerate([(1.0, 0.0, 0.0), (0.0, 0.0, 1.0)]):
                for c in range(3):
                    s.slide_axis[i][k][c] = ax[c]
                s.dof_lo[di + k], s.dof_hi[di + k] = -1e9, 1e9
            lo, hi = -1e9, 1e9
        else:
            lo, hi = rng
        d = di + ns
        s.dof_lo[d], s.dof_hi[d] = lo, hi
        s.dof_stiffness[d], s.dof_damping[d] = float(stiff), float(damp)
        joint_dof[name] = d
        vols, ctrs = [], []
        for e0, e1, r in geoms:
            vols.append(_vol("capsule", e0, e1, r))
            ctrs.append((np.asarray(e0, dtype=np.float64) + np.asarray(e1, dtype=np.float64)) / 2)
            coll += [(i, e0, r), (i, e1, r)]
        _set3(s.com, i, sum(v * c for v, c in zip(vols, ctrs)) / sum(vols))
        s.mass[i] = 1.0
        _set3(s.inv_inertia, i, (1.0, 1.0, 1.0))
        s.k_pos[i], s.k_vel[i], s.k_limit[i], s.k_ang_damp[i] = k_pos, k_vel, k_limit, k_ang_damp
        qi, di = qi + ns + 1, di + ns + 1
    s.n_coll = len(coll)
    assert s.n_coll <= _lib.BRAX_MAX_COLL
    for k, (link, pos, rad) in enumerate(coll):
        s.coll_link[k], s.coll_radius[k] = link, rad
        _set3(s.coll_pos, k, pos)
    return link_ids, joint_dof


def _walker_common(s):
    s.max_episode_steps = 1000
    s.terminate_when_unhealthy = 1
    s.exclude_current_positions = 1
    s.reset_vel_uniform = 1
    s.dt, s.n_frames = 0.001, 8
    s.gravity_z, s.vel_damping, s.ang_damping = -9.81, 0.0, 0.0
    s.baumgarte_erp, s.elasticity, s.friction = 0.1, 0.0, 1.0
    s.healthy_reward, s.ctrl_cost_weight, s.forward_reward_weight = 1.0, 1e-3, 1.0
    s.reset_noise_scale, s.reset_vel_scale = 5e-3, 5e-3
    s.obs_qd_clip = 10.0
    s.healthy_q_index = 2  # rooty: the torso pitch


def hopper_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """Hopper: planar torso + thigh / leg / foot hinges (about -y); q 6, qd 6, 3 motors (gear 200),
    obs 11 = q[1:] ++ clip(qd, +-10).  Healthy while z >= 0.7 and |pitch| <= 0.2; reward = forward
    velocity + 1 - 1e-3 |a|^2; reset noise U(+-5e-3) on q and qd.  Geometry and ranges restated from
    upstream memory of brax's ``hopper.xml`` (a Gym-Hopper derivative) and ``brax/envs/hopper.py``;
    dt 0.001 x 8 frames and the spring constants are this build's choice.  PARITY UNPINNED."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_HOPPER
    _walker_common(s)
    s.n_links, s.n_q, s.n_dof, s.n_act = 4, 6, 6, 3
    s.obs_dim = 11
    s.healthy_z_lo, s.healthy_z_hi = 0.7, 1e9
    s.healthy_q_lo, s.healthy_q_hi = -0.2, 0.2
    ny = (0, -1, 0)
    links = [
        ("torso", -1, (0, 0, 0), (0, 1, 0), None, 0, 0, [((0, 0, 0.2), (0, 0, -0.2), 0.05)]),
        ("thigh", 0, (0, 0, -0.2), ny, (math.radians(-150), 0.0), 0, 1, [((0, 0, 0), (0, 0, -0.45), 0.05)]),
        ("leg", 1, (0, 0, -0.45), ny, (math.radians(-150), 0.0), 0, 1, [((0, 0, 0), (0, 0, -0.5), 0.04)]),
        ("foot", 2, (0, 0, -0.5), ny, (math.radians(-45), math.radians(45)), 0, 1,
         [((-0.13, 0, 0), (0.26, 0, 0), 0.06)]),
    ]
    link_ids, joint_dof = _planar_chain(s, links, k_pos=20000.0, k_vel=100.0, k_limit=1000.0, k_ang_damp=20.0)
    s.init_q[1] = 1.25  # rootz carries MuJoCo's ref = 1.25: q[1] (and obs[0]) is the torso height
    for k, name in enumerate(["thigh", "leg", "foot"]):
        s.act_dof[k], s.act_gear[k], s.act_lo[k], s.act_hi[k] = joint_dof[name], 200.0, -1.0, 1.0
    _wire_context(s, feature_names, reference_compat, link_ids,
                  {"mass_torso": 10.0, "mass_thigh": 4.0578904, "mass_leg": 2.7813568, "mass_foot": 5.3155746})
    # STATE_INDICES["hopper"] = [5, 6] (brax_walker_goal_wrapper.py:10), hopper.xml timestep 0.002
    s.goal_obs_idx[0], s.goal_obs_idx[1], s.goal_dt = 5, 6, 0.002
    return s


def walker2d_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """Walker2d: planar torso + two (thigh, leg, foot) chains; q 9, qd 9, 6 motors (gear 100), obs 17.
    Healthy while 0.8 <= z <= 2 and |pitch| <= 1.  Restated from upstream memory of brax's
    ``walker2d.xml`` / ``brax/envs/walker2d.py``; PARITY UNPINNED."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_WALKER2D
    _walker_common(s)
    s.n_links, s.n_q, s.n_dof, s.n_act = 7, 9, 9, 6
    s.obs_dim = 17
    s.healthy_z_lo, s.healthy_z_hi = 0.8, 2.0
    s.healthy_q_lo, s.healthy_q_hi = -1.0, 1.0
    ny = (0, -1, 0)
    leg_rng = (math.radians(-150), 0.0)
    foot_rng = (math.radians(-45), math.radians(45))
    links = [("torso", -1, (0, 0, 0), (0, 1, 0), None, 0, 0, [((0, 0, 0.2), (0, 0, -0.2), 0.05)])]
    for suffix in ("", "_left"):
        base = len(links)
        links += [
            ("thigh" + suffix, 0, (0, 0, -0.2), ny, leg_rng, 0, 0.1, [((0, 0, 0), (0, 0, -0.45), 0.05)]),
            ("leg" + suffix, base, (0, 0, -0.45), ny, leg_rng, 0, 0.1, [((0, 0, 0), (0, 0, -0.5), 0.04)]),
            ("foot" + suffix, base + 1, (0, 0, -0.5), ny, foot_rng, 0, 0.1, [((0.0, 0, 0), (0.2, 0, 0), 0.06)]),
        ]
    link_ids, joint_dof = _planar_chain(s, links, k_pos=20000.0, k_vel=100.0, k_limit=1000.0, k_ang_damp=20.0)
    s.init_q[1] = 1.25  # rootz ref, as for the hopper
    for k, name in enumerate(["thigh", "leg", "foot", "thigh_left", "leg_left", "foot_left"]):
        s.act_dof[k], s.act_gear[k], s.act_lo[k], s.act_hi[k] = joint_dof[name], 100.0, -1.0, 1.0
    _wire_context(s, feature_names, reference_compat, link_ids,
                  {"mass_torso": 10.0, "mass_thigh": 4.0578904, "mass_leg": 2.7813568, "mass_foot": 3.1667254,
                   "mass_thigh_left": 4.0578904, "mass_leg_left": 2.7813568, "mass_foot_left": 3.1667254})
    # STATE_INDICES["walker2d"] = [8, 9] (brax_walker_goal_wrapper.py:11), walker2d.xml timestep 0.002
    s.goal_obs_idx[0], s.goal_obs_idx[1], s.goal_dt = 8, 9, 0.002
    return s


def inverted_pendulum_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """InvertedPendulum: a cart on a slider (x, range +-1; no hinge: all three rotations locked by the
    joint) carrying a pole on a hinge about y; q 2, qd 2, one motor on the slider (gear 100, ctrl +-3),
    obs 4, reward 1 per step, done when |pole angle| > 0.2; no contacts.  Restated from upstream memory
    of brax's ``inverted_pendulum.xml`` / ``brax/envs/inverted_pendulum.py``; dt 0.005 x 8 frames and
    the spring constants are this build's choice.  PARITY UNPINNED."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_INVERTED_PENDULUM
    s.n_links, s.n_q, s.n_dof, s.n_act = 2, 2, 2, 1
    s.obs_dim = 4
    s.max_episode_steps = 1000
    s.terminate_when_unhealthy = 1
    s.exclude_current_positions = 0
    s.reset_vel_uniform = 1
    s.dt, s.n_frames = 0.005, 8
    s.gravity_z, s.vel_damping, s.ang_damping = -9.81, 0.0, 0.0
    s.baumgarte_erp, s.elasticity, s.friction = 0.1, 0.0, 1.0
    s.healthy_z_lo, s.healthy_z_hi = -1e9, 1e9
    s.healthy_q_index, s.healthy_q_lo, s.healthy_q_hi = 1, -0.2, 0.2
    s.healthy_reward, s.ctrl_cost_weight, s.forward_reward_weight = 1.0, 0.0, 0.0
    s.reset_noise_scale, s.reset_vel_scale = 0.01, 0.01
    ident = (1.0, 0.0, 0.0, 0.0)
    # cart: slide along x against the world, no rotational dof
    s.parent[0], s.n_slide[0], s.n_link_dof[0], s.q_start[0], s.dof_start[0] = -1, 1, 1, 0, 0
    _set3(s.link_rot, 0, ident)
    _set3(s.joint_rot, 0, ident)
    for c, v in enumerate((1.0, 0.0, 0.0)):
        s.slide_axis[0][0][c] = v
    s.dof_lo[0], s.dof_hi[0] = -1.0, 1.0
    s.dof_damping[0] = 1.0
    # pole: hinge about y at the cart's origin, capsule (0,0,0)-(0.001,0,0.6)
    s.parent[1], s.n_slide[1], s.n_link_dof[1], s.q_start[1], s.dof_start[1] = 0, 0, 1, 1, 1
    _set3(s.link_rot, 1, ident)
    _set3(s.joint_rot, 1, _axis_quat((0, 1, 0)))
    _set3(s.com, 1, (0.0005, 0.0, 0.3))
    s.dof_lo[1], s.dof_hi[1] = math.radians(-90), math.radians(90)
    s.dof_damping[1] = 1.0
    for i in range(2):
        s.dof_sign3[i] = 1.0
        s.mass[i] = 1.0
        _set3(s.inv_inertia, i, (1.0, 1.0, 1.0))
        s.k_pos[i], s.k_vel[i], s.k_limit[i], s.k_ang_damp[i] = 10000.0, 100.0, 1000.0, 10.0
    s.act_dof[0], s.act_gear[0], s.act_lo[0], s.act_hi[0] = 0, 100.0, -3.0, 3.0
    s.n_coll = 0
    _wire_context(s, feature_names, reference_compat, {"cart": 0, "pole": 1}, {"mass_cart": 1.0, "mass_pole": 1.0})
    return s


def humanoidstandup_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """HumanoidStandup: the Humanoid model lying on its back (root rotated -90 deg about y, torso
    0.105 above the ground); reward = torso height / dt_env (uph_cost) + 1 - 0.1 |a|^2, never
    terminates, observation as for Humanoid.  Restated from upstream memory of brax's
    ``humanoidstandup.xml`` / ``brax/envs/humanoidstandup.py`` (a Gym-HumanoidStandup derivative);
    PARITY UNPINNED."""
    s = humanoid_sys(feature_names, reference_compat)
    s.env_kind = _lib.BRAX_HUMANOIDSTANDUP
    s.terminate_when_unhealthy = 0
    s.healthy_z_lo, s.healthy_z_hi = -1e9, 1e9
    s.healthy_reward, s.ctrl_cost_weight, s.forward_reward_weight = 1.0, 0.1, 1.0
    s.reward_height, s.reward_on_com = 1, 0
    h = math.sqrt(0.5)
    for i, v in enumerate([0.0, 0.0, 0.105, h, 0.0, -h, 0.0]):
        s.init_q[i] = v
    return s


def inverted_double_pendulum_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """InvertedDoublePendulum: cart on a slider (x, range +-1) + two poles of length 0.6 on hinges about
    y; q 3, qd 3, one motor on the slider (gear 500, ctrl +-1).  Observation (8) = cart x ++ sin(q[1:])
    ++ cos(q[1:]) ++ clip(qd, +-10); reward = 10 - (0.01 x_tip^2 + (z_tip - 2)^2) - (1e-3 qd1^2 +
    5e-3 qd2^2); done when the tip of the second pole is at z <= 1; reset q + U(+-0.01), qd = 0.1 N(0,1).
    Restated from upstream memory of brax's ``inverted_double_pendulum.xml`` /
    ``brax/envs/inverted_double_pendulum.py``; dt 0.0025 x 20 frames and the spring constants are this
    build's choice.  PARITY UNPINNED."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_INVERTED_DOUBLE_PENDULUM
    s.n_links, s.n_q, s.n_dof, s.n_act = 3, 3, 3, 1
    s.obs_trig_from = 1
    s.obs_dim = 1 + 2 + 2 + 3
    s.max_episode_steps = 1000
    s.terminate_when_unhealthy = 0  # the tip rule below decides
    s.exclude_current_positions = 0
    s.dt, s.n_frames = 0.0025, 20  # at 0.005 the gear-500 slider drives the spring joints unstable
    s.gravity_z, s.vel_damping, s.ang_damping = -9.81, 0.0, 0.0
    s.baumgarte_erp, s.elasticity, s.friction = 0.1, 0.0, 1.0
    s.healthy_z_lo, s.healthy_z_hi = -1e9, 1e9
    s.healthy_q_index = -1
    s.healthy_reward, s.ctrl_cost_weight, s.forward_reward_weight = 10.0, 0.0, 0.0
    s.reset_noise_scale, s.reset_vel_scale = 0.01, 0.1
    s.obs_qd_clip = 10.0
    s.tip_link = 2
    for c, v in enumerate((0.0, 0.0, 0.6)):
        s.tip_offset[c] = v
    s.tip_x_weight, s.tip_height, s.tip_min_height = 0.01, 2.0, 1.0
    s.tip_vel_weight[0], s.tip_vel_weight[1] = 1e-3, 5e-3
    s.tip_vel_dof[0], s.tip_vel_dof[1] = 1, 2
    ident = (1.0, 0.0, 0.0, 0.0)
    hinge_y = _axis_quat((0, 1, 0))
    # cart: slide along x against the world, no rotational dof
    s.parent[0], s.n_slide[0], s.n_link_dof[0], s.q_start[0], s.dof_start[0] = -1, 1, 1, 0, 0
    _set3(s.link_rot, 0, ident)
    _set3(s.joint_rot, 0, ident)
    for c, v in enumerate((1.0, 0.0, 0.0)):
        s.slide_axis[0][0][c] = v
    s.dof_lo[0], s.dof_hi[0] = -1.0, 1.0
    s.dof_damping[0] = 0.05
    for i, (parent, pos) in enumerate([(0, (0.0, 0.0, 0.0)), (1, (0.0, 0.0, 0.6))], start=1):
        s.parent[i], s.n_slide[i], s.n_link_dof[i], s.q_start[i], s.dof_start[i] = parent, 0, 1, i, i
        _set3(s.link_pos, i, pos)
        _set3(s.link_rot, i, ident)
        _set3(s.joint_rot, i, hinge_y)
        _set3(s.com, i, (0.0, 0.0, 0.3))
        s.dof_lo[i], s.dof_hi[i] = -1e9, 1e9
        s.dof_damping[i] = 0.05
    for i in range(3):
        s.dof_sign3[i] = 1.0
        s.mass[i] = 1.0
        _set3(s.inv_inertia, i, (1.0, 1.0, 1.0))
        s.k_pos[i], s.k_vel[i], s.k_limit[i], s.k_ang_damp[i] = 10000.0, 100.0, 1000.0, 10.0
    s.act_dof[0], s.act_gear[0], s.act_lo[0], s.act_hi[0] = 0, 500.0, -1.0, 1.0
    s.n_coll = 0
    _wire_context(s, feature_names, reference_compat, {"cart": 0, "pole": 1, "pole2": 2},
                  {"mass_cart": 1.0, "mass_pole": 1.0, "mass_pole2": 1.0})
    return s


def reacher_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """Reacher: a two-link arm in the horizontal plane (body0 on a hinge about z against the world,
    body1 on a hinge about z, range +-3 rad, 0.1 m further out; fingertip 0.11 m along body1) and a
    goal marker on two slides (x, y, range +-0.27) against the world; q 4, qd 4, two motors (ctrl +-1).
    Observation (11) = cos(q[:2]) ++ sin(q[:2]) ++ goal (x, y) ++ arm qd ++ (fingertip - goal);
    reward = -|fingertip - goal| - |a|^2; never terminates; reset: arm q = U(+-0.1), arm qd =
    U(+-0.005), goal at a uniform distance (< 0.2) and bearing, at rest.  Restated from upstream memory
    of brax's ``reacher.xml`` / ``brax/envs/reacher.py`` (spring backend: dt 0.005 x 4 frames, gear 25).
    Link masses are the reference's defaults (carl/envs/brax/carl_reacher.py:33-38); rotational inertias
    are 1 (the MJCF's armature = 1 dominates the capsules' 1e-5 kg m^2), the goal marker is given 0.01 kg
    (its 3e-6 kg sphere cannot be carried by an explicit spring) and the spring constants are sized for
    these masses -- this build's choices.  PARITY UNPINNED."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_REACHER
    s.n_links, s.n_q, s.n_dof, s.n_act = 3, 4, 4, 2
    s.target_link, s.target_max_dist = 2, 0.2
    s.tip_link = 1
    for c, v in enumerate((0.11, 0.0, 0.0)):
        s.tip_offset[c] = v
    s.obs_dim = 11
    s.max_episode_steps = 1000
    s.terminate_when_unhealthy = 0
    s.exclude_current_positions = 0
    s.reset_vel_uniform = 1
    s.dt, s.n_frames = 0.005, 4
    s.gravity_z, s.vel_damping, s.ang_damping = -9.81, 0.0, 0.0
    s.baumgarte_erp, s.elasticity, s.friction = 0.1, 0.0, 1.0
    s.healthy_z_lo, s.healthy_z_hi = -1e9, 1e9
    s.healthy_q_index = -1
    s.healthy_reward, s.ctrl_cost_weight, s.forward_reward_weight = 0.0, 1.0, 0.0
    s.reset_noise_scale, s.reset_vel_scale = 0.1, 0.005
    ident = (1.0, 0.0, 0.0, 0.0)
    hinge_z = _axis_quat((0, 0, 1))
    arm = [(-1, (0.0, 0.0, 0.01), 0.05, 0.03560472, (-1e9, 1e9)),
           (0, (0.1, 0.0, 0.0), (0.03560472 * 0.05 + 0.00418879 * 0.11) / 0.03979351, 0.03979351, (-3.0, 3.0))]
    for i, (parent, pos, com_x, mass, rng) in enumerate(arm):
        s.parent[i], s.n_slide[i], s.n_link_dof[i], s.q_start[i], s.dof_start[i] = parent, 0, 1, i, i
        _set3(s.link_pos, i, pos)
        _set3(s.link_rot, i, ident)
        _set3(s.joint_rot, i, hinge_z)
        _set3(s.com, i, (com_x, 0.0, 0.0))
        s.mass[i] = mass
        s.dof_lo[i], s.dof_hi[i] = rng
        s.dof_damping[i] = 1.0
        s.k_pos[i], s.k_vel[i], s.k_limit[i], s.k_ang_damp[i] = 400.0, 1.5, 100.0, 1.0
        s.act_dof[i], s.act_gear[i], s.act_lo[i], s.act_hi[i] = i, 25.0, -1.0, 1.0
    # goal marker: two slides against the world, no rotational dof
    s.parent[2], s.n_slide[2], s.n_link_dof[2], s.q_start[2], s.dof_start[2] = -1, 2, 2, 2, 2
    _set3(s.link_pos, 2, (0.0, 0.0, 0.01))
    _set3(s.link_rot, 2, ident)
    _set3(s.joint_rot, 2, ident)
    for k, ax in enumerate(((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))):
        for c, v in enumerate(ax):
            s.slide_axis[2][k][c] = v
        s.dof_lo[2 + k], s.dof_hi[2 + k] = -0.27, 0.27
    s.mass[2] = 0.01
    s.k_pos[2], s.k_vel[2], s.k_limit[2], s.k_ang_damp[2] = 100.0, 1.0, 100.0, 1.0
    for i in range(3):
        s.dof_sign3[i] = 1.0
        _set3(s.inv_inertia, i, (1.0, 1.0, 1.0))
    s.n_coll = 0
    _wire_context(s, feature_names, reference_compat, {"body0": 0, "body1": 1},
                  {"mass_body0": 0.03560472, "mass_body1": 0.03979351})
    return s


PUSHER_MASSES = masses("pusher")


def pusher_sys(feature_names: list[str] | None = None, reference_compat: bool = False) -> _lib.BraxSys:
    """Pusher: a 7-hinge arm (shoulder pan z / lift y / upper-arm roll x, elbow flex y, forearm roll x,
    wrist flex y / roll x; the jointless upper-arm, forearm and fork bodies are fused into their
    parents as brax's MJCF loader does) whose U-shaped gripper pushes a puck (radius 0.05, half height
    0.05, on two damped slides at table height) towards a goal.  q 9, qd 9, 7 motors (gear 1, ctrl +-2),
    obs 23 = arm q ++ arm qd ++ COM of the gripper link, the puck, the goal; reward = -|puck - goal| -
    0.1 |a|^2 - 0.5 |puck - gripper|; never terminates; reset: arm at init_q with rates U(+-0.005), puck
    uniform in [-0.3, 0] x [-0.2, 0.2] about its MJCF position, pushed out of the 0.17 disc around the
    goal.  Restated from upstream memory of brax's ``pusher.xml`` (a Gym Pusher derivative: gravity
    0 0 0 in the MJCF, joint damping 1 / 0.1) and ``brax/envs/pusher.py``.  The goal position is the
    context's ``goal_position_x/y/z`` (carl/envs/brax/carl_pusher.py:80-103 hands it to the env as
    ``_goal_pos``); without those rows it is the MJCF goal body (0.45, -0.05, -0.323), and brax's goal
    marker body (two slides, no collisions) is not simulated.  Link masses are the reference's defaults
    (carl_pusher.py:37-79).  This build's choices: rotational inertias 1 (shoulder) ... 0.05 (wrist) in
    place of armature 0.04 + geometry; gripper-puck contact = 7 spheres along the fork against the puck
    (penalty contact with regularised Coulomb friction, ``carl_brax_sys_t::n_pair`` / ``pair_ct``); the table
    (round 5, ABI 8): the same 7 fork spheres collide with the plane z = -0.325 (``plane_z``: the MJCF's table
    geom, on which the puck's bottom face lies), and the puck slides on it with Coulomb friction under its
    weight (``obj_support``: friction x m |g| -- nothing with the MJCF's own zero gravity, the context's
    friction x 9.8 m/s^2 with CARL's default gravity); dt 0.001 x 50 so that
    the 1.8 g puck and the 5 g wrist link sit on explicit springs.  NOTE the reference's context default
    gravity = -9.8 applies in the intended form (the MJCF has none): the 2 N m motors do not hold the arm
    against it.  PARITY UNPINNED."""
    s = _lib.BraxSys()
    s.env_kind = _lib.BRAX_PUSHER
    s.n_links, s.n_q, s.n_dof, s.n_act = 8, 9, 9, 7
    s.push_link, s.tip_link = 7, 6
    for c, v in enumerate((0.45, -0.05, -0.323)):
        s.push_goal[c] = v
    s.push_near_weight, s.push_min_dist = 0.5, 0.17
    s.push_lo[0], s.push_hi[0], s.push_lo[1], s.push_hi[1] = -0.3, 0.0, -0.2, 0.2
    s.obs_dim = 23
    s.max_episode_steps = 1000
    s.terminate_when_unhealthy = 0
    s.exclude_current_positions = 0
    s.reset_vel_uniform = 1
    s.dt, s.n_frames = 0.001, 50
    s.gravity_z, s.vel_damping, s.ang_damping = 0.0, 0.0, 0.0
    s.baumgarte_erp, s.elasticity, s.friction = 0.1, 0.0, 1.0
    s.healthy_z_lo, s.healthy_z_hi = -1e9, 1e9
    s.healthy_q_index = -1
    s.healthy_reward, s.ctrl_cost_weight, s.forward_reward_weight = 0.0, 0.1, 0.0
    s.reset_noise_scale, s.reset_vel_scale = 0.0, 0.005
    ident = (1.0, 0.0, 0.0, 0.0)
    X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    names = ["r_shoulder_pan_link", "r_shoulder_lift_link", "r_upper_arm_roll_link", "r_elbow_flex_link",
             "r_forearm_roll_link", "r_wrist_flex_link", "r_wrist_roll_link", "object"]
    # parent, position in the parent, hinge axis, range, damping, COM, inertia, k_pos, k_vel
    arm = [(-1, (0.0, -0.6, 0.0), Z, (-2.2854, 1.714602), 1.0, (0.0, 0.0, -0.2), 1.0, 20000.0, 200.0),
           (0, (0.1, 0.0, 0.0), Y, (-0.5236, 1.3963), 1.0, (0.0, 0.0, 0.0), 1.0, 20000.0, 100.0),
           (1, (0.0, 0.0, 0.0), X, (-1.5, 1.7), 0.1, (0.2, 0.0, 0.0), 0.5, 10000.0, 50.0),
           (2, (0.4, 0.0, 0.0), Y, (-2.3213, 0.0), 0.1, (0.0, 0.0, 0.0), 0.2, 5000.0, 20.0),
           (3, (0.0, 0.0, 0.0), X, (-1.5, 1.5), 0.1, (0.14, 0.0, 0.0), 0.2, 5000.0, 20.0),
           (4, (0.321, 0.0, 0.0), Y, (-1.094, 0.0), 0.1, (0.0, 0.0, 0.0), 0.05, 1000.0, 2.0),
           (5, (0.0, 0.0, 0.0), X, (-1.5, 1.5), 0.1, (0.03, 0.0, 0.0), 0.05, 1000.0, 5.0)]
    for i, (parent, pos, axis, rng, damp, com, inertia, kp, kv) in enumerate(arm):
        s.parent[i], s.n_slide[i], s.n_link_dof[i], s.q_start[i], s.dof_start[i] = parent, 0, 1, i, i
        _set3(s.link_pos, i, pos)
        _set3(s.link_rot, i, ident)
        _set3(s.joint_rot, i, _axis_quat(axis))
        _set3(s.com, i, com)
        s.mass[i] = PUSHER_MASSES["mass_" + names[i]]
        _set3(s.inv_inertia, i, (1.0 / inertia,) * 3)
        s.dof_lo[i], s.dof_hi[i] = rng
        s.dof_damping[i] = damp
        s.k_pos[i], s.k_vel[i], s.k_limit[i], s.k_ang_damp[i] = kp, kv, 100.0, 0.5
        s.act_dof[i], s.act_gear[i], s.act_lo[i], s.act_hi[i] = i, 1.0, -2.0, 2.0
    # the puck: two slides against the world, no rotational dof
    s.parent[7], s.n_slide[7], s.n_link_dof[7], s.q_start[7], s.dof_start[7] = -1, 2, 2, 7, 7
    _set3(s.link_pos, 7, (0.45, -0.05, -0.275))
    _set3(s.link_rot, 7, ident)
    _set3(s.joint_rot, 7, ident)
    for k, ax in enumerate((X, Y)):
        for c, v in enumerate(ax):
            s.slide_axis[7][k][c] = float(v)
        s.dof_lo[7 + k], s.dof_hi[7 + k] = -10.3213, 10.3213
        s.dof_damping[7 + k] = 0.5
    s.mass[7] = PUSHER_MASSES["mass_object"]
    _set3(s.inv_inertia, 7, (1.0,) * 3)
    s.k_pos[7], s.k_vel[7], s.k_limit[7], s.k_ang_damp[7] = 500.0, 0.5, 100.0, 1.0
    for i in range(8):
        s.dof_sign3[i] = 1.0
    # the fork of r_wrist_roll_link: cross bar (0, +-0.1, 0) and two prongs reaching x = 0.1
    fork = [(0.0, -0.1, 0.0), (0.0, 0.0, 0.0), (0.0, 0.1, 0.0), (0.05, -0.1, 0.0), (0.1, -0.1, 0.0),
            (0.05, 0.1, 0.0), (0.1, 0.1, 0.0)]
    s.n_pair, s.pair_link = len(fork), 6
    for k, pos in enumerate(fork):
        _set3(s.pair_pos, k, pos)
        s.pair_radius[k] = 0.02
    s.pair_obj_radius, s.pair_obj_half, s.pair_k, s.pair_c = 0.05, 0.05, 500.0, 0.5
    # the table: the fork's spheres against the plane the puck lies on; friction in both contacts.  pair_ct: the
    # regularisation slope of the pair friction -- explicit, so pair_ct dt / m_puck (0.28) stays below 1
    s.plane_z, s.pair_ct, s.obj_support = -0.325, 0.5, 1
    s.n_coll = len(fork)
    for k, pos in enumerate(fork):
        s.coll_link[k] = 6
        _set3(s.coll_pos, k, pos)
        s.coll_radius[k] = 0.02
    _wire_context(s, feature_names, reference_compat, {n: i for i, n in enumerate(names)}, PUSHER_MASSES)
    return s


SYSTEMS = {"pusher": pusher_sys, "reacher": reacher_sys, "inverted_double_pendulum": inverted_double_pendulum_sys, "humanoidstandup": humanoidstandup_sys, "ant": ant_sys, "halfcheetah": halfcheetah_sys, "humanoid": humanoid_sys, "hopper": hopper_sys,
           "walker2d": walker2d_sys, "inverted_pendulum": inverted_pendulum_sys}
