"""The Brax kernel instance table (tests/brax_kernel_cases.py) against the library: every case lists exactly the widths
it names, and the cases together reach every entry of carl_brax.hip's `kBraxKernels` -- a kernel added without a case,
or a case whose kernel went away, fails here (host-side: no GPU)."""
import ctypes as C
import os
import re

from brax_kernel_cases import CASES, EXTRA_CASES, FP32, build, lane_widths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _instantiated():
    """(step entries, reset entries) of kBraxKernels as {(class, K)}, read off its initializer in carl_brax.hip"""
    with open(os.path.join(ROOT, "carl_amd", "csrc", "carl_brax.hip")) as f:
        src = f.read()
    body = re.search(r"const BraxKernel kBraxKernels\[\] = \{(.*?)\n\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    b = lambda v: v == "true"  # noqa: E731
    step, reset = [], []
    for m in re.finditer(r"CARL_BRAX\((\w+), (\d+), (\w+)\)", body):  # (MULTI, K, TASK): reset + step
        c = (b(m[1]), b(m[3]), False, False)
        step.append((c, int(m[2])))
        reset.append((c, int(m[2])))
    for m in re.finditer(r"CARL_BRAX_STEP\((\w+), (\d+), (\w+), (\w+)\)", body):  # (MULTI, K, PLANAR, F32): step only
        step.append(((b(m[1]), False, b(m[3]), b(m[4])), int(m[2])))
    n_entries = len(re.findall(r"CARL_BRAX(?:_STEP)?\(", body))
    assert len(step) == n_entries, "an entry of kBraxKernels this test cannot read"
    return step, reset


def test_every_case_lists_its_widths():
    for case in CASES + EXTRA_CASES:
        s, _, _ = build(case.model)
        assert lane_widths(s, case.flags) == case.widths, case


def test_the_cases_reach_every_kernel_instance():
    step, reset = _instantiated()
    assert len(step) == 29 and len(set(step)) == 29 and len(reset) == 11 and len(set(reset)) == 11
    assert {(c.step_class, w) for c in CASES for w in c.widths} == set(step)
    # a reset launch pinned to width w takes the narrowest width >= w of the case's reset class: the float64 cases pin
    # every reset entry exactly; the flagged ones (Hopper under GENERIC at 11: lean-16) land on one of them
    assert {(c.reset_class, w) for c in CASES if not c.flags for w in c.widths} == set(reset)
    for c in CASES + EXTRA_CASES:
        assert all(any(rc == c.reset_class and k >= w for rc, k in reset) for w in c.widths), c


def test_one_leg_ant_is_lean_and_the_task_models_refuse_float32():
    from carl_amd import _lib

    lib = _lib.load()
    ant, _, _ = build("one_leg_ant")
    assert (ant.n_links, ant.n_q, ant.n_dof, ant.n_act, ant.n_coll, ant.obs_dim) == (3, 9, 8, 2, 6, 15)
    assert list(ant.act_dof[:2]) == [6, 7]
    assert not lib.carl_brax_model_is_planar(C.byref(ant))
    assert lane_widths(ant, 0) == lane_widths(ant, FP32) == [4, 7, 8, 9, 16]
    for planar in ("hopper", "back_half_cheetah"):
        s, _, _ = build(planar)
        assert lib.carl_brax_model_is_planar(C.byref(s)), planar
    reacher, _, _ = build("reacher")
    assert lane_widths(reacher, FP32) == []


# ---- the inputs of tests/test_gpu_brax_context_matrix.py, on the float64 oracle alone -----------------------------------
import numpy as np  # noqa: E402
import pytest  # noqa: E402

import brax_kernel_cases as K  # noqa: E402

CTX_IDS = [c.label for c in K.CTX_CASES]


def test_the_env_wires_its_floors_through_the_function_the_cases_use():
    from carl_amd.envs.brax import carl_brax_env, models

    s, names, _ = K.build("hopper")
    K.wire_floors(s, names, "hopper")
    k = [names[s.ctx.mass_row[k]] for k in range(s.ctx.n_mass)].index("mass_torso")
    assert s.ctx.mass_ratio_floor[k] == np.float32(0.13) and s.ctx.mass_ratio_floor_multi[k] == np.float32(0.13 * 1.65)
    k = [names[s.ctx.mass_row[k]] for k in range(s.ctx.n_mass)].index("mass_foot")  # not measured: the default floor
    assert s.ctx.mass_ratio_floor[k] == np.float32(0.1)
    with open(carl_brax_env.__file__) as f:
        src = f.read()
    assert "models.wire_mass_floors(sys_table, names, self.env_name)" in src and "COMBINED_FLOOR_SCALE" not in src
    with open(K.__file__) as f:  # and the tests hold no copy of the rule
        assert "COMBINED_FLOOR_SCALE" not in f.read() and callable(models.wire_mass_floors)


def test_the_stiffness_cases_declare_the_column_and_list_their_widths():
    for case in K.STIFFNESS_CASES:
        s, names, _ = K.build(case.model)
        assert s.ctx.joint_stiffness_scale == names.index("joint_stiffness"), case
        assert set(case.widths) <= set(lane_widths(s, case.flags)), case
    assert [c.label for c in K.CTX_CASES if "joint_stiffness" in K.build(c.model)[1]] == ["cheetah_half_stiff",
                                                                                         "humanoid_stiff_f32"]


@pytest.mark.parametrize("case", K.CTX_CASES, ids=CTX_IDS)
def test_context_matrix_rows_cover_every_regime_and_every_reset_changes_the_masses(case):
    inp = K.ctx_inputs(case)
    s, names, rows = inp.sys, inp.names, inp.rows
    assert rows.shape == (K.CTX_N_CTX, len(names)) and (rows == rows.astype(np.float32)).all()
    for name, (lo, hi) in K.CTX_RANGES.items():  # every physics column the model declares moves, inside its range
        if name in names:
            col = rows[:, names.index(name)]
            assert len(np.unique(col)) == len(col) and col.min() >= np.float32(lo) and col.max() <= np.float32(hi), name
    for name in ("target_distance", "target_direction", "target_radius"):
        if name in names:
            assert (rows[:, names.index(name)] == inp.default[names.index(name)]).all()
    reg = K.mass_regimes(s, rows)
    assert (reg != "-").all()
    M = s.ctx.n_mass
    for k in range(M):
        # one mass feature (Ant): (d) needs two light links, which one feature cannot give
        for r in ("abcd" if M >= 2 else "abc"):
            assert (reg[:, k] == r).sum() >= 1, (case, k, r)
        for r in ("abcd" if 2 <= M <= 4 else "abc" if M == 1 else "ad"):  # twice wherever 37 rows can hold it
            assert (reg[:, k] == r).sum() >= 2, (case, k, r)
    # the effective masses of consecutive contexts of a lane differ (stride 3 of 37: every reset moves to another row)
    ratio, eff, _ = K.mass_ratios(s, rows)
    nxt = (np.arange(K.CTX_N_CTX) + K.CTX_STRIDE) % K.CTX_N_CTX
    assert ((ratio != ratio[nxt]).any(1) & (eff != eff[nxt]).any(1)).all()
    # on the oracle: every env resets inside the window, and each reset changes its context
    traj = K.oracle_trajectory(inp, inp.touch)
    resets = np.zeros(inp.n, int)
    for snap, _, _, _, _, _, ctx_after, done in traj:
        assert (ctx_after[done] == (snap["ctx_idx"][done] + K.CTX_STRIDE) % K.CTX_N_CTX).all()
        assert (ctx_after[done] != snap["ctx_idx"][done]).all() and (ctx_after[~done] == snap["ctx_idx"][~done]).all()
        resets += done
    assert resets.min() >= 2  # TimeLimit 4 in 9 steps
    assert len(np.unique(np.concatenate([t[0]["ctx_idx"] for t in traj]))) == K.CTX_N_CTX


@pytest.mark.parametrize("case", K.CTX_CASES, ids=CTX_IDS)
def test_context_matrix_rows_are_stable_and_not_edge_prone(case):
    """Every observation of the window finite and below 1e4, from reset and from the touched-down start; and the share of
    lane-steps whose contact hash or `terminated` flips when the start state is rounded to float32 -- the lane-steps the
    GPU comparison would have to exclude -- at most a third of the GPU cap."""
    inp = K.ctx_inputs(case)
    for touched in ([False, True] if inp.touch else [False]):
        edge = 0
        for snap, act, obs, rew, term, sig, _, _ in K.oracle_trajectory(inp, touched):
            assert np.isfinite(obs).all() and np.abs(obs).max() < 1e4 and np.isfinite(rew).all(), (case, touched)
            _, _, te, h, _ = K.restep(inp, snap, act, state=snap["state"].astype(np.float32).astype(np.float64))
            edge += int(((h != sig) | (te != term)).sum())
        share = edge / (inp.n * inp.steps)
        print(f"{case.label} touched={touched}: edge-prone share {share:.2e}")
        assert share <= K.ctx_bars(case)[2] / 3, (case, touched, share)


@pytest.mark.parametrize("case", [c for c in K.CTX_CASES if c.flags & FP32], ids=str)
def test_f32_light_mass_amplification_is_what_the_oracle_measures(case):
    inp = K.ctx_inputs(case)
    new, nominal = K.f32_start_deviation(inp, inp.rows), K.f32_start_deviation(inp, K.nominal_mass_rows(inp))
    r99, rmax = new[0] / nominal[0], new[1] / nominal[1]
    print(f"{case.label}: new rows p99 {new[0]:.3e} max {new[1]:.3e} | nominal p99 {nominal[0]:.3e} max {nominal[1]:.3e} | "
          f"R p99 {r99:.3f} max {rmax:.3f}")
    want = K.F32_LIGHT_MASS_AMPLIFICATION[case.label]
    assert abs(want[0] - r99) <= 0.2 * r99 and abs(want[1] - rmax) <= 0.2 * rmax, (case, r99, rmax)


def _copy_sys(s):
    return type(s).from_buffer_copy(s)


def _context_faults(inp):
    """The faults a wrong `load_ctx` could have, as changes to what the oracle is given: {name: (keyword arguments of
    `K.restep` for a snapshot, affected rows [n_ctx] bool or None: every row)}"""
    s, names, rows = inp.sys, inp.names, inp.rows
    cm = s.ctx
    M = cm.n_mass
    ratio, eff, n_light = K.mass_ratios(s, rows)
    faults = {}
    for a, b in ([(0, 1)] if M >= 2 else []) + ([(M - 2, M - 1)] if M >= 4 else []):  # a wrong link index
        t = _copy_sys(s)
        t.ctx.mass_link[a], t.ctx.mass_link[b] = cm.mass_link[b], cm.mass_link[a]
        faults[f"mass columns {a} and {b} swapped"] = (dict(sys_table=t), eff[:, a] != eff[:, b])
    t = _copy_sys(s)
    for k in range(M):
        t.ctx.mass_ratio_floor[k] = t.ctx.mass_ratio_floor_multi[k] = 0.0
    faults["floors zeroed"] = (dict(sys_table=t), (eff != ratio).any(1))
    if M >= 2:
        t = _copy_sys(s)
        for k in range(M):
            t.ctx.mass_ratio_floor_multi[k] = cm.mass_ratio_floor[k]
        single = np.array([cm.mass_ratio_floor[k] for k in range(M)], np.float32)
        faults["combined floor replaced by the single one"] = (
            dict(sys_table=t), (n_light >= 2) & (np.maximum(ratio, single) != eff).any(1))
    faults["previous context of the lane"] = (dict(ctx_shift=-K.CTX_STRIDE), None)
    for name in ("ang_damping", "elasticity", "joint_stiffness"):
        if name in names:
            r = rows.copy()
            r[:, names.index(name)] = inp.default[names.index(name)]
            faults[f"{name} at its default"] = (dict(rows=r), None)
    return faults


# (case, fault) pairs that do not reach 100 x the bar on a tenth of the affected lane-steps: the multiple of the bar they
# must still reach there (about 0.8 x the measured one; 0: the fault cannot move the model at all), and the reason.
# (Ant and the one-leg Ant have one mass feature: no columns to swap and never two light links, so those two faults do not
# exist for them.)
NO_CONTACT = "no collision spheres: elasticity enters through ground contact alone"
F32_BAR_IS_WIDE = ("the float32 bar is 20 to 29 times the float64 one; the fault moves an env step by a few per cent of a "
                   "velocity at most (ang_damping: |d ang_damping| dt n_frames <= 2.3 % of an angular velocity), which is "
                   "this multiple of the bar, measured -- the float64 case of the same model reaches 100 x")
CANNOT_MOVE = {
    ("multi", "elasticity at its default"): (0, NO_CONTACT),
    ("task", "elasticity at its default"): (0, NO_CONTACT),
    ("multi_f32", "elasticity at its default"): (0, NO_CONTACT),
    ("lean_f32", "ang_damping at its default"): (30, F32_BAR_IS_WIDE),            # measured 38
    ("planar_f32", "ang_damping at its default"): (5, F32_BAR_IS_WIDE),           # 6.2
    ("multi_f32", "ang_damping at its default"): (18, F32_BAR_IS_WIDE),           # 23
    ("generic_f32", "ang_damping at its default"): (5, F32_BAR_IS_WIDE),          # 7.0
    ("cheetah_half_f32", "ang_damping at its default"): (16, F32_BAR_IS_WIDE),    # 21
    ("ant_f32", "ang_damping at its default"): (55, F32_BAR_IS_WIDE),             # 69
    ("humanoid_f32", "ang_damping at its default"): (6, F32_BAR_IS_WIDE),         # 7.8: no float64 Humanoid case here
    ("humanoid_stiff_f32", "ang_damping at its default"): (6, F32_BAR_IS_WIDE),   # 7.5
    ("planar_f32", "elasticity at its default"): (18, F32_BAR_IS_WIDE),           # 23
    ("generic_f32", "elasticity at its default"): (21, F32_BAR_IS_WIDE),          # 27
    ("humanoid_f32", "elasticity at its default"): (48, F32_BAR_IS_WIDE),         # 60
    ("humanoid_stiff_f32", "elasticity at its default"): (68, F32_BAR_IS_WIDE),   # 85
    ("planar_f32", "mass columns 2 and 3 swapped"): (74, F32_BAR_IS_WIDE),        # 93 (columns 0 and 1: above 100)
}


@pytest.mark.parametrize("case", K.CTX_CASES, ids=CTX_IDS)
def test_the_oracle_moves_far_past_the_bar_under_every_context_fault(case):
    """What shows that the GPU comparison on these inputs would notice a wrong `load_ctx`: with each fault injected into
    the ORACLE's inputs, at least 10 % of the affected lane-steps of the window move by more than 100 x the case's bar
    (the GPU test fails on ONE agreeing lane-step above 1 x the bar)."""
    inp = K.ctx_inputs(case)
    traj = K.oracle_trajectory(inp, inp.touch)
    bar = K.ctx_bars(case)[0]
    short = []
    for name, (kw, rows_hit) in _context_faults(inp).items():
        kw = dict(kw)
        shift = kw.pop("ctx_shift", 0)
        dist = []
        for snap, act, obs, rew, _, sig, _, _ in traj:
            idx = snap["ctx_idx"]
            o, r, _, _, _ = K.restep(inp, snap, act, ctx_idx=(idx + shift) % K.CTX_N_CTX if shift else None, **kw)
            hit = np.ones(inp.n, bool) if rows_hit is None else rows_hit[idx]
            if name.startswith("elasticity"):
                hit = hit & (sig != 0)  # a contact impulse was delivered
            dist.append(K.moved(o, r, obs, rew)[hit])
        dist = np.concatenate(dist)
        reach = float(np.percentile(dist, 90)) / bar if dist.size else 0.0  # a tenth of the lane-steps move further
        print(f"{case.label}: {name}: {dist.size} affected lane-steps, a tenth of them move by more than {reach:.3g} x the "
              f"bar ({bar:.2e}); {int((dist > 100 * bar).sum())} by more than 100 x")
        need = CANNOT_MOVE.get((case.label, name), (100.0, ""))[0]
        if reach < need or (need and dist.size < 0.02 * inp.n * inp.steps):
            short.append((name, dist.size, reach))
    assert not short, (case, short)
