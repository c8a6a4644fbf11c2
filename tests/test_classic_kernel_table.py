"""The classic-control kernel instance table (tests/classic_kernel_cases.py) against carl_amd.hip's source and against
the library's own launch rule (carl_rollout_plan_io) -- host-side: no GPU.

* the instances `staged_kernel`, the CARL_LAUNCH dispatch, `launch_reset` and `launch_pair` can launch are read off
  the source (every entry must be readable);
* every case's plan, asked of the library with host-made structs, names exactly the instance the case claims;
* the instances the cases reach are the instances the source holds, minus the explicit unreachable list (int64
  actions for the Box families), whose refusal is asserted through the API.

A kernel added without a case, or a rule change that reroutes a case, fails here.  The module also re-steps every
rollout case's inputs with the oracle's float32 variant against its float64 variant (the matrix's inputs stay inside
the re-step helper's threshold-edge cap before they go to a GPU) and measures the AcrobotFast bar.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import classic_kernel_cases as K
from carl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "carl_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _family_traits():
    """{family type: (discrete, has a DEEP threshold, dense done path)} read off classic_control.hip.h"""
    src = _read("classic_control.hip.h")
    assert "using Acrobot = AcrobotT<double>;" in src and "using AcrobotFast = AcrobotT<float>;" in src
    heads = [(m.start(), m[1]) for m in re.finditer(r"^struct (\w+) \{", src, re.M)]
    traits = {}
    for i, (pos, name) in enumerate(heads):
        body = src[pos: heads[i + 1][0] if i + 1 < len(heads) else len(src)]
        action = re.search(r"using Action = (int|float);", body)
        if action is None:
            continue
        traits[name] = (action[1] == "int", re.search(r"kDeepBelowLanes = [1-9]", body) is not None,
                        re.search(r"kDenseDone = true", body) is not None)
    traits["Acrobot"] = traits["AcrobotFast"] = traits.pop("AcrobotT")
    assert sorted(traits) == sorted(K.FAMS), sorted(traits)
    dispatch = re.search(r"int with_classic_family\(.*?\n\}", src, re.S)[0]
    assert sorted(set(re.findall(r"fn\(carl::(\w+)\{\}\)", dispatch))) == sorted(K.FAMS)
    return traits


def _instantiated():
    """every kernel instance carl_amd.hip can launch, as instance tuples, read off its source"""
    src = _read("carl_amd.hip")
    kinds = dict(re.findall(r"\b(kAct\w+) = (\d)", re.search(r"constexpr int kActU8[^;]*;", _read("engine_kernels.hip.h"))[0]))
    traits = _family_traits()
    found = []

    # ---- staged_kernel: CARL_STAGED / CARL_STAGED_01 lines under their `if constexpr` guards
    body = re.search(r"constexpr bool dense = carl::dense_done_of<Fam>::value, deep = carl::deep_below_lanes_of<Fam>::value > 0;"
                     r"(.*?)#undef CARL_STAGED_01", src, re.S)[1]
    body = re.sub(r"//[^\n]*", "", body)
    guards = {"std::is_same_v<typename Fam::Action, int>": 0, "deep": 1, "dense": 2}
    entries, stack = [], []  # entries: (guard list [(trait index, wanted)], both action widths, args)
    for line in filter(None, (ln.strip() for ln in body.split("\n"))):
        inline = []
        if line == "} else {":
            stack[-1] = (stack[-1][0], not stack[-1][1])
            continue
        if line == "}":
            stack.pop()
            continue
        m = re.match(r"if constexpr \((.+?)\) (\{|CARL_STAGED.*)$", line)
        if m:
            if m[2] == "{":
                stack.append((guards[m[1]], True))
                continue
            inline, line = [(guards[m[1]], True)], m[2]
        m = re.fullmatch(r"CARL_STAGED(_01)?\(([^)]*)\)", line)
        assert m, f"a line of staged_kernel this test cannot read: {line!r}"
        args = [a.strip() for a in m[2].split(",")]
        entries.append((stack + inline, bool(m[1]), args))
    assert not stack and len(entries) == len(re.findall(r"CARL_STAGED(?:_01)?\(", body)) and len(entries) == 15
    for fam in K.FAMS:
        for cond, both, args in entries:
            if all(traits[fam][i] == want for i, want in cond):
                aks = [0, 1] if both else [int(kinds.get(args[0].replace("carl::", ""), args[0]))]
                flags = [bool(int(a)) for a in (args if both else args[1:])]
                assert len(flags) == 6
                found += [("staged", fam, ak, *flags) for ak in aks]

    # ---- per-call step and direct-store rollout: the four-way CARL_LAUNCH
    launch = re.search(r"#define CARL_LAUNCH\(KERNEL, \.\.\.\)(.*?)while \(0\)", src, re.S)[1]
    four = re.findall(r"carl::KERNEL<Fam, (true|false), (true|false)>", launch)
    assert len(four) == launch.count("hipLaunchKernelGGL") == 4 and len(set(four)) == 4
    uses = re.findall(r"CARL_LAUNCH\((\w+),", src.split("while (0)")[1])
    assert uses == ["step_kernel", "rollout_kernel"]
    for kind in ("step", "direct"):
        found += [(kind, fam, lds == "true", a64 == "true") for fam in K.FAMS for lds, a64 in four]

    # ---- reset
    reset = re.search(r"int launch_reset\(.*?\n\}", src, re.S)[0]
    two = re.findall(r"carl::reset_kernel<Fam, (true|false)>", reset)
    assert sorted(two) == ["false", "true"] and reset.count("hipLaunchKernelGGL") == 2
    found += [("reset", fam, lds == "true") for fam in K.FAMS for lds in two]

    # ---- pair: Acrobot + each family of carl_rollout_pair's switch; ARB only for a dense-done second family
    pair = re.search(r"int launch_pair\(.*?\n\}", src, re.S)[0]
    assert "using FamA = carl::Acrobot;" in pair
    inst = re.findall(r"rollout_staged_pair_kernel<FamA, FamB, (true|false), (true|false)>", pair)
    assert inst == [("false", "false"), ("false", "true")]
    assert re.search(r"if constexpr \(carl::dense_done_of<FamB>::value\) \{\s*if \(pb\.ar\) kern = [^;]*false, true>\);", pair)
    seconds = re.findall(r"return launch_pair<carl::(\w+)>", src)
    assert len(seconds) == 4 and len(src.split("launch_pair<")) == 5
    found += [("pair", f, False) for f in seconds] + [("pair", f, True) for f in seconds if traits[f][2]]
    assert len(set(found)) == len(found)
    return found


def _count(instances, kind):
    return sum(1 for i in instances if i[0] == kind)


def test_the_source_holds_the_counted_instances():
    inst = _instantiated()
    assert [_count(inst, k) for k in ("staged", "step", "direct", "reset", "pair")] == [60, 24, 24, 12, 5]
    assert len(K.UNREACHABLE) == 14 and set(K.UNREACHABLE) <= set(inst)


@pytest.mark.parametrize("case", K.CASES, ids=str)
def test_every_case_takes_the_instance_it_names(case):
    b, io = case.host_batch_io()
    plan = K.plan_of(b, io)
    assert K.instance_of(case, plan) == case.instance, (case, [(k, getattr(plan, k)) for k, _ in plan._fields_])
    if case.kind == "step":
        assert plan.step_block == K.STEP_BLOCK[case.label.split("-")[2]]
    if case.kind in ("staged", "direct"):
        want = _lib.ROLLOUT_STAGED if case.kind == "staged" else (
            _lib.ROLLOUT_DIRECT_FLAG if case.direct else _lib.ROLLOUT_DIRECT_SHAPE)
        assert plan.variant == want == _lib.load().carl_rollout_variant_io(C.byref(b), C.byref(io))
        assert bool(plan.lean) == (case.selector == K.STATIC and not case.fin and not case.final_obs and case.kind == "staged")
        # the rollout's lane count is ragged: a partial last workgroup and, but for rows of a wider array, n % 16 != 0
        assert case.n % 256 and (case.n % 16 or case.layout == "wide")
    if case.kind == "staged":
        assert plan.lds_bytes > 0 and (plan.lds_bytes <= 160 * 1024)


def test_the_cases_reach_every_instance_but_the_unreachable_ones():
    inst = _instantiated()
    reached = {c.instance for c in K.CASES} | {i for _, _, i in K.PAIR_CASES}
    assert reached == set(inst) - set(K.UNREACHABLE)
    assert len(reached) == 111
    # a class of rollout instances sees T in {1, 9, 37} and a T that is neither a multiple of 8 nor of 4
    for fam in K.FAMS:
        assert {1, 9, 37} <= {c.T for c in K.ROLLOUT_CASES if c.fam == fam}, fam


@pytest.mark.parametrize("fam_b,auto_b,instance", K.PAIR_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else "")
def test_every_pair_case_takes_the_instance_it_names(fam_b, auto_b, instance):
    a, b = K.pair_parts(fam_b, auto_b)
    pa, pb = K.plan_of(*a.host_batch_io()), K.plan_of(*b.host_batch_io())
    assert K.pair_instance_of(pa, pb, fam_b) == instance
    assert a.n != b.n and a.T % 4 and a.T == b.T


@pytest.mark.parametrize("instance", K.UNREACHABLE, ids=str)
def test_the_unreachable_instances_are_refused_through_the_api(instance):
    """int64 actions for a Box family: carl_step / carl_rollout say CARL_ERR_INVALID_ARGUMENT before anything is
    launched (validate_io), in the configuration that would otherwise take the instance"""
    lib = _lib.load()
    kind, fam = instance[0], instance[1]
    if kind == "staged":
        _, _, ak, plain, ldsctx, *_ = instance
        case = K.Case("staged", fam, instance, dtype="i64", n_ctx=K.C_LDS if ldsctx or plain else K.C_GLOBAL,
                      selector=K.STATIC if plain else K.RR)
    else:
        case = K.Case(kind, fam, instance, dtype="i64", n_ctx=K.C_LDS if instance[2] else K.C_GLOBAL, selector=K.RR,
                      direct=kind == "direct")
    b, io = case.host_batch_io()
    # the rule itself would route the launch to the instance ...
    assert K.instance_of(case, K.plan_of(b, io)) == instance
    # ... and the argument check in front of it refuses the dtype
    rc = lib.carl_step(C.byref(b), C.byref(io), None) if kind == "step" else lib.carl_rollout(C.byref(b), C.byref(io), 9, None)
    assert rc == _lib.ERR_INVALID_ARGUMENT and b"continuous family needs float32" in lib.carl_last_error()


def test_plan_query_validates_its_arguments():
    lib = _lib.load()
    p = _lib.RolloutPlan()
    b, io = K.CASES[0].host_batch_io()
    assert lib.carl_rollout_plan_io(None, C.byref(io), C.byref(p)) == -1 and b"NULL" in lib.carl_last_error()
    assert lib.carl_rollout_plan_io(C.byref(b), C.byref(io), None) == -1
    assert lib.carl_rollout_plan_io(C.byref(b), None, C.byref(p)) == 0 and p.variant == _lib.ROLLOUT_DIRECT_SHAPE  # dense rows
    b.n_contexts = 0
    assert lib.carl_rollout_plan_io(C.byref(b), C.byref(io), C.byref(p)) == -1 and b"n_contexts" in lib.carl_last_error()
    b.n_contexts, b.family = 4, -1
    assert lib.carl_rollout_plan_io(C.byref(b), C.byref(io), C.byref(p)) == -1 and b"classic-control" in lib.carl_last_error()
    b.family, io.row_pitch = 0, 16
    assert lib.carl_rollout_plan_io(C.byref(b), C.byref(io), C.byref(p)) == -1 and b"row_pitch" in lib.carl_last_error()


# ---------------------------------------------------------------- the inputs, re-stepped on the CPU
FIVE = [c for c in K.ROLLOUT_CASES if not c.fp32]
REPRESENTATIVES = {c.group: c for c in reversed(FIVE)}  # (a group shares its inputs: one member speaks for it)


@pytest.mark.parametrize("case", list(REPRESENTATIVES.values()), ids=str)
def test_matrix_inputs_stay_inside_the_edge_flag_cap_on_the_float32_oracle(case):
    """the oracle's float32 variant, run over the case's inputs, re-stepped by its float64 variant with the matrix's own
    helper: within 1e-5 and at most 8 threshold-edge flags -- the inputs leave the kernels the same room"""
    from test_gpu_parity import restep_rollout_with_oracle

    _, acts = K.table_and_actions(case)
    s0, ctx, outs = K.oracle_rollout(case, "f32")
    done = (outs["terminated"] | outs["truncated"]) != 0
    assert int(done.sum()) >= case.n  # episodes end inside the window
    if not case.final_obs:
        del outs["final_obs"]
    rows, s_prev, a, flat, kept = K.flatten_rollout(case, s0, ctx, acts, outs)
    assert kept >= 0.75 * case.T * case.n  # (all of them with auto-reset)
    checked = restep_rollout_with_oracle(case.family, rows, s_prev, a, flat)
    assert checked >= kept - (0 if case.final_obs else int(done.sum())) - 8


def acrobot_fast_f32_deviation():
    """worst rel_err of the oracle's float32 Acrobot from its float64 one over every AcrobotFast input of the matrix:
    each (context, state, action) the float32 variant visits in the rollout cases, and the step cases' rows"""
    from oracle import oracle as O
    from test_gpu_parity import rel_err, state_from_obs

    worst = 0.0
    seen = set()
    for case in K.CASES:
        if not case.fp32 or case.kind == "reset" or case.group in seen:
            continue
        seen.add(case.group)
        if case.kind == "step":
            table, idx, s, a = K.step_inputs(case)
            rows, states, actions = table[idx], s.astype(np.float64), a
            g_s, g_obs, g_rew, _ = O.transitions(O.ACROBOT, rows, s, a, precision="f32")
        else:
            _, acts = K.table_and_actions(case)
            s0, ctx, outs = K.oracle_rollout(case, "f32")
            T, n = acts.shape
            prev = [s0] + [state_from_obs(O.ACROBOT, outs["obs"][t]) for t in range(T - 1)]
            rows, states, actions = ctx.reshape(T * n, -1), np.concatenate(prev), acts.reshape(-1)
            done = ((outs["terminated"] | outs["truncated"]) != 0).reshape(-1)
            g_obs = np.where(done[:, None], outs["final_obs"].reshape(T * n, -1), outs["obs"].reshape(T * n, -1))
            g_rew, g_s = outs["reward"].reshape(-1), None
        w_s, w_obs, w_rew, _ = O.transitions(O.ACROBOT, rows, states, actions, precision="f64")
        e = max(float(rel_err(g_obs, w_obs).max()), float(rel_err(g_rew, w_rew).max()))
        if g_s is not None:
            e = max(e, float(rel_err(g_s, w_s).max()))
        worst = max(worst, e)
    return worst


def test_acrobot_fast_bar_comes_from_the_float32_oracle_on_the_matrix_inputs():
    worst = acrobot_fast_f32_deviation()
    print(f"AcrobotFast: float32 oracle vs float64 oracle over the matrix's inputs: worst rel_err {worst:.3e}")
    # the recorded deviation is the measured one (to the three digits it is written with), the bar follows from it
    assert abs(worst - K.ACROBOT_FAST_F32_DEVIATION) <= 0.005 * K.ACROBOT_FAST_F32_DEVIATION + 1e-12, worst
    assert K.ACROBOT_FAST_BAR == max(5e-5, 3 * K.ACROBOT_FAST_F32_DEVIATION)
