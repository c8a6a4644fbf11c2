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
