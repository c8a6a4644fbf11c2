"""Host half of the device math primitives' tests (tests/math_primitive_cases.py; the device half is
tests/test_gpu_math_primitives.py): every math function of the three headers has a case, each case's recorded E_host is
the restatement's measured error, the longdouble reference agrees with mpmath, and the inputs hold the edges they claim."""
import os
import re

import numpy as np
import pytest

import math_primitive_cases as M

IDS = [c.name for c in M.CASES]


def test_every_header_primitive_has_a_case():
    found = M.header_primitives()
    assert len(found) >= 25, sorted(found)  # (the parser still reads the headers)
    covered = {x for c in M.CASES for x in c.covers}
    missing = found - covered - set(M.NOT_PRIMITIVES)
    assert not missing, f"device math functions without a case in tests/math_primitive_cases.py: {sorted(missing)}"
    stale = (covered | set(M.NOT_PRIMITIVES)) - found
    assert not stale, f"cases name functions the headers no longer have: {sorted(stale)}"
    assert set(M.E_HOST) == set(IDS)
    # every case's entry point exists in the probe's source
    probe = open(os.path.join(M.ROOT, "tests", "probe", "math_probe.hip")).read()
    entries = set(re.findall(r"^ENTRY_\w+\((\w+)", probe, re.M)) | set(re.findall(r'extern "C" int probe_(\w+)\(', probe))
    assert {c.entry for c in M.CASES} <= entries, {c.entry for c in M.CASES} - entries
    # the table kernels are launched with the workgroup sizes the product uses
    eng = open(os.path.join(M.CSRC, "engine_kernels.hip.h")).read()
    lanes = int(re.search(r"constexpr int kRolloutLanes = (\d+);", eng).group(1))
    assert re.search(r"constexpr int kRolloutThreads = kRolloutLanes \+ kWave;", eng) and lanes + 64 in M.TAB_BLOCKS


@pytest.mark.parametrize("case", M.CASES, ids=IDS)
def test_e_host_constants_are_the_measured_ones(case):
    worst = case.e_host()
    print(f"{case.name}: E_host {worst:.3e} ({case.measure}) over {case.inputs()[0].shape[0]} inputs")
    # the recorded figure is the measured one (to the digits it is written with); the device bar follows from it
    assert abs(worst - M.E_HOST[case.name]) <= 0.005 * M.E_HOST[case.name], worst


@pytest.mark.parametrize("case", [c for c in M.CASES if c.mp], ids=[c.name for c in M.CASES if c.mp])
def test_longdouble_reference_agrees_with_mpmath(case):
    """at the case's special points (the guards and their neighbours, 0, subnormals, 1, the extremes: indexed explicitly),
    at its largest arguments (where a libm's argument reduction would go wrong first) and on a random sample; non-finite
    inputs must give NaN"""
    import mpmath as mp

    ins, ref = case.inputs(), case.reference()
    n = ins[0].shape[0]
    finite = np.all([np.isfinite(a) for a in ins], axis=0)
    order = np.argsort(-np.max([np.abs(np.where(finite, a, 0)) for a in ins], axis=0))
    special = M.special_indices(case)
    assert special.size >= 3 or case.name.endswith("_wide"), (case.name, special.size)  # (the wide table case is sweeps only)
    idx = np.unique(np.concatenate([special[:400], order[:60], np.random.default_rng(3).integers(0, n, 240)]))
    idx = idx[finite[idx]]
    if case.mp == "atan2":  # mpmath has no signed zero: the axis points are IEEE's convention, checked on the device
        idx = idx[(ins[0][idx] != 0) & (ins[1][idx] != 0)]
    want = M.mp_reference(case, idx)
    eps = 2.0 ** -63
    for j, i in enumerate(idx):
        for o, w in zip(ref, want[j]):
            hi = float(o[i])
            got = mp.mpf(hi) + mp.mpf(float(o[i] - M.L(hi)))  # longdouble -> mpf, exactly: two doubles
            assert abs(got - w) <= 2 * eps * max(abs(w), mp.mpf(2) ** -1000), (case.name, [float(a[i]) for a in ins], float(o[i]))
    if case.mp in ("sincos", "sincos2", "cos", "cos2"):
        assert all(np.isnan(o[~finite]).all() for o in ref)


def test_inputs_hold_the_edges_they_claim():
    f32, f64 = np.float32, np.float64
    (x,) = M.BY_NAME["sincos_fast_f32"].inputs()
    s = set(x.view(np.uint32).tolist())

    def has(v, dt=f32, pool=s):
        return int(np.asarray(v, dt).view(np.uint32 if dt == f32 else np.uint64)) in pool

    for v in (1e5, np.nextafter(f32(1e5), f32(0)), np.nextafter(f32(1e5), f32(np.inf)), 0.78, np.nextafter(f32(0.78), f32(1)),
              np.nextafter(f32(0.78), f32(0)), 0.0, -0.0, 1.17549435e-38, 1e-45, 3e38, np.inf, -np.inf):
        assert has(v) and has(-f32(v)), v
    assert np.isnan(x).any()
    k = np.arange(1, 63662)
    near = (k.astype(M.L) * (M.PI / 2)).astype(f32)
    assert all(has(v) for v in near[:: 997]) and has(near[-1]) and has(np.nextafter(near[-1], f32(0)))
    # ties: x 2 / pi within an ulp of a half-integer, all the way to the guard
    y = x[np.isfinite(x) & (np.abs(x) <= 1e5)].astype(f64) * (2 / np.pi)
    frac = np.abs(y - np.floor(y) - 0.5)
    tie = frac <= np.spacing(np.abs(y).astype(f32)).astype(f64)
    assert tie.sum() > 120000 and np.abs(y[tie]).max() > 63000
    for name in ("sincos_fast_pk", "sincos_fast_smallarg", "cos_fast"):
        assert np.array_equal(M.BY_NAME[name].inputs()[0].view(np.uint32), x.view(np.uint32))
    (d,) = M.BY_NAME["sincos_fast_f64"].inputs()
    assert np.isnan(d).any() and np.isinf(d).any() and (np.abs(d[np.isfinite(d)]) > 1e6).sum() > 1000 and (d == 1e6).any()
    assert np.abs(M.BY_NAME["sincos_fast_f64_nofallback"].inputs()[0]).max() == 1e6
    xa, xb = M.BY_NAME["SinCosTab_sincos2"].inputs()
    grid = (np.arange(-1024, 1025).astype(M.L) * (M.PI / 256)).astype(f64)
    pool = set(xa.view(np.uint64).tolist())
    assert all(has(g, f64, pool) and has(np.nextafter(g, np.inf), f64, pool) and has(np.nextafter(g, -np.inf), f64, pool) for g in grid)
    assert (xa < 0).sum() > 50000 and np.abs(xa).max() <= 40 and set(xb.view(np.uint64).tolist()) == pool
    assert np.abs(M.BY_NAME["SinCosTab_sincos2_wide"].inputs()[0]).max() > 9e3
    (r,) = M.BY_NAME["rcp_fast"].inputs()
    assert r.min() < -1e289 and r.max() > 1e289 and np.abs(r).min() < 1e-289 and np.isfinite(r).all() and (r != 0).all()
    (h,) = M.BY_NAME["cos_twice_fast"].inputs()
    assert np.isnan(h).any() and (np.abs(h[np.isfinite(h)]) > 5e4).any() and (h == f32(1.85)).any() and (h == np.nextafter(f32(1.85), f32(2))).any()
    for name in ("atan2_fast", "atan2_f64"):
        y, x = M.BY_NAME[name].inputs()
        for sy in (0.0, -0.0):
            for sx in (0.0, -0.0, -1.0):
                assert ((y == 0) & (np.signbit(y) == np.signbit(sy)) & (x == sx) & (np.signbit(x) == np.signbit(sx))).any()
        assert ((np.abs(y) == np.abs(x)) & (x != 0)).sum() >= 4000 and ((x == 0) & (y != 0)).any()
        for q in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            assert ((np.sign(y) == q[0]) & (np.sign(x) == q[1])).sum() > 10000
        assert np.abs(y[y != 0]).min() < 1e-29 and np.abs(y).max() > 1e29
    assert (M.BY_NAME["atan2_f64_xpos"].inputs()[1] >= 0).all() and not np.signbit(M.BY_NAME["atan2_f64_xpos"].inputs()[1]).any()
    (q,) = M.BY_NAME["sqrt01_f64"].inputs()
    assert (q == 0).any() and (q == 1).any() and (q == 1 - 2.0 ** -53).any() and ((q > 0) & (q < 2.3e-308)).any()
    assert (q == np.nextafter(1e-30, 1)).any() and (q == np.nextafter(1e-30, 0)).any() and q.min() >= 0 and q.max() <= 1
    for name, dt in (("asin_f64", f64), ("asin_r_f32", f32)):
        (a,) = M.BY_NAME[name].inputs()
        one = dt(1)
        assert all((a == v).any() for v in (one, -one, np.nextafter(one, dt(0)), -np.nextafter(one, dt(0)), dt(0))) and np.abs(a).max() == 1
    a, b = M.BY_NAME["div_fast"].inputs()
    qq = np.abs(a.astype(f64) / b.astype(f64))
    assert qq.min() >= 1e-30 * 0.99 and qq.max() <= 1e30 * 1.01 and (a < 0).any() and (b < 0).any() and qq.min() < 1e-25 and qq.max() > 1e25
    k, ang = M.BY_NAME["qaxis"].inputs()
    assert set(k.tolist()) == {0, 1, 2} and ang.min() < -12.5 and ang.max() > 12.5
