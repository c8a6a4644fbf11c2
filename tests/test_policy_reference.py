"""The host reference of the closed-loop policy (oracle/carl_oracle.c: oracle_policy_forward), checked on the CPU: its fma
is libm's correctly rounded fmaf (including where a product-then-add or a float64-then-float32 evaluation rounds
differently), its fp32 forward pass stays within its own error bound of a float64 one over the shape matrix the GPU
suite launches, and it reads MLPPolicy's packed layout -- every set of a stack and the shift / scale / clip tail.
Also the host-side refusal of a summary without auto-reset (include/carl_amd.h: carl_rollout_policy)."""
import ctypes as C

import numpy as np
import pytest

from carl_amd import _lib
from carl_amd.engine import VecEngine
from carl_amd.policy import MLPPolicy
from oracle import oracle as O
from policy_cases import ACTS, HIDDEN_SHAPES, c_batch, forward64


def _libm_fmaf():
    m = C.CDLL("libm.so.6")
    m.fmaf.restype = C.c_float
    m.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
    return m.fmaf


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_fma_is_libm_fmaf_bit_for_bit():
    rng = np.random.default_rng(0)
    f32 = np.float32
    tiny = np.finfo(np.float32).smallest_subnormal
    a, b, c = [], [], []
    # random magnitudes over most of the exponent range, both signs
    for _ in range(3000):
        a.append(rng.normal() * 2.0 ** rng.integers(-60, 60))
        b.append(rng.normal() * 2.0 ** rng.integers(-60, 60))
        c.append(rng.normal() * 2.0 ** rng.integers(-120, 120))
    # c = -fl(a * b): the fma returns the product's rounding error, a product-then-add returns 0
    ra, rb = rng.normal(size=500).astype(f32), rng.normal(size=500).astype(f32)
    a += list(ra)
    b += list(rb)
    c += list(-(ra * rb))
    # (1 + i 2^-12)(1 + j 2^-12), i and j odd: the exact product ends in 2^-24, a float32 midpoint.  With c a nudge below
    # float64 resolution, the float64 sum rounds back onto the midpoint and the cast then rounds it to even -- half of
    # the time the wrong way; the fma rounds once, the right way
    for i in range(1, 32, 2):
        for j in range(1, 32, 2):
            for nudge in (2.0 ** -80, -(2.0 ** -80)):
                a.append(1 + i * 2.0 ** -12), b.append(1 + j * 2.0 ** -12), c.append(nudge)
    a += [1 + 2.0 ** -12] * 2
    b += [1 + 2.0 ** -12] * 2
    c += [-1.0, -(1 + 2.0 ** -11)]
    # subnormal operands and results, signed zeros, infinities, NaN
    specials = [0.0, -0.0, tiny, -tiny, tiny * 3, 2.0 ** -126, -(2.0 ** -126), 1.0, -1.0, 2.0 ** -75, 2.0 ** 64,
                np.inf, -np.inf, np.nan]
    for x in specials:
        for y in specials:
            for z in specials[:8]:
                a.append(x), b.append(y), c.append(z)
    a, b, c = (np.asarray(v, np.float64).astype(np.float32) for v in (a, b, c))
    got = O.fmaf(a, b, c)
    libm = _libm_fmaf()
    want = np.array([libm(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(_bits(got)[~nan], _bits(want)[~nan])  # bits: -0 != +0 here
    # the triples are adversarial: both shortcut evaluations differ from the fma on some of them
    with np.errstate(all="ignore"):
        twice = a * b + c
        via64 = (a.astype(np.float64) * b + c).astype(np.float32)
    ok = ~nan & np.isfinite(want)
    assert (_bits(twice)[ok] != _bits(want)[ok]).sum() >= 400
    assert (_bits(via64)[ok] != _bits(want)[ok]).sum() >= 100
    # signed zeros: the exact sum is an exact zero -> +0 unless both addends are -0
    z = O.fmaf([-0.0, 0.0, -0.0, 1.0, -1.0], [1.0, -1.0, -1.0, 1.0, 1.0], [-0.0, -0.0, 0.0, -1.0, 1.0])
    assert list(np.signbit(z)) == [True, True, False, False, False]


def _policy(rng, family, widths, act, n_ctx, weight_scale=1.0, clip=None):
    info = _lib.family_info(family)
    D = int(info.obs_dim)
    n_out = int(info.n_actions) if info.action_is_discrete else 1
    dims = [n_ctx + D, *widths, n_out]
    layers = [((rng.normal(size=(o, i)) * weight_scale / np.sqrt(i)).astype(np.float32),
               rng.normal(size=o).astype(np.float32)) for i, o in zip(dims[:-1], dims[1:])]
    return MLPPolicy(family, D, list(range(n_ctx)), layers, act, input_shift=rng.normal(size=dims[0]),
                     input_scale=rng.uniform(0.2, 3.0, dims[0]), input_clip=clip)


# a linear policy has no activation: it is listed once
CASES = [((), "identity")] + [(w, a) for w in HIDDEN_SHAPES for a in ACTS]


@pytest.mark.parametrize("widths, act", CASES, ids=["x".join(map(str, w)) + "-" + a if w else "linear" for w, a in CASES])
def test_fp32_forward_is_within_its_bound_of_float64(widths, act):
    rng = np.random.default_rng(len(widths) * 100 + sum(widths) + ACTS.index(act))
    worst = 0.0
    for family, n_ctx, ws, clip in ((_lib.CARTPOLE, 8, 1.0, None), (_lib.PENDULUM, 0, 30.0, 2.5),
                                    (_lib.ACROBOT, 14, 3.0, 1.0), (_lib.MOUNTAINCAR_CONT, 3, 100.0, None)):
        pol = _policy(rng, family, widths, act, n_ctx, ws, clip)
        x = rng.normal(size=(2000, pol.n_in)) * rng.choice([0.01, 1.0, 30.0], size=(2000, 1))
        r = O.policy_forward(pol.params, pol.n_in, pol.widths, pol.n_out, act, x)
        x32 = x.astype(np.float32)
        np.testing.assert_allclose(r.y64, forward64(pol, x32), rtol=1e-10, atol=1e-12)
        err = np.abs(r.y32.astype(np.float64) - r.y64)
        assert np.all(err <= r.bound + 1e-12 * np.abs(r.y64)), (family, err.max(), r.bound.max())
        assert np.all(np.isfinite(r.bound))
        worst = max(worst, float((err / np.maximum(r.bound, 1e-300)).max()))
        first = np.argmax(r.y32, axis=1)  # numpy's argmax also takes the first maximum
        np.testing.assert_array_equal(r.action, first)
    assert worst <= 1.0
    print(f"{widths} {act}: largest |fp32 - float64| / bound = {worst:.3f}")


def test_tanh_saturates_exactly():
    pol = MLPPolicy(_lib.PENDULUM, 3, [], [(np.array([[100.0, 0, 0], [-100.0, 0, 0]], np.float32), np.zeros(2)),
                                           (np.array([[1.0, 2.0]], np.float32), np.zeros(1))], "tanh")
    r = O.policy_forward(pol.params, 3, [2], 1, "tanh", np.array([[1.0, 0, 0], [-1.0, 0, 0]]))
    np.testing.assert_array_equal(r.y32[:, 0], [1.0 - 2.0, -1.0 + 2.0])


def test_reads_every_set_of_a_stack_and_the_input_tail():
    rng = np.random.default_rng(5)
    for family, widths, act in ((_lib.CARTPOLE, (33, 7), "relu"), (_lib.MOUNTAINCAR, (), "identity"),
                                (_lib.PENDULUM, (5,), "tanh")):
        sets = [_policy(rng, family, widths, act, 2, clip=float(c)) for c in (0.5, 1.0, np.inf, 3.0, 2.0)]
        st = MLPPolicy.stack(sets, 256)
        x = rng.normal(size=(500, st.n_in)) * 4
        which = rng.integers(0, len(sets), 500)
        r = O.policy_forward(st.params, st.n_in, st.widths, st.n_out, act, x, which)
        for k, p in enumerate(sets):
            m = which == k
            np.testing.assert_allclose(r.y64[m], forward64(p, x[m].astype(np.float32)), rtol=1e-10, atol=1e-12)
            alone = O.policy_forward(p.params, p.n_in, p.widths, p.n_out, act, x[m])
            np.testing.assert_array_equal(r.y32[m], alone.y32)
        # the sets differ in every part of the block: the same inputs give different outputs under different sets
        a = O.policy_forward(st.params, st.n_in, st.widths, st.n_out, act, x[:50], np.zeros(50, np.int32)).y32
        b = O.policy_forward(st.params, st.n_in, st.widths, st.n_out, act, x[:50], np.full(50, 4, np.int32)).y32
        assert not np.array_equal(a, b)


def test_clip_shift_scale_and_nan_inputs():
    """x = min(max((v - shift) * scale, -clip), clip): a NaN (input NaN, or 0 * inf) becomes -clip"""
    layers = [(np.eye(3, dtype=np.float32), np.zeros(3, np.float32)), (np.zeros((1, 3), np.float32), np.zeros(1))]
    pol = MLPPolicy(_lib.PENDULUM, 3, [], layers, "identity", input_shift=[1, 0, 0], input_scale=[2, np.inf, 1],
                    input_clip=4.0)
    # first layer = identity: read the transformed inputs back through a head per unit
    for j in range(3):
        head = np.zeros((1, 3), np.float32)
        head[0, j] = 1
        p = MLPPolicy(_lib.PENDULUM, 3, [], [layers[0], (head, np.zeros(1))], "identity", input_shift=pol.shift,
                      input_scale=pol.scale, input_clip=4.0)
        x = np.array([[2.5, 0.0, np.nan], [-9.0, 1e-30, 3.0], [np.nan, -1.0, -7.0]], np.float32)
        y = O.policy_forward(p.params, 3, [3], 1, "identity", x).y32[:, 0]
        want = {0: [3.0, -4.0, -4.0], 1: [-4.0, 4.0, -4.0], 2: [-4.0, 3.0, -4.0]}[j]
        np.testing.assert_array_equal(y, want)


def test_summary_without_auto_reset_is_refused():
    # C: refused before anything is enqueued (the batch's device pointers are never dereferenced)
    lib = _lib.load()
    b = c_batch(flags=0)
    pol = _policy(np.random.default_rng(0), _lib.CARTPOLE, (8,), "tanh", 2)
    p = pol.struct(1000, 0x2000)
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), None, 10, C.byref(summ), None) == _lib.ERR_UNSUPPORTED
    assert b"CARL_FLAG_AUTORESET" in lib.carl_last_error()
    assert lib.carl_last_error() == (
        b"carl_rollout_policy: a summary needs CARL_FLAG_AUTORESET (without auto-reset a finished lane reports done on "
        b"every later step, and its episode would be counted on each of them)")
    # the last check of all: a policy without params is refused for that, with or without the flag
    p.params = None
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), None, 10, C.byref(summ), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == b"carl_rollout_policy: params is NULL"
    p.params = 0x2000
    for n_steps, n_lanes in ((0, 1000), (10, 0)):  # (the no-step shortcut too)
        b.n_lanes = n_lanes
        assert lib.carl_rollout_policy(C.byref(b), C.byref(p), None, n_steps, C.byref(summ), None) == _lib.ERR_UNSUPPORTED
    # Python: the same decision before any upload
    eng = object.__new__(VecEngine)
    info = _lib.family_info(_lib.CARTPOLE)
    eng.family, eng.D, eng.n, eng.info, eng.b = _lib.CARTPOLE, 4, 1000, info, _lib.Batch()
    eng.b.flags = 0
    with pytest.raises(ValueError, match="auto_reset"):
        eng.rollout_policy(pol, 10, mode="summary")
