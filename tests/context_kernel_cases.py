"""Named configurations for the device context sampler and verifier (carl_amd/csrc/context_kernels.hip.h:
`sample_contexts_kernel`, `verify_contexts_kernel`, reached through `carl_sample_contexts` / `carl_verify_contexts`).

A case is a list of `carl_feature_spec_t` built directly -- not through CARL feature objects, so edges the Python
layer refuses are still reachable -- with `(n_contexts, ctx_stride, context_offset, seed)`.  tests/
test_context_kernel_table.py holds the table against the oracle (oracle/context_sampler.c) on the host: every branch a
case claims is reached by the oracle's trace, the extreme-draw ids are what they say, the recorded deviations are the
measured ones.  tests/test_gpu_context_kernel_matrix.py runs every case on the device against the oracle.

Branches (`Case.reaches`): linear, log, int, categorical, constant, normal0 (accepted at attempt 0), normal8 (accepted
at an attempt >= 8), exhausted (all 32 attempts out of bounds: the last candidate, clipped).

Bars.  CONSTANT, linear UNIFORM_FLOAT, UNIFORM_INT, CATEGORICAL, sigma = 0 and always-exhausted normals are the same
float32 expressions on both sides: bit-exact.
  log-uniform: relative error <= max(3e-6, 4 x D_log); D_log[case] is the worst relative deviation of a float32 NumPy
    evaluation of the kernel's expression from the oracle's double one over that case's draws (one logf and one expf
    of the host's libm; the factor 4 is for the device's differing from them by a couple of ulp each).
  normal: |got - want| <= sigma x max(4.5e-6, 4 x D_z) + 2 ulp32(max(|mu|, |want|)); D_z[case] is the worst
    |z32 - z64| of a float32 NumPy evaluation of sqrt(-2 log(1 - u1)) cos(2 pi u2) over the attempts the case draws.
  An accept / reject decision may go the other way where a candidate lies within the bar of a bound: the oracle's
  result under both decisions at the first such attempt is accepted, for at most 1 entry in 1000 of a case
  (`flip_cap`); the seeds are such that the oracle's trace has none (asserted on the host).

The context ids of EXTREME_U0 / EXTREME_UTOP were found once with `oracle.scan_u(99, 0, 0, 2**27)`: the first draw of
feature row 0 under seed 99 is u = 0 / u = 1 - 2^-24 there (for a NORMAL_FLOAT row that is its u1, so the second is
also the largest |z| an attempt can reach).
"""
import functools

import numpy as np

from carl_amd import _lib
from carl_amd.context.context_space import (
    CategoricalContextFeature,
    ContextSpace,
    NormalFloatContextFeature,
    UniformFloatContextFeature,
    UniformIntegerContextFeature,
)
from oracle import oracle as O

# ---- the configuration of tests/test_device_sampler.py and tests/test_gpu_device_sampler.py (CARL feature objects)
SPACE = ContextSpace({
    "gravity": UniformFloatContextFeature("gravity", lower=0.1, upper=np.inf, default_value=9.8),
    "length": UniformFloatContextFeature("length", lower=0.05, upper=5.0, default_value=0.5),
    "mass": UniformFloatContextFeature("mass", lower=1e-3, upper=10.0, default_value=1.0),
    "n_legs": UniformIntegerContextFeature("n_legs", lower=1, upper=8, default_value=4),
    "direction": CategoricalContextFeature("direction", choices=[1, 3, 2, 4, 12, 32], default_value=1),
    "noise": UniformFloatContextFeature("noise", lower=-np.inf, upper=np.inf, default_value=0.0),
})
DISTS = [
    UniformFloatContextFeature("gravity", 5, 15),
    NormalFloatContextFeature("length", mu=0.5, sigma=0.4, lower=0.05, upper=5.0),
    UniformFloatContextFeature("mass", 0.01, 10.0, log=True),
    UniformIntegerContextFeature("n_legs", 2, 6),
    CategoricalContextFeature("direction", choices=[1, 3, 2, 4, 12, 32]),
]

# ---- spec constructors
INF = float("inf")
F32 = np.float32
NORMAL_TRIES = 32
BRANCHES = ("linear", "log", "int", "categorical", "constant", "normal0", "normal8", "exhausted")
CANARY = np.array([0xCAFEF00D], np.uint32).view(np.float32)[0]  # an ordinary negative float32, no NaN: compared as bits
GARBAGE = 0x5A5A5A5A                                            # what n_bad_out holds before a verification


def up(x, k=1):
    """x moved k float32 ulps towards +inf"""
    x = F32(x)
    for _ in range(k):
        x = np.nextafter(x, F32(INF))
    return float(x)


def _spec(kind, lower=0.0, upper=0.0, **kw):
    sp = _lib.FeatureSpec()
    sp.kind, sp.lower, sp.upper = kind, lower, upper
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def U(lower, upper, log=False):
    return _spec(_lib.FEAT_UNIFORM_FLOAT, lower, upper, log_scale=int(log))


def I(lower, upper):  # noqa: E743
    return _spec(_lib.FEAT_UNIFORM_INT, lower, upper)


def NRM(mu, sigma, lower=-INF, upper=INF):
    return _spec(_lib.FEAT_NORMAL_FLOAT, lower, upper, mu=mu, sigma=sigma)


def CONST(value, lower=-INF, upper=INF):
    return _spec(_lib.FEAT_CONSTANT, lower, upper, value=value)


def CAT(choices, kind=_lib.FEAT_CATEGORICAL):
    """kind = FEAT_CONSTANT: a categorical of the context space that is not sampled (device_sampler.feature_spec):
    its default, verified against [min, max] of the choices"""
    sp = _spec(kind, float(min(choices)), float(max(choices)), n_choices=len(choices), value=float(choices[0]))
    for k, c in enumerate(choices):
        sp.choices[k] = c
    return sp


def branch_of(sp):
    return {_lib.FEAT_CONSTANT: "constant", _lib.FEAT_UNIFORM_INT: "int", _lib.FEAT_CATEGORICAL: "categorical",
            _lib.FEAT_NORMAL_FLOAT: "normal"}.get(sp.kind) or ("log" if sp.log_scale else "linear")


def is_exact(sp):
    """the oracle evaluates this spec with the kernel's own float32 expression"""
    if sp.kind == _lib.FEAT_NORMAL_FLOAT:
        # sigma = 0: fma(0, z, mu) = mu; a window 10 sigma out: |z| <= sqrt(-2 log 2^-24) = 5.77, every attempt fails
        return sp.sigma == 0.0 or sp.lower >= sp.mu + 6.0 * sp.sigma
    return not (sp.kind == _lib.FEAT_UNIFORM_FLOAT and sp.log_scale)


def round_up_16(n):
    return (n + 15) // 16 * 16


# ---- float32 emulations of the kernel's inexact expressions (NumPy's libm in place of the device's)
def log_uniform_f32(sp, u):
    lo, hi = np.log(F32(sp.lower)), np.log(F32(sp.upper))
    v = np.exp(O.fmaf(F32(hi - lo), u.astype(F32), lo)).astype(F32)
    return np.minimum(np.maximum(v, F32(sp.lower)), F32(sp.upper))


def log_uniform_f64(sp, u):
    lo, hi = np.log(np.float64(sp.lower)), np.log(np.float64(sp.upper))
    return np.exp(lo + (hi - lo) * u.astype(np.float64))


def z_f32(u1, u2):
    u1, u2 = u1.astype(F32), u2.astype(F32)
    return (np.sqrt(F32(-2.0) * np.log(F32(1.0) - u1)) * np.cos(F32(6.28318530717958647692) * u2)).astype(F32)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


class Case:
    def __init__(self, name, specs, n, *, stride=None, offset=0, seed=99, reaches=()):
        self.name, self.spec_list, self.n = name, list(specs), n
        self.stride = n if stride is None else stride
        self.offset, self.seed = offset, seed
        self.reaches = set(reaches) or {b for b in map(branch_of, specs) if b != "normal"}
        assert self.stride >= n and self.reaches <= set(BRANCHES)

    F = property(lambda self: len(self.spec_list))

    def __repr__(self):
        return self.name

    def specs(self):
        arr = (_lib.FeatureSpec * self.F)()
        for j, sp in enumerate(self.spec_list):
            arr[j] = sp
        return arr

    def rows(self, branch):
        return [j for j, sp in enumerate(self.spec_list) if branch_of(sp) == branch]

    def canary_table(self):
        return np.full((self.F, self.stride), CANARY, np.float32)

    def u(self, row):
        """the first draw of every context of a row (what every kind but NORMAL_FLOAT samples from)"""
        return u_first(self.seed, self.offset, self.n, row)

    def trace(self, row):
        return _trace(self, row)

    # ---- bars
    def log_bar(self):
        return max(3e-6, 4 * D_LOG[self.name])

    def normal_bar(self, row, want):
        sp = self.spec_list[row]
        return (sp.sigma * max(4.5e-6, 4 * D_Z.get(self.name, 0.0))
                + 2 * ulp32(np.maximum(abs(sp.mu), np.abs(want.astype(np.float64)))))

    def flip_cap(self):
        return len(self.rows("normal")) * self.n // 1000

    def normal_alternative(self, row, want):
        """[n] float64: the oracle's result had the accept / reject decision gone the other way at the first attempt
        whose candidate lies within the bar of a bound; NaN where no drawn attempt does."""
        sp, t = self.spec_list[row], self.trace(row)
        bar = np.broadcast_to(self.normal_bar(row, want), (self.n,))
        alt = np.full(self.n, np.nan)
        cand32 = t.candidate.astype(np.float32)
        inside = (cand32 >= F32(sp.lower)) & (cand32 <= F32(sp.upper))
        near = np.minimum(np.abs(t.candidate - sp.lower), np.abs(t.candidate - sp.upper)) <= bar[:, None]
        near &= np.arange(NORMAL_TRIES)[None, :] <= np.minimum(t.accepted, NORMAL_TRIES - 1)[:, None]
        for c in np.nonzero(near.any(axis=1))[0]:
            a = int(np.argmax(near[c]))
            if a < t.accepted[c]:      # the oracle rejected it: the device may take it
                alt[c] = cand32[c, a]
            else:                      # the oracle took it: the device may draw on
                later = np.nonzero(inside[c, a + 1:])[0]
                alt[c] = cand32[c, a + 1 + later[0]] if later.size else np.clip(cand32[c, -1], F32(sp.lower), F32(sp.upper))
        return alt


@functools.lru_cache(maxsize=None)
def u_first(seed, offset, n, row):
    out = np.array([O.u01(O.lane_words(seed, offset + c, row, 0x40000000)[0]) for c in range(n)], np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _trace(case, row):
    return O.normal_trace(case.spec_list[row], case.seed, case.offset, case.n, row)


@functools.lru_cache(maxsize=None)
def oracle_table(case):
    """[F][stride] float32 of the oracle, the padding columns holding CANARY; computed once, read-only"""
    t = O.sample_contexts(case.specs(), case.n, case.seed, case.offset, ctx_stride=case.stride, out=case.canary_table())
    t.setflags(write=False)
    return t


def measure_d_log(case):
    worst = 0.0
    for j in case.rows("log"):
        sp, u = case.spec_list[j], case.u(j)
        want = log_uniform_f64(sp, u)
        worst = max(worst, float(np.max(np.abs(log_uniform_f32(sp, u).astype(np.float64) - want) / want)))
    return worst


def measure_d_z(case):
    worst = 0.0
    for j in case.rows("normal"):
        if case.spec_list[j].sigma == 0.0:
            continue
        t = case.trace(j)
        drawn = np.arange(NORMAL_TRIES)[None, :] <= np.minimum(t.accepted, NORMAL_TRIES - 1)[:, None]
        worst = max(worst, float(np.max(np.abs(z_f32(t.u1, t.u2).astype(np.float64) - t.z)[drawn])))
    return worst


def near_bound_entries(case):
    """entries of the oracle's own trace whose decision could go either way on the device"""
    return sum(int(np.isfinite(case.normal_alternative(j, oracle_table(case)[j, :case.n])).sum())
               for j in case.rows("normal") if not is_exact(case.spec_list[j]))


# ---- planted tables for the verifier
PLANT_COLUMNS = (0, 63, 64, 255, 256)   # and n - 1: wave and workgroup edges


def plant_values(sp):
    """NaN, +-inf (bad against finite bounds, valid against infinite ones), -0.0 (valid against a 0.0 bound), and one
    ulp off a choice / the upper bound"""
    near = up(sp.choices[0]) if sp.n_choices > 0 else up(sp.upper) if np.isfinite(sp.upper) else 1.0
    return [float("nan"), INF, -INF, -0.0, near]


def planted_table(case):
    """A copy of the oracle's table with entries planted at the wave / workgroup edge columns (feature rows in turn),
    every value of `plant_values` in every feature row (columns 10..14: whole contexts planted), one more entry per
    feature row, and every padding column overwritten with NaN -- those must not count."""
    t = oracle_table(case).copy()
    n, F = case.n, case.F
    vals = [plant_values(sp) for sp in case.spec_list]
    for i, col in enumerate(sorted({c for c in PLANT_COLUMNS + (n - 1,) if 0 <= c < n})):
        f = (3 * i + 1) % F
        t[f, col] = vals[f][i % 5]
    for k in range(5):
        if 10 + k < n:
            for f in range(F):
                t[f, 10 + k] = vals[f][k]
    for f in range(F):
        t[f, (7 * f + 3) % n] = vals[f][f % 5]
    t[:, n:] = np.nan
    return t


# ---- the table
S32, S64 = 2**32 + 1, 2**64 - 1          # the Philox key's high half: 1, all ones
OFF_CARRY, OFF_HIGH = 2**32 - 5, 2**62   # the context id carries into the high counter word 5 contexts in / lives there
N_EDGE = 1003                            # three workgroups and a partial one whose last wave is partial too

MIXED7 = [U(5, 15), NRM(0.5, 0.4, 0.05, 5.0), U(0.01, 10.0, log=True), I(2, 6), CAT([1, 3, 2, 4, 12, 32]),
          CONST(0.0), NRM(0.0, 1.0)]     # 7 x 42 LDS words: no multiple of the 256 threads that stage them
POOL = MIXED7 + [U(-1, 2), NRM(0.0, 1.0, 1.0, 1.5), I(-7, 3), CAT([3, -1, 2.5, -8, 0]), CONST(-INF), U(0.5, 1.0, log=True),
                 NRM(0.0, 1.0, 10.0, 11.0), NRM(2.0, 0.0, 1.0, 3.0)]

CASES = []


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


# shapes x strides x random-stream keys on the seven mixed features
for _i, _n in enumerate((1, 63, 64, 65, 255, 256, 257, 1003)):
    _stride = (_n, round_up_16(_n), _n + 5)[_i % 3]
    _add(f"shape-n{_n}-s{_stride}", MIXED7, _n, stride=_stride, offset=(0, OFF_HIGH, OFF_CARRY)[_i % 3],
         seed=(99, S32, S64)[(_i + _i // 3) % 3])
_add("f1", [U(5, 15)], 257, stride=272, seed=S32)
_add("f256", [POOL[k % len(POOL)] for k in range(256)], 257, stride=272, offset=OFF_CARRY, seed=S64)

# per kind
_add("linear", [U(3, 3), U(-5, -2), U(-1, 2), U(1, up(1)), U(5, 15)], N_EDGE, stride=N_EDGE + 5)
# exp(log x) in float32 (NumPy's libm) rounds below x for 0.001 and 0.1, to x for 0.5, above x for 2.5 and 10
_add("log", [U(x, x, log=True) for x in (0.001, 0.1, 0.5, 2.5, 10.0)]
     + [U(0.3, 0.3 * (1 + 1e-4), log=True), U(2.5, 2.5 * (1 + 1e-4), log=True), U(0.5, 1.0, log=True)],
     N_EDGE, stride=N_EDGE + 5, seed=S32)
_add("log-wide", [U(1e-30, 1e30, log=True)], N_EDGE, stride=round_up_16(N_EDGE), seed=S64)
_add("int", [I(5, 5), I(-7, 3), I(0, 1), I(0, 2**25)], N_EDGE, stride=N_EDGE + 5, offset=OFF_CARRY)
_add("categorical", [CAT([7]), CAT([0.5 * k - 3 for k in range(32)]), CAT([3, -1, 2.5, -8, 0]),
                     CAT([1.0, up(1.0), up(1.0, 2)])], N_EDGE, stride=N_EDGE + 5, seed=S32)
_add("normal-edges", [NRM(0.0, 1.0), NRM(2.0, 0.0, 1.0, 3.0), NRM(5.0, 0.0, 1.0, 3.0), NRM(-5.0, 0.0, 1.0, 3.0),
                      NRM(1e6, 1.0)], N_EDGE, stride=N_EDGE + 5, seed=S64, reaches={"normal0", "exhausted"})
# acceptance 0.092 per attempt: 4.6 % of the entries exhaust the 32, the rest spread over every attempt index
_add("normal-window", [NRM(0.5, 0.4, 0.9, 1.1), NRM(0.0, 1.0, 1.0, 1.5)], N_EDGE, stride=N_EDGE + 5, offset=OFF_HIGH,
     reaches={"normal0", "normal8", "exhausted"})
_add("normal-exhausted", [NRM(0.0, 1.0, 10.0, 11.0), NRM(3.0, 0.5, 8.0, 8.5)], N_EDGE, stride=N_EDGE + 5, seed=S32,
     reaches={"exhausted"})
_add("constant", [CONST(0.0), CONST(-0.0, 0.0, 0.0), CONST(1e-40, 1e-40, 1e-40), CONST(INF), CONST(-INF),
                  CAT([1, 3, 2], kind=_lib.FEAT_CONSTANT)], N_EDGE, stride=N_EDGE + 5)
# what the verifier must and must not count: +-inf against infinite bounds, -0.0 against a 0.0 bound, one ulp off a choice
_add("verify-edges", [NRM(0.0, 1.0), U(0.0, 1.0), CAT([1, 2, 3]), CAT([1, 3, 2], kind=_lib.FEAT_CONSTANT), I(0, 1)],
     257, stride=262, seed=S32, reaches={"normal0", "linear", "categorical", "constant", "int"})

# extreme draws: feature row 0 under seed 99 draws u = 0 at EXTREME_U0 and u = 1 - 2^-24 at EXTREME_UTOP
EXTREME_U0, EXTREME_UTOP = 9534654, 2158653
N_EXTREME, EXTREME_AT = 257, 128
EXTREME_SPECS = {
    "linear": U(5, 15), "log": U(0.01, 10.0, log=True), "log-narrow": U(2.5, 2.5 * (1 + 1e-4), log=True),
    "log-wide": U(1e-30, 1e30, log=True), "log-to-one": U(0.5, 1.0, log=True), "int": I(2, 6), "int-wide": I(0, 2**25),
    "categorical": CAT([1, 3, 2, 4, 12, 32]), "categorical-32": CAT([0.5 * k - 3 for k in range(32)]),
    "normal": NRM(0.0, 1.0), "normal-bounded": NRM(0.5, 0.4, 0.05, 5.0),
}
for _k, _sp in EXTREME_SPECS.items():
    _r = {"normal0"} if branch_of(_sp) == "normal" else ()
    # the extreme id is context EXTREME_AT of N_EXTREME: small, yet enough draws around it that the case's measured
    # D_log / D_z is the expression's deviation and not the luck of three draws (a [1e-30, 1e30] range moves by
    # 7.6e-6 per ulp of its logarithms: three draws measured 1.4e-6 where a thousand measure 3.8e-6)
    _add(f"u0-{_k}", [_sp], N_EXTREME, stride=N_EXTREME + 5, offset=EXTREME_U0 - EXTREME_AT, reaches=_r)
    _add(f"utop-{_k}", [_sp], N_EXTREME, stride=N_EXTREME + 5, offset=EXTREME_UTOP - EXTREME_AT, reaches=_r)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Measured by tests/test_context_kernel_table.py (test_recorded_deviations_are_the_measured_ones prints them) and held
# there: worst relative deviation of the float32 log-uniform / worst |z32 - z64|, per case with such a feature.
D_LOG = {
    "shape-n1-s1": 4.836e-08,
    "shape-n63-s64": 2.648e-07,
    "shape-n64-s69": 3.157e-07,
    "shape-n65-s65": 1.382e-07,
    "shape-n255-s256": 2.714e-07,
    "shape-n256-s261": 2.710e-07,
    "shape-n257-s257": 2.402e-07,
    "shape-n1003-s1008": 3.301e-07,
    "f256": 3.557e-07,
    "log": 1.792e-07,
    "log-wide": 3.793e-06,
    "u0-log": 2.783e-07,
    "utop-log": 3.098e-07,
    "u0-log-narrow": 1.366e-07,
    "utop-log-narrow": 1.282e-07,
    "u0-log-wide": 3.687e-06,
    "utop-log-wide": 3.773e-06,
    "u0-log-to-one": 1.455e-07,
    "utop-log-to-one": 1.335e-07,
}
D_Z = {
    "shape-n1-s1": 1.283e-07,
    "shape-n63-s64": 5.055e-07,
    "shape-n64-s69": 5.333e-07,
    "shape-n65-s65": 5.738e-07,
    "shape-n255-s256": 9.379e-07,
    "shape-n256-s261": 7.651e-07,
    "shape-n257-s257": 6.507e-07,
    "shape-n1003-s1008": 1.199e-06,
    "f256": 1.390e-06,
    "normal-edges": 8.325e-07,
    "normal-window": 1.526e-06,
    "normal-exhausted": 1.539e-06,
    "verify-edges": 5.551e-07,
    "u0-normal": 6.951e-07,
    "utop-normal": 7.094e-07,
    "u0-normal-bounded": 6.951e-07,
    "utop-normal-bounded": 7.094e-07,
}
