"""One case per device math primitive of fast_math.hip.h, classic_control.hip.h (SinCosTab) and brax_kernels.hip.h:
its inputs, its exact reference, a plain NumPy restatement of its formula and the error measure.  No GPU here.

A case is evaluated twice.  tests/test_math_primitive_table.py (host) measures E_host, the worst error of the RESTATEMENT
against the reference over exactly the case's inputs, and holds `E_HOST[case]` below to that measurement.
tests/test_gpu_math_primitives.py runs the primitive itself (tests/probe/math_probe.hip) on the same inputs; its bar is

    |device - reference| <= 2 E_host scale + ulp(reference, in the result type),   scale = 1 (abs) or |reference| (rel)

-- the factor covers the restatement's double rounding and the spread of the hardware seeds, the ulp the final rounding.
Nothing in the bar comes from the device.

Reference: NumPy `longdouble` libm (64-bit mantissa) over the exact float32 / float64 inputs; `mp_reference` is the same
function in mpmath, for the special points and for checking the longdouble reference itself on a sample.

Restatement rules.  float32 fma: exact double product plus addend, rounded to float32 (the sum is rounded twice: that is
what the factor 2 is for).  float64 fma: error-free product (Dekker), summed in longdouble, rounded to double.  A hardware
approximation instruction is its exact value, rounded to the instruction's type and moved by its documented accuracy in
either direction -- the restatement runs once per sign combination and the worse error counts:
v_rcp_f32 / v_rsq_f32 1 ulp of float32, v_rcp_f64 2^-24 relative (2^29 ulp: the ISA manual's figure, the same as
fast_math.hip.h's).  A library call (the ballot-guarded fallbacks) is the correctly rounded value moved by 1 ulp, inside the function's range.
"""
import functools
import itertools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "carl_amd", "csrc")
f32, f64, L = np.float32, np.float64, np.longdouble
PI = L("3.14159265358979323846264338327950288")
TAB_BLOCKS = (64, 256, 320)  # the product's workgroup sizes over the table: per-call kernels, and kRolloutThreads


# ------------------------------------------------------------------------------------------------ arithmetic helpers
def fma32(a, b, c):
    with np.errstate(all="ignore"):
        return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def fma64(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, f64), np.asarray(b, f64), np.asarray(c, f64))
    with np.errstate(all="ignore"):
        p = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        r = ((p.astype(L) + c.astype(L)) + e.astype(L)).astype(f64)
        return np.where(np.isfinite(r), r, p + c)  # (overflow / non-finite operands: the plain sum has the right class)


def ulp_of(ref, dtype):
    """one ulp of `dtype` at the magnitude of `ref`"""
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(ref, L)).astype(dtype)).astype(L)


def approx(exact, dtype, sign, rel=None):
    """a hardware approximation: `exact` rounded to dtype, then moved by one ulp (or by `rel` relative) towards `sign`"""
    with np.errstate(all="ignore"):
        v = np.asarray(exact, L).astype(dtype)
        step = np.spacing(np.abs(v)) if rel is None else np.abs(v) * dtype(rel)
        out = (v + sign * step).astype(dtype)
        return np.where(np.isfinite(v) & (v != 0), out, v)


def library(ref, dtype, limit=None):
    """a library call: correctly rounded, moved one ulp further from the exact value -- but never out of the function's
    range [-limit, limit] (sinf cannot return 1.0000001: there the ulp goes towards zero, the only side it has)"""
    with np.errstate(all="ignore"):
        v = np.asarray(ref, L).astype(dtype)
        s = np.where(v.astype(L) >= ref, 1, -1).astype(dtype)
        out = (v + s * np.spacing(np.abs(v))).astype(dtype)
        if limit is not None:
            over = np.abs(out) > dtype(limit)
            out = np.where(over, np.nextafter(v, dtype(0)), out).astype(dtype)
        return np.where(np.isfinite(v), out, v)


def neighbours(v, dtype):
    v = np.asarray(v, dtype).ravel()
    return np.concatenate([np.nextafter(v, dtype(-np.inf)), v, np.nextafter(v, dtype(np.inf))])


def logspace(lo, hi, n, dtype, rng=None, both_signs=True):
    v = np.exp(np.linspace(np.log(lo), np.log(hi), n)).astype(dtype)
    return np.concatenate([v, -v]) if both_signs else v


def _sin(x):
    with np.errstate(invalid="ignore"):
        return np.sin(np.asarray(x, L))


def _cos(x):
    with np.errstate(invalid="ignore"):
        return np.cos(np.asarray(x, L))


# ------------------------------------------------------------------------------------------------ restatements
S32 = (2.7557314297e-06, -1.9841270114e-04, 8.3333337680e-03, -1.6666667163e-01)
C32 = (-2.7557314297e-07, 2.4801587642e-05, -1.3888889225e-03, 4.1666667908e-02)
TWO_OVER_PI32 = float.fromhex("0x1.45f306p-1")
HI32, MID32, LO32 = float.fromhex("0x1.921fb6p+0"), float.fromhex("-0x1.777a5cp-25"), float.fromhex("-0x1.ee59dap-50")


def _poly32(r):
    z = (r * r).astype(f32)
    ps = fma32(z, f32(S32[0]), f32(S32[1]))
    ps = fma32(z, ps, f32(S32[2]))
    ps = fma32(z, ps, f32(S32[3]))
    S = fma32((r * z).astype(f32), ps, r)
    pc = fma32(z, f32(C32[0]), f32(C32[1]))
    pc = fma32(z, pc, f32(C32[2]))
    pc = fma32(z, pc, f32(C32[3]))
    C = fma32((z * z).astype(f32), pc, fma32(z, f32(-0.5), f32(1.0)))
    return S, C


def _quadrant(q, S, C):
    odd = (q & 1) != 0
    s2, c2 = np.where(odd, C, S), np.where(odd, S, C)
    return np.where((q & 2) != 0, -s2, s2), np.where(((q + 1) & 2) != 0, -c2, c2)


def _fallback32(x, sn, cs, big):
    return (np.where(big, library(_sin(x), f32, 1), sn).astype(f32), np.where(big, library(_cos(x), f32, 1), cs).astype(f32))


def re_sincos_fast_f32(x):
    with np.errstate(all="ignore"):
        big = ~(np.abs(x) <= f32(1.0e5))
        xs = np.where(big, f32(0), x)
        k = np.rint((xs * f32(TWO_OVER_PI32)).astype(f32))
        r = fma32(k, f32(-HI32), xs)
        r = fma32(k, f32(-MID32), r)
        r = fma32(k, f32(-LO32), r)
        S, C = _poly32(r)
        sn, cs = _quadrant(k.astype(np.int64), S, C)
        return _fallback32(x, sn, cs, big)


def re_sincos_fast_pk(x):
    with np.errstate(all="ignore"):
        big = ~(np.abs(x) <= f32(1.0e5))
        xs = np.where(big, f32(0), x)
        magic = f32(1.5 * 2 ** 23)
        t = fma32(xs, f32(TWO_OVER_PI32), magic)
        k = (t - magic).astype(f32)
        r = fma32(k, f32(-HI32), xs)
        r = fma32(k, f32(-MID32), r)
        r = fma32(k, f32(-LO32), r)
        S, C = _poly32(r)
        q = t.view(np.uint32).astype(np.int64)  # the low mantissa bits of t are k (two's complement)
        sn, cs = _quadrant(q, S, C)
        return _fallback32(x, sn, cs, big)


def re_cos_fast(x):
    return (re_sincos_fast_f32(x)[1],)


def re_cos_twice_fast(h):
    with np.errstate(all="ignore"):
        c = [f32(float.fromhex(v)) for v in ("-0x1.1173p-22", "0x1.9ec0c8p-16", "-0x1.6c0d24p-10", "0x1.555518p-5", "-0x1.fffffep-2")]
        z = (h * h).astype(f32)
        p = fma32(z, c[0], c[1])
        for ck in c[2:]:
            p = fma32(z, p, ck)
        cs = fma32(z, p, f32(1.0))
        r = fma32((cs + cs).astype(f32), cs, f32(-1.0))
        wide = ~(np.abs(h) <= f32(1.85))
        return (np.where(wide, re_sincos_fast_f32((h + h).astype(f32))[1], r).astype(f32),)


S64 = (1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04,
       8.33333333332248946124e-03, -1.66666666666666324348e-01)
C64 = (-1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05,
       -1.38888888888741095749e-03, 4.16666666666666019037e-02)
HI64, MID64, LO64 = (float.fromhex("0x1.921fb54442d18p+0"), float.fromhex("0x1.1a62633145c07p-54"),
                     float.fromhex("-0x1.f1976b7ed8fbcp-110"))


def _sincos64_fast(x):
    with np.errstate(all="ignore"):
        k = np.rint(x * float.fromhex("0x1.45f306dc9c883p-1"))
        r = fma64(k, -HI64, x)
        r = fma64(k, -MID64, r)
        r = fma64(k, -LO64, r)
        z = r * r
        ps = fma64(z, S64[0], S64[1])
        for ck in S64[2:]:
            ps = fma64(z, ps, ck)
        S = fma64(r * z, ps, r)
        pc = fma64(z, C64[0], C64[1])
        for ck in C64[2:]:
            pc = fma64(z, pc, ck)
        C = fma64(z * z, pc, fma64(z, -0.5, 1.0))
        return _quadrant(k.astype(np.int64), S, C)


def re_sincos_fast_f64_nofallback(x):
    return _sincos64_fast(x)


def re_sincos_fast_f64(x):
    big = ~(np.abs(x) <= 1.0e6)
    sn, cs = _sincos64_fast(np.where(big, 0.0, x))
    return np.where(big, library(_sin(x), f64, 1), sn), np.where(big, library(_cos(x), f64, 1), cs)


def re_sincos2_fast(xa, xb):
    return (*_sincos64_fast(xa), *_sincos64_fast(xb))


@functools.lru_cache(None)
def sincos_table():
    src = open(os.path.join(CSRC, "sincos_table.inc")).read()
    consts = {m.group(1): float.fromhex(m.group(2)) for m in re.finditer(r"#define (CARL_SINCOS_TAB_\w+) (-?0x[0-9a-f.]+p[+-]\d+)", src)}
    vals = [float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", src.split("CARL_SINCOS_TAB_VALUES")[1])]
    return consts, np.array(vals).reshape(-1, 2)


def _two_product(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def tab_lookup(x):
    """SinCosTab::lookup2 for one angle: (table index, reduced argument), EXACTLY as two fmas round (the device's bits
    are compared with these; |x / step| < 2^51)"""
    consts, tab = sincos_table()
    x = np.asarray(x, f64)
    # t = fma(x, inv, 1.5 * 2^52): the exact product p + e rounded to the nearest integer, ties to even
    p, e = _two_product(x, np.full_like(x, consts["CARL_SINCOS_TAB_INV_STEP"]))
    k = np.rint(p)
    d0 = p - k  # exact; |d0| <= 1/2, and off the tie the error term e cannot carry p + e across it
    k = k + np.where((d0 == 0.5) & (e > 0), 1.0, 0.0) - np.where((d0 == -0.5) & (e < 0), 1.0, 0.0)
    i = k.astype(np.int64) & (tab.shape[0] - 1)  # the low dword of the two's-complement sum, masked
    # r = fma(k, -hi, x): k hi = q + f exactly, x - q is exact (Sterbenz: q within a factor 2 of x, or k = 0), one rounding
    q, f = _two_product(k, np.full_like(x, consts["CARL_SINCOS_TAB_STEP_HI"]))
    return i, (x - q) - f


def _tab_sincos(x):
    _, tab = sincos_table()
    i, r = tab_lookup(x)
    z = r * r
    sr = fma64(r * z, -1.0 / 6.0, r)
    cr = fma64(z, fma64(z, 1.0 / 24.0, -0.5), 1.0)
    S, C = tab[i, 0], tab[i, 1]
    return fma64(S, cr, C * sr), fma64(C, cr, -(S * sr))


def re_tab_sincos2(xa, xb):
    return (*_tab_sincos(xa), *_tab_sincos(xb))


def _variants(n_seeds, fn):
    """run `fn(signs)` for every combination of seed signs; a list of output tuples"""
    return [fn(s) for s in itertools.product((-1, 1), repeat=n_seeds)]


def _rcp64_seed(d, sign):
    with np.errstate(all="ignore"):
        return approx(L(1) / np.asarray(d, L), f64, sign, rel=2.0 ** -24)


def re_rcp_fast(d):
    def one(s):
        r = _rcp64_seed(d, s[0])
        e = fma64(-d, r, 1.0)
        r = fma64(r, e, r)
        e = fma64(-d, r, 1.0)
        return (fma64(r, e, r),)
    return _variants(1, one)


def _rcp_fast1(d, sign):
    r = _rcp64_seed(d, sign)
    return fma64(r, fma64(-d, r, 1.0), r)


def re_rcp_fast1(d):
    return _variants(1, lambda s: (_rcp_fast1(d, s[0]),))


def _rcp32(x, sign):
    with np.errstate(all="ignore"):
        return approx(L(1) / np.asarray(x, L), f32, sign)


def _atan2_fast(y, x, s):
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
        t = (mn * _rcp32(mx, s[0])).astype(f32)
        t = np.where(mx > 0, t, f32(0))
        mid = t > f32(0.41421356237)
        tr = np.where(mid, ((t - f32(1)).astype(f32) * _rcp32((t + f32(1)).astype(f32), s[1])).astype(f32), t)
        z = (tr * tr).astype(f32)
        p = fma32(z, f32(8.05374449538e-2), f32(-1.38776856032e-1))
        p = fma32(z, p, f32(1.99777106478e-1))
        p = fma32(z, p, f32(-3.33329491539e-1))
        r = (fma32((p * z).astype(f32), tr, tr) + np.where(mid, f32(0.78539816339), f32(0))).astype(f32)
        r = np.where(ay > ax, (f32(1.57079632679) - r).astype(f32), r)
        r = np.where(np.signbit(x), (f32(3.14159265359) - r).astype(f32), r)
        return np.copysign(r, y).astype(f32)


def re_atan2_fast(y, x):
    return _variants(2, lambda s: (_atan2_fast(y, x, s),))


def re_div_fast(a, b):
    return _variants(1, lambda s: ((a * _rcp32(b, s[0])).astype(f32),))


def re_asin_r_f32(x):
    def one(s):
        with np.errstate(all="ignore"):
            c2 = np.maximum(((f32(1) - x).astype(f32) * (f32(1) + x).astype(f32)).astype(f32), f32(0))
            rs = approx(L(1) / np.sqrt(np.maximum(c2, f32(1e-30)).astype(L)), f32, s[0])
            return (_atan2_fast(x, (c2 * rs).astype(f32), s[1:]),)
    return _variants(3, one)


A64 = (-3.76549087472088720e-02, 6.97418621847181036e-02, -8.99255026739464586e-02, 1.11034566044549116e-01,
       -1.42853865353561232e-01, 1.99999930530023323e-01, -3.33333332769153445e-01, 9.99999999999244826e-01)


def _atan2_f64(y, x, sign, xpos):
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
        mid = mn > 0.41421356237309503 * mx
        num, den = np.where(mid, mn - mx, mn), np.where(mid, mn + mx, mx)
        t = num * _rcp_fast1(den, sign)
        t = np.where(mx > 0, t, 0.0)
        z = t * t
        p = fma64(z, A64[0], A64[1])
        for ck in A64[2:]:
            p = fma64(z, p, ck)
        r = fma64(t, p, np.where(mid, 0.78539816339744831, 0.0))
        r = np.where(ay > ax, 1.5707963267948966 - r, r)
        if not xpos:
            r = np.where(np.signbit(x), 3.1415926535897932 - r, r)
        return np.copysign(r, y)


def re_atan2_f64(y, x):
    return _variants(1, lambda s: (_atan2_f64(y, x, s[0], False),))


def re_atan2_f64_xpos(y, x):
    return _variants(1, lambda s: (_atan2_f64(y, x, s[0], True),))


def _sqrt01(x, sign):
    with np.errstate(all="ignore"):
        xf = x.astype(f32)
        y = approx(L(1) / np.sqrt(xf.astype(L)), f32, sign).astype(f64)
        g, h = x * y, 0.5 * y
        r = fma64(-g, h, 0.5)
        g = fma64(g, r, g)
        h = fma64(h, r, h)
        g = fma64(fma64(-g, g, x), h, g)
        return np.where(x > 1e-30, g, 0.0)


def re_sqrt01_f64(x):
    return _variants(1, lambda s: (_sqrt01(x, s[0]),))


def re_asin_f64(x):
    return _variants(2, lambda s: (_atan2_f64(x, _sqrt01((1.0 - x) * (1.0 + x), s[0]), s[1], True),))


def re_qaxis(k, angle):
    s, c = re_sincos_fast_f32((f32(0.5) * angle).astype(f32))
    z = np.zeros_like(s)
    return (np.stack([c, np.where(k == 0, s, z), np.where(k == 1, s, z), np.where(k == 2, s, z)], 1),)


# ------------------------------------------------------------------------------------------------ references
def ref_sincos(x):
    return _sin(x), _cos(x)


def ref_sincos2(xa, xb):
    return _sin(xa), _cos(xa), _sin(xb), _cos(xb)


def ref_rcp(d):
    with np.errstate(all="ignore"):
        return (L(1) / d.astype(L),)


def ref_atan2(y, x):
    return (np.arctan2(y.astype(L), x.astype(L)),)


def ref_div(a, b):
    return (a.astype(L) / b.astype(L),)


def ref_sqrt01(x):
    """the documented function: sqrt(x) above the 1e-30 cut, exactly 0 at and below it"""
    return (np.where(x > 1e-30, np.sqrt(x.astype(L)), L(0)),)


def ref_asin(x):
    return (np.arcsin(x.astype(L)),)


def ref_qaxis(k, angle):
    h = angle.astype(L) * L(0.5)
    s, c = _sin(h), _cos(h)
    z = np.zeros_like(s)
    return (np.stack([c, np.where(k == 0, s, z), np.where(k == 1, s, z), np.where(k == 2, s, z)], 1),)


MP_FUNCS = {"sincos": lambda mp, x: (mp.sin(x), mp.cos(x)),
            "sincos2": lambda mp, a, b: (mp.sin(a), mp.cos(a), mp.sin(b), mp.cos(b)),
            "cos": lambda mp, x: (mp.cos(x),), "cos2": lambda mp, h: (mp.cos(2 * h),),
            "rcp": lambda mp, d: (1 / d,), "atan2": lambda mp, y, x: (mp.atan2(y, x),),
            "div": lambda mp, a, b: (a / b,), "sqrt01": lambda mp, x: (mp.sqrt(x) if x > 1e-30 else mp.mpf(0),),
            "asin": lambda mp, x: (mp.asin(x),)}


def special_points(dtype):
    """|values| at which these functions change path or a float format changes regime: the guards of the three headers
    with their neighbours, 0, the subnormal / normal boundary, 1 and its neighbours, the extremes"""
    fi = np.finfo(dtype)
    guards = [0.78, 1.85, 3.7, 1.0e5, 1.0e6, 1.0, 0.5, 1e-30, np.tan(np.pi / 8), np.pi / 2, np.pi, np.pi / 256, np.pi / 512]
    pts = np.concatenate([neighbours(guards, dtype), np.array([0.0, fi.tiny, fi.smallest_subnormal, fi.max, 3e38 if dtype == f32 else 1e300,
                                                               1 - 2.0 ** -53, 1e-45, 5.9e-39, 1e-310], dtype=dtype)])
    return np.unique(np.abs(pts))


def special_indices(case, per_value=2):
    """indices of the case's inputs where some argument sits at a special point (a few per distinct value)"""
    ins = case.inputs()
    hit = np.zeros(ins[0].shape[0], bool)
    for a in ins:
        if a.dtype.kind == "f":
            hit |= np.isin(np.abs(a), special_points(a.dtype.type))
    idx = np.flatnonzero(hit)
    key = np.stack([np.abs(a[idx]).astype(np.float64) for a in ins], 1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    rank = np.zeros(idx.size, np.int64)
    seen = {}
    for j, g in enumerate(np.ravel(inv).tolist()):
        rank[j] = seen.get(g, 0)
        seen[g] = rank[j] + 1
    return idx[rank < per_value]


def mp_reference(case, idx):
    """the case's reference at inputs[idx] in 60-digit mpmath: a list of output tuples of mpf (non-finite inputs excluded
    by the caller)"""
    import mpmath as mp

    mp.mp.dps = 60
    ins = case.inputs()
    return [MP_FUNCS[case.mp](mp, *(mp.mpf(float(a[i])) for a in ins)) for i in idx]


# ------------------------------------------------------------------------------------------------ inputs
def _rng(name):
    import zlib

    return np.random.default_rng(zlib.crc32(name.encode()))


F32_SPECIAL = np.array([0.0, -0.0, 1.17549435e-38, -1.17549435e-38, 1e-45, -1e-45, 5.9e-39, -5.9e-39, 3e-39, 1e-30, -1e-30,
                        3e38, -3e38, 3.4028235e38, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, 16777216.0, 1e9, -1e9, 1e20],
                       dtype=f32)


def in_sincos_f32(name):
    """every float nearest j pi / 4 (even j: the quadrant boundaries k pi / 2; odd j: the reduction's ties, x 2 / pi a
    half-integer) and its neighbours, up to the 1e5 guard and a little past; the guards; the specials; sweeps"""
    rng = _rng(name)
    j = np.arange(-127400, 127401)
    quarter = neighbours((j.astype(L) * (PI / 4)).astype(f32), f32)
    guards = np.concatenate([neighbours([1e5, -1e5, 0.78, -0.78, 1.85, -1.85, 3.7, -3.7], f32), F32_SPECIAL])
    sweeps = np.concatenate([rng.uniform(-1e5, 1e5, 120000), rng.uniform(-10, 10, 60000), rng.uniform(-1, 1, 20000),
                             rng.uniform(-3e5, 3e5, 10000), np.round(rng.uniform(-4e5, 4e5, 4000))]).astype(f32)
    big = logspace(1e5, 3e38, 4000, f32)
    small = logspace(1e-45, 1.0, 8000, f32)
    return (np.concatenate([quarter, guards, sweeps, big, small]).astype(f32),)


def in_cos_twice(name):
    rng = _rng(name)
    grid = np.linspace(-1.85, 1.85, 400001).astype(f32)
    edges = np.concatenate([neighbours([1.85, -1.85, 0.0, 5e4, -5e4], f32), F32_SPECIAL,
                            np.array([np.nan, 1.8500001, 1.9, -1.9, 6e4, -6e4, 1e6], dtype=f32)])
    wide = np.concatenate([rng.uniform(-60, 60, 40000), rng.uniform(-7e4, 7e4, 40000), np.round(rng.uniform(-2e5, 2e5, 2000))]).astype(f32)
    h = np.concatenate([grid, edges, wide, logspace(1e-45, 1.85, 4000, f32)]).astype(f32)
    return (h[~(np.isfinite(h) & (np.abs(h) > 1.7e38))],)  # (2 h must be a float32: the function is cos of THAT number)


F64_SPECIAL = np.array([0.0, -0.0, 2.2250738585072014e-308, -2.2250738585072014e-308, 5e-324, -5e-324, 1e-310, 1.0, -1.0])


def in_sincos_f64(name, span=1.0e6, beyond=False):
    rng = _rng(name)
    j = np.arange(-40000, 40001)
    quarter = neighbours((j.astype(L) * (PI / 4)).astype(f64), f64)
    far = neighbours((rng.integers(-int(span * 4 / np.pi), int(span * 4 / np.pi), 40000).astype(L) * (PI / 4)).astype(f64), f64)
    parts = [quarter, far, neighbours([span, -span], f64), F64_SPECIAL, rng.uniform(-span, span, 60000),
             rng.uniform(-10, 10, 40000), logspace(1e-320, 1.0, 4000, f64), np.round(rng.uniform(-span, span, 2000))]
    x = np.concatenate(parts)
    x = x[np.abs(x) <= span]
    if beyond:
        x = np.concatenate([x, neighbours([span, -span], f64), logspace(span, 1e300, 6000, f64),
                            rng.uniform(-1e9, 1e9, 6000), np.array([np.inf, -np.inf, np.nan, 1.7976931348623157e308])])
    return (x.astype(f64),)


def in_sincos2(name):
    (x,) = in_sincos_f64(name)
    return x, _rng(name + "b").permutation(x)


def _tab_grid():
    i = np.arange(-1024, 1025)
    grid = neighbours((i.astype(L) * (PI / 256)).astype(f64), f64)
    half = neighbours(((i.astype(L) + L(0.5)) * (PI / 256)).astype(f64), f64)
    return grid, half


def in_tab(name):
    rng = _rng(name)
    grid, half = _tab_grid()
    xa = np.concatenate([grid, half, rng.uniform(-40, 40, 100000), rng.uniform(-40, 0, 20000), F64_SPECIAL[:9],
                         logspace(1e-300, 1.0, 2000, f64)])
    return xa.astype(f64), rng.permutation(xa).astype(f64)


def in_tab_wide(name):
    rng = _rng(name)
    xa = np.concatenate([rng.uniform(-1e4, 1e4, 4000), -rng.uniform(40, 1e4, 2000),
                         neighbours((rng.integers(-800000, 800000, 700).astype(L) * (PI / 256)).astype(f64), f64)])
    return xa.astype(f64), rng.permutation(xa).astype(f64)


def in_rcp(name):
    rng = _rng(name)
    p2 = 2.0 ** np.arange(-960, 961)
    near1 = np.concatenate([neighbours([1.0, 2.0, 0.5], f64), 1 + rng.uniform(-1e-3, 1e-3, 20000), rng.uniform(0.5, 2, 40000)])
    mant = (1 + rng.random(60000)) * 2.0 ** rng.integers(-60, 60, 60000)
    v = np.concatenate([logspace(1e-290, 1e290, 60000, f64, both_signs=False), p2, near1, mant])
    return (np.concatenate([v, -v]),)


RCP_DOCUMENTED_POINTS = np.array([0.0, -0.0, np.inf, -np.inf])  # evaluated and written down, not held to a bar


def _atan2_pairs(name, dtype, lo, hi, xpos):
    rng = _rng(name)
    n = 60000
    ang = rng.uniform(-np.pi, np.pi, n)
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    together = (mag * np.sin(ang), mag * np.cos(ang))                                  # the pair scaled together
    span = np.log(hi / lo)
    my = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    apart = (my * rng.choice([-1, 1], n), my * np.exp(rng.uniform(-span, span, n)).clip(lo / my, hi / my) * rng.choice([-1, 1], n))
    unit = (rng.uniform(-1, 1, n), rng.uniform(-1, 1, n))
    m = np.exp(rng.uniform(np.log(lo), np.log(hi), 4000)).astype(dtype).astype(f64)
    sg = rng.choice([-1.0, 1.0], (2, 4000))
    diag = (sg[0] * m, sg[1] * m)                                                      # |y| = |x|
    t8 = neighbours(np.tan(np.pi / 8) * np.ones(1), dtype).astype(f64)                 # t either side of tan(pi / 8)
    tt = np.concatenate([t8, np.tan(np.pi / 8) * (1 + rng.uniform(-1e-6, 1e-6, 4000))])
    mm = np.exp(rng.uniform(np.log(lo) / 2, np.log(hi) / 2, tt.size))
    q = rng.choice([-1.0, 1.0], (2, tt.size))
    swap = rng.random(tt.size) < 0.5
    octant = (np.where(swap, mm, mm * tt) * q[0], np.where(swap, mm * tt, mm) * q[1])
    z, one = np.array([0.0, -0.0]), np.array([1.0, -1.0, 3.0, -2.5e-20, 1e25])
    axes_y = np.concatenate([np.repeat(z, 2), np.repeat(z, one.size), np.tile(one, 2)])
    axes_x = np.concatenate([np.tile(z, 2), np.tile(one, 2), np.repeat(z, one.size)])
    y = np.concatenate([together[0], apart[0], unit[0], diag[0], octant[0], axes_y]).astype(dtype)
    x = np.concatenate([together[1], apart[1], unit[1], diag[1], octant[1], axes_x]).astype(dtype)
    if xpos:
        x = np.abs(x)  # (+0 included: the hinge's scalar part after the sign flip is >= 0)
    return y, x


def in_atan2_f32(name):
    return _atan2_pairs(name, f32, 1e-30, 1e30, False)


def in_atan2_f64(name):
    return _atan2_pairs(name, f64, 1e-30, 1e30, False)


def in_atan2_f64_xpos(name):
    return _atan2_pairs(name, f64, 1e-30, 1e30, True)


def in_sqrt01(name):
    rng = _rng(name)
    return (np.concatenate([np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-40, 1e-31, 1.0, 1 - 2.0 ** -53, 0.25, 0.5]),
                            neighbours([1e-30], f64), logspace(1e-30 * (1 + 1e-9), 1.0, 100000, f64, both_signs=False),
                            rng.uniform(0, 1, 100000), 1 - np.exp(rng.uniform(np.log(1e-16), 0, 20000)),
                            logspace(1e-320, 1e-30, 2000, f64, both_signs=False)]).clip(0, 1),)


def _asin_inputs(name, dtype):
    rng = _rng(name)
    one = dtype(1)
    edge = np.array([one, np.nextafter(one, dtype(0)), -one, -np.nextafter(one, dtype(0)), 0.0, -0.0, 0.5, -0.5], dtype=dtype)
    near = 1 - np.exp(rng.uniform(np.log(np.finfo(dtype).eps), 0, 20000))
    return (np.concatenate([edge, rng.uniform(-1, 1, 150000), np.linspace(-1, 1, 50001), near, -near,
                            logspace(1e-30, 1e-3, 4000, f64)]).astype(dtype).clip(-1, 1),)


def in_asin_f64(name):
    return _asin_inputs(name, f64)


def in_asin_f32(name):
    return _asin_inputs(name, f32)


def in_div(name):
    """both signs; numerator, divisor and quotient each inside 1e-30 .. 1e30 (all normal, the divisor's reciprocal too)"""
    rng = _rng(name)
    n = 200000
    lb = rng.uniform(np.log(1e-30), np.log(1e30), n)
    lq = rng.uniform(np.maximum(np.log(1e-30), np.log(1e-30) - lb), np.minimum(np.log(1e30), np.log(1e30) - lb))
    b = (np.exp(lb) * rng.choice([-1, 1], n)).astype(f32)
    a = (np.exp(lq) * b.astype(f64) * rng.choice([-1, 1], n)).astype(f32)
    near = (rng.uniform(0.5, 2, 50000).astype(f32), rng.uniform(0.5, 2, 50000).astype(f32))
    a, b = np.concatenate([a, near[0], 2.0 ** rng.integers(-90, 90, 2000)]).astype(f32), np.concatenate([b, near[1], 2.0 ** rng.integers(-9, 9, 2000)]).astype(f32)
    ok = (np.abs(a) >= 1e-30) & (np.abs(a) <= 1e30)
    return a[ok], b[ok]


def in_qaxis(name):
    rng = _rng(name)
    ang = np.concatenate([rng.uniform(-4 * np.pi, 4 * np.pi, 90000), neighbours((np.arange(-16, 17).astype(L) * (PI / 2)).astype(f32), f32),
                          np.array([0.0, -0.0, 1e-40, 12.566371, -12.566371])]).astype(f32)
    k = (np.arange(ang.size) % 3).astype(np.int32)
    return k, ang


# ------------------------------------------------------------------------------------------------ the table
class Case:
    """name: test id.  covers: the header functions this case evaluates, as `file:function(first argument type)`.
    entry: the probe's entry point.  kind: argument layout (tests/math_probe.py).  measure: abs | rel.
    signed_zero: a zero result carries the reference's sign (documented by the primitive)."""

    def __init__(self, name, covers, entry, kind, dtype, gen, ref, restate, measure, mp, *, blocks=(256,), signed_zero=False,
                 seed=None):
        self.name, self.covers, self.entry, self.kind, self.dtype = name, tuple(covers), entry, kind, dtype
        self._gen, self._ref, self._restate = gen, ref, restate
        self.measure, self.mp, self.blocks, self.signed_zero = measure, mp, tuple(blocks), signed_zero
        self.seed = seed or name  # cases that are compared bit for bit draw the same inputs

    @functools.lru_cache(None)
    def inputs(self):
        ins = tuple(np.ascontiguousarray(a) for a in self._gen(self.seed))
        assert all(a.shape[0] == ins[0].shape[0] for a in ins) and 0 < ins[0].shape[0] <= 2 ** 20, self.name
        for a in ins:
            a.setflags(write=False)
        return ins

    @functools.lru_cache(None)
    def reference(self):
        """longdouble outputs; NaN where the primitive has no value (non-finite trig arguments)"""
        out = tuple(np.asarray(r, L) for r in self._ref(*self.inputs()))
        for r in out:
            r.setflags(write=False)
        return out

    def restatements(self):
        """the NumPy restatement's outputs: a list (one per hardware-seed sign combination) of output tuples"""
        r = self._restate(*self.inputs())
        return r if isinstance(r, list) else [r]

    def error(self, got, ref):
        """the case's error measure, elementwise (0 where both are NaN; inf where only one is)"""
        with np.errstate(all="ignore"):
            got, ref = np.asarray(got).astype(L), np.asarray(ref, L)
            e = np.abs(got - ref)
            if self.measure == "rel":
                e = np.where(ref != 0, e / np.abs(ref), e)
            nan_g, nan_r = np.isnan(got), np.isnan(ref)
            e = np.where(nan_g & nan_r, 0, e)
            return np.where(nan_g != nan_r, np.inf, e)

    def bound(self, ref):
        """the device bar at each element (module docstring)"""
        ref = np.asarray(ref, L)
        with np.errstate(all="ignore"):
            scale = np.abs(ref) if self.measure == "rel" else L(1)
            b = 2 * L(E_HOST[self.name]) * scale + ulp_of(ref, self.dtype)
            return np.where(np.isnan(ref), L(0), b)

    def e_host(self):
        worst = 0.0
        for outs in self.restatements():
            for got, ref in zip(outs, self.reference()):
                worst = max(worst, float(self.error(got, ref).max()))
        return worst


FM, CC, BK = "fast_math.hip.h", "classic_control.hip.h", "brax_kernels.hip.h"
CASES = [
    Case("sincos_fast_f32", [f"{FM}:sincos_fast(float)"], "sincos_fast_f32", "sc", f32, in_sincos_f32, ref_sincos,
         re_sincos_fast_f32, "abs", "sincos", seed="sincos32"),
    Case("sincos_fast_pk", [f"{FM}:sincos_fast_pk(float)"], "sincos_fast_pk", "sc", f32, in_sincos_f32, ref_sincos,
         re_sincos_fast_pk, "abs", "sincos", seed="sincos32"),
    Case("sincos_fast_smallarg", [f"{FM}:sincos_fast_smallarg(float)"], "sincos_fast_smallarg", "sc", f32, in_sincos_f32,
         ref_sincos, re_sincos_fast_f32, "abs", "sincos", seed="sincos32"),  # (documented: the same bits as sincos_fast)
    Case("sincos_fast_f64", [f"{FM}:sincos_fast(double)"], "sincos_fast_f64", "sc", f64,
         lambda name: in_sincos_f64(name, beyond=True), ref_sincos, re_sincos_fast_f64, "abs", "sincos"),
    Case("sincos_fast_f64_nofallback", [f"{FM}:sincos_fast(double)"], "sincos_fast_f64_nofallback", "sc", f64, in_sincos_f64,
         ref_sincos, re_sincos_fast_f64_nofallback, "abs", "sincos", seed="sincos64"),
    Case("sincos2_fast", [f"{FM}:sincos2_fast(double)"], "sincos2_fast", "sc2", f64, in_sincos2, ref_sincos2, re_sincos2_fast,
         "abs", "sincos2", seed="sincos64"),
    Case("rcp_fast", [f"{FM}:rcp_fast(double)"], "rcp_fast", "unary", f64, in_rcp, ref_rcp, re_rcp_fast, "rel", "rcp", seed="rcp"),
    Case("rcp_fast1", [f"{FM}:rcp_fast1(double)"], "rcp_fast1", "unary", f64, in_rcp, ref_rcp, re_rcp_fast1, "rel", "rcp", seed="rcp"),
    Case("cos_fast", [f"{FM}:cos_fast(float)"], "cos_fast", "unary", f32, in_sincos_f32, lambda x: (_cos(x),), re_cos_fast,
         "abs", "cos", seed="sincos32"),
    Case("cos_twice_fast", [f"{FM}:cos_twice_fast(float)"], "cos_twice_fast", "unary", f32, in_cos_twice,
         lambda h: (_cos(2 * h.astype(L)),), re_cos_twice_fast, "abs", "cos2"),
    Case("atan2_fast", [f"{FM}:atan2_fast(float)"], "atan2_fast", "binary", f32, in_atan2_f32, ref_atan2, re_atan2_fast, "abs",
         "atan2", signed_zero=True, seed="atan2f"),
    Case("div_fast", [f"{FM}:div_fast(float)"], "div_fast", "binary", f32, in_div, ref_div, re_div_fast, "rel", "div"),
    Case("SinCosTab_sincos2", [f"{CC}:SinCosTab::sincos2", f"{CC}:SinCosTab::stage", f"{CC}:SinCosTab::lds"], "tab_sincos2",
         "sc2", f64, in_tab, ref_sincos2, re_tab_sincos2, "abs", "sincos2", blocks=TAB_BLOCKS, seed="tab"),
    Case("SinCosTab_lookup2_finish2", [f"{CC}:SinCosTab::lookup2", f"{CC}:SinCosTab::finish2"], "tab_lookup_finish", "sc2",
         f64, in_tab, ref_sincos2, re_tab_sincos2, "abs", "sincos2", blocks=TAB_BLOCKS, seed="tab"),
    Case("SinCosTab_sincos2_wide", [f"{CC}:SinCosTab::sincos2"], "tab_sincos2", "sc2", f64, in_tab_wide, ref_sincos2,
         re_tab_sincos2, "abs", "sincos2", blocks=TAB_BLOCKS),  # (+-1e4 rad: the error is the dropped k lo)
    Case("atan2_f64", [f"{BK}:atan2_f64(double)"], "atan2_f64", "binary", f64, in_atan2_f64, ref_atan2, re_atan2_f64, "abs",
         "atan2", signed_zero=True, seed="atan2d"),
    Case("atan2_f64_xpos", [f"{BK}:atan2_f64(double)"], "atan2_f64_xpos", "binary", f64, in_atan2_f64_xpos, ref_atan2,
         re_atan2_f64_xpos, "abs", "atan2", signed_zero=True, seed="atan2dx"),
    Case("atan2_r_f64", [f"{BK}:atan2_r(double)"], "atan2_r_f64", "binary", f64, in_atan2_f64, ref_atan2, re_atan2_f64, "abs",
         "atan2", signed_zero=True, seed="atan2d"),
    Case("atan2_r_f64_xpos", [f"{BK}:atan2_r(double)"], "atan2_r_f64_xpos", "binary", f64, in_atan2_f64_xpos, ref_atan2,
         re_atan2_f64_xpos, "abs", "atan2", signed_zero=True, seed="atan2dx"),
    Case("atan2_r_f32", [f"{BK}:atan2_r(float)"], "atan2_r_f32", "binary", f32, in_atan2_f32, ref_atan2, re_atan2_fast, "abs",
         "atan2", signed_zero=True, seed="atan2f"),
    Case("sqrt01_f64", [f"{BK}:sqrt01_f64(double)"], "sqrt01_f64", "unary", f64, in_sqrt01, ref_sqrt01, re_sqrt01_f64, "rel",
         "sqrt01"),
    Case("asin_f64", [f"{BK}:asin_f64(double)"], "asin_f64", "unary", f64, in_asin_f64, ref_asin, re_asin_f64, "abs", "asin", seed="asind"),
    Case("asin_r_f64", [f"{BK}:asin_r(double)"], "asin_r_f64", "unary", f64, in_asin_f64, ref_asin, re_asin_f64, "abs", "asin", seed="asind"),
    Case("asin_r_f32", [f"{BK}:asin_r(float)"], "asin_r_f32", "unary", f32, in_asin_f32, ref_asin, re_asin_r_f32, "abs", "asin"),
    Case("qaxis", [f"{BK}:qaxis(int)"], "qaxis", "qaxis", f32, in_qaxis, ref_qaxis, re_qaxis, "abs", None),
]
BY_NAME = {c.name: c for c in CASES}

# Helpers of the three headers that have no case of their own, and why.
NOT_PRIMITIVES = {
    f"{FM}:sconst(double)": "pins a constant in a scalar register; the value is unchanged (inside sincos_fast(double) / sincos2_fast)",
    f"{FM}:sincosf_outlined(float)": "the library call of sincos_fast_pk's fallback: evaluated by the sincos_fast_pk case beyond 1e5",
    f"{FM}:cos_fast_outlined(float)": "cos_fast as a call: evaluated by the cos_twice_fast case beyond 1.85",
    f"{BK}:fma_r(double)": "the fma builtin under the substep's arithmetic type",
    f"{BK}:fma_r(float)": "the fma builtin under the substep's arithmetic type",
}

# E_host per case: the restatement's worst error against the reference over the case's inputs, as measured by
# tests/test_math_primitive_table.py::test_e_host_constants_are_the_measured_ones (which holds each to 0.5 %).
E_HOST = {
    "sincos_fast_f32": 9.224e-08,
    "sincos_fast_pk": 9.226e-08,
    "sincos_fast_smallarg": 9.224e-08,
    "sincos_fast_f64": 1.730e-16,
    "sincos_fast_f64_nofallback": 1.721e-16,
    "sincos2_fast": 1.721e-16,
    "rcp_fast": 1.110e-16,
    "rcp_fast1": 3.664e-15,
    "cos_fast": 9.224e-08,
    "cos_twice_fast": 1.590e-07,
    "atan2_fast": 3.408e-07,
    "div_fast": 2.298e-07,
    "SinCosTab_sincos2": 7.370e-14,
    "SinCosTab_lookup2_finish2": 7.370e-14,
    "SinCosTab_sincos2_wide": 4.208e-13,
    "atan2_f64": 2.727e-13,
    "atan2_f64_xpos": 2.725e-13,
    "atan2_r_f64": 2.727e-13,
    "atan2_r_f64_xpos": 2.725e-13,
    "atan2_r_f32": 3.408e-07,
    "sqrt01_f64": 1.109e-16,
    "asin_f64": 2.722e-13,
    "asin_r_f64": 2.722e-13,
    "asin_r_f32": 2.976e-07,
    "qaxis": 9.178e-08,
}

# Pairs whose outputs must agree bit for bit (no tolerance): (case a, case b, how b's inputs / outputs map onto a's).
BIT_IDENTICAL = [
    ("sincos_fast_smallarg", "sincos_fast_f32"),            # the header: "the same bits as sincos_fast"
    ("SinCosTab_lookup2_finish2", "SinCosTab_sincos2"),     # "same operations, same values as sincos2"
    ("atan2_r_f64", "atan2_f64"), ("atan2_r_f64_xpos", "atan2_f64_xpos"), ("atan2_r_f32", "atan2_fast"),
    ("asin_r_f64", "asin_f64"),                             # the _r forms are aliases by arithmetic type
]
# Primitives with a ballot-guarded branch: a lane's result must not depend on its wave mates.
BALLOT_GUARDED = ["sincos_fast_f32", "sincos_fast_pk", "sincos_fast_smallarg", "cos_twice_fast"]


def header_primitives():
    """`file:function(first argument type)` of every device math function in the three headers, read off the source:
    all of fast_math.hip.h, SinCosTab's members, and brax_kernels.hip.h's functions from scalars to a scalar / quaternion"""
    found = set()
    fn = re.compile(r"^(?:template <[^>]*>\s*\n)?\s*(?:__host__ )?__device__ (?:__forceinline__ |static |__attribute__\(\(noinline\)\) )*"
                    r"([\w:]+\*?) (\w+)\(([^)]*)\)\s*\{", re.M)
    for m in fn.finditer(open(os.path.join(CSRC, FM)).read()):
        found.add(f"{FM}:{m.group(2)}({m.group(3).split()[0]})")
    cc = open(os.path.join(CSRC, CC)).read()
    body = cc.split("struct SinCosTab {")[1].split("\n};")[0]
    for m in fn.finditer(body):
        found.add(f"{CC}:SinCosTab::{m.group(2)}")
    for m in fn.finditer(open(os.path.join(CSRC, BK)).read()):
        params = [p.strip() for p in m.group(3).split(",") if p.strip()]
        if m.group(1) in ("float", "double", "qt") and params and all(re.fullmatch(r"(?:const )?(float|double|int) \w+", p) for p in params):
            found.add(f"{BK}:{m.group(2)}({params[0].split()[-2]})")
    return found
