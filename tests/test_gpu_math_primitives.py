"""Every device math primitive, evaluated on its own on the device (tests/probe/math_probe.hip through tests/math_probe.py)
against the exact reference of tests/math_primitive_cases.py -- needs an MI355X.

The bar of each case is 2 E_host + one ulp of the result type (cases module docstring): it comes from the host restatement
of the formula and the documented accuracy of the hardware seeds, never from what the device returns.  Measured device
worst per case (printed by test_accuracy; DESIGN.md section 7 has the table beside E_host and the bar).

Bit-identity checks have no tolerance.  The reciprocals at d = +-0 / +-inf are evaluated and printed as documented
behaviour (fast_math.hip.h), not held to a bar."""
import numpy as np
import pytest

import math_primitive_cases as M
import math_probe as P

pytestmark = pytest.mark.gpu

_CACHE = {}


def device_outputs(case, block, device):
    key = (case.name, block)
    if key not in _CACHE:
        _CACHE[key] = P.run(case.entry, case.kind, case.inputs(), case.dtype, device, block=block)
    return _CACHE[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


ACCURACY = [(c, b) for c in M.CASES for b in c.blocks]


@pytest.mark.parametrize("case,block", ACCURACY, ids=[f"{c.name}-b{b}" for c, b in ACCURACY])
def test_accuracy(case, block, device):
    outs = device_outputs(case, block, device)
    refs = case.reference()
    worst, worst_ratio = 0.0, 0.0
    for got, ref in zip(outs, refs):
        assert got.dtype == case.dtype and got.shape == ref.shape
        err, bound = case.error(got, ref), case.bound(ref)
        if case.measure == "rel":  # the bound is absolute (2 E |ref| + ulp): bring the measured relative error to it
            err = np.where(np.isfinite(err), err * np.where(ref != 0, np.abs(ref), 1), err)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{case.name}: NaN exactly where the reference has none"
        fin = ~np.isnan(ref)
        worst = max(worst, float(case.error(got, ref)[fin].max()))
        ratio = np.where(fin, err / np.where(bound > 0, bound, 1), 0)
        worst_ratio = max(worst_ratio, float(ratio.max()))
        i = int(np.unravel_index(np.argmax(ratio), ratio.shape)[0])
        assert (err[fin] <= bound[fin]).all(), (case.name, i, [a[i] for a in case.inputs()], got[i], ref[i], float(ratio.max()))
        if case.signed_zero:
            z = (ref == 0)
            assert np.array_equal(np.signbit(got[z]), np.signbit(ref[z])), f"{case.name}: sign of a zero result"
    print(f"{case.name} block {block}: device worst {worst:.3e} ({case.measure}), E_host {M.E_HOST[case.name]:.3e}, "
          f"worst error / bar {worst_ratio:.2f}", flush=True)


@pytest.mark.parametrize("a,b", M.BIT_IDENTICAL, ids=[f"{a}=={b}" for a, b in M.BIT_IDENTICAL])
def test_bit_identity(a, b, device):
    ca, cb = M.BY_NAME[a], M.BY_NAME[b]
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(ca.inputs(), cb.inputs()))
    for block in ca.blocks:
        for x, y in zip(device_outputs(ca, block, device), device_outputs(cb, block, device)):
            same = bits(x) == bits(y)
            assert same.all(), (a, b, block, int((~same).sum()), [v[int(np.argmin(same))] for v in ca.inputs()])


def test_sincos2_fast_is_sincos_fast_without_fallback_on_both_halves(device):
    """`sincos2_fast`: "same operations and constants as sincos_fast<false>: bit-identical results" -- on either half, and
    with the halves swapped"""
    c2, c1 = M.BY_NAME["sincos2_fast"], M.BY_NAME["sincos_fast_f64_nofallback"]
    xa, xb = c2.inputs()
    sa, ca, sb, cb = device_outputs(c2, 256, device)
    s1, c1a = device_outputs(c1, 256, device)
    assert np.array_equal(bits(xa), bits(c1.inputs()[0]))
    assert np.array_equal(bits(sa), bits(s1)) and np.array_equal(bits(ca), bits(c1a))
    sbb, cbb = P.run(c1.entry, c1.kind, (xb,), c1.dtype, device)
    assert np.array_equal(bits(sb), bits(sbb)) and np.array_equal(bits(cb), bits(cbb))
    w = P.run(c2.entry, c2.kind, (xb, xa), c2.dtype, device)
    for got, want in zip(w, (sb, cb, sa, ca)):
        assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("block", M.TAB_BLOCKS)
def test_staged_table_and_lookup(block, device):
    """SinCosTab::stage copies the whole table into every workgroup's LDS whatever the workgroup size, and lookup2 reads
    the entry of the nearest grid point (negative angles: the low dword of a two's-complement sum, masked) and leaves
    the reduced argument the restatement computes -- over +-40 rad and over +-1e4 rad."""
    _, tab = M.sincos_table()
    got = P.staged_table(device, 5, block)
    assert got.shape == (5,) + tab.shape
    assert all(np.array_equal(bits(g), bits(tab)) for g in got)
    for name in ("SinCosTab_sincos2", "SinCosTab_sincos2_wide"):
        xa, xb = M.BY_NAME[name].inputs()
        (out,) = P.run("tab_lookup2", "lookup2", (xa, xb), np.float64, device, block=block)
        for x, cols, rcol in ((xa, (0, 1), 4), (xb, (2, 3), 5)):
            i, r = M.tab_lookup(x)
            step = np.pi / 256
            near = np.rint(x / step)
            d = np.abs(i - (near.astype(np.int64) & (tab.shape[0] - 1)))
            assert (np.minimum(d, tab.shape[0] - d) <= 1).all()  # circular distance (off by one only at a half-step tie)
            assert (np.abs(r) <= step / 2 * (1 + 1e-9) + np.abs(x) * 2e-16).all()
            assert np.array_equal(bits(out[:, cols[0]]), bits(tab[i, 0])) and np.array_equal(bits(out[:, cols[1]]), bits(tab[i, 1])), name
            assert np.array_equal(bits(out[:, rcol]), bits(r)), name


def _arrangements(fast, slow, rng):
    """the same values in three orders: waves uniformly fast or uniformly slow; one slow lane per wave of 64; shuffled"""
    n_w = slow.size
    fast = fast[: n_w * 63]
    sorted_ = np.concatenate([fast, slow])
    one = np.concatenate([fast.reshape(n_w, 63), slow[:, None]], axis=1)
    one = np.stack([np.roll(row, w % 64) for w, row in enumerate(one)]).ravel()  # the slow lane moves through the wave
    return [sorted_, one, rng.permutation(sorted_)]


@pytest.mark.parametrize("name", M.BALLOT_GUARDED)
def test_wave_independence(name, device):
    """the ballot-guarded fallbacks: a lane's result must not depend on whether a wave mate takes the slow path"""
    case = M.BY_NAME[name]
    (x,) = case.inputs()
    guard = {"sincos_fast_smallarg": 0.78, "cos_twice_fast": 1.85}.get(name, 1.0e5)
    rng = np.random.default_rng(11)
    slow_all = x[~(np.abs(x) <= np.float32(guard))]
    fast_all = x[np.abs(x) <= np.float32(guard)]
    slow = rng.choice(slow_all, 1024)
    slow[:4] = [np.nan, np.inf, -np.inf, np.nextafter(np.float32(guard), np.float32(np.inf))]
    fast = rng.choice(fast_all, 1024 * 63)
    fast[:2] = [np.float32(guard), -np.float32(guard)]
    assert fast.size % 64 == 0 and slow.size % 64 == 0  # "sorted": no wave mixes the two kinds
    table = {}
    for k, arr in enumerate(_arrangements(fast.astype(np.float32), slow.astype(np.float32), rng)):
        outs = P.run(case.entry, case.kind, (arr,), case.dtype, device)
        packed = np.stack([bits(o).astype(np.uint64) for o in outs], 1)
        order = np.argsort(bits(arr), kind="stable")
        key, val = bits(arr)[order], packed[order]
        if k == 0:
            first = np.concatenate([[True], key[1:] != key[:-1]])
            table = dict(zip(key[first].tolist(), map(tuple, val[first].tolist())))
        # NaN results compare by bits too: the library path is deterministic per input
        bad = [(kk, tuple(vv)) for kk, vv in zip(key.tolist(), val.tolist()) if table[kk] != tuple(vv)]
        assert not bad, (name, k, len(bad), bad[:3])


TAIL = 300
PARTIAL = sorted({(c.entry, c.kind): c for c in M.CASES}.values(), key=lambda c: c.name)  # one case per kernel


@pytest.mark.parametrize("n", [1003, 65])
@pytest.mark.parametrize("case", PARTIAL, ids=[c.name for c in PARTIAL])
def test_partial_last_wave_and_workgroup(case, n, device):
    """n is no multiple of the wave or the workgroup: the first n outputs are those of the full run, and the canaries
    behind them are untouched"""
    full = device_outputs(case, case.blocks[-1], device)
    outs = P.run(case.entry, case.kind, case.inputs(), case.dtype, device, block=case.blocks[-1], n=n, tail=TAIL)
    canary = bits(np.full(1, P.CANARY[np.dtype(case.dtype)], case.dtype))[0]
    for got, want in zip(outs, full):
        assert got.shape[0] == n + TAIL
        assert np.array_equal(bits(got[:n]), bits(want[:n]))
        assert (bits(got[n:]) == canary).all()


def test_reciprocals_at_zero_and_infinity_documented_behaviour(device):
    """d = +-0 and +-inf: v_rcp_f64 returns +-inf / +-0 and the Newton step's fma(-d, r, 1) is 0 x inf = NaN.  Documented in
    fast_math.hip.h (the callers' divisors -- a determinant, a norm -- are finite and non-zero); printed, not held to a bar."""
    d = M.RCP_DOCUMENTED_POINTS
    for entry in ("rcp_fast", "rcp_fast1"):
        (r,) = P.run(entry, "unary", (d,), np.float64, device)
        print(f"{entry}({d.tolist()}) = {r.tolist()}", flush=True)
        assert r.shape == d.shape
