"""carl_policy_stats_merge on the GPU from synthetic slabs: the launch is called directly, as InputStats.update calls
it, with slabs, steps, running state and parameter blocks built here -- shapes, counts, floors, the clamp and what is
written that no real evaluation launch produces.  Two references.

1. The same order: stats_ref.merge, the header's operations in NumPy float64.  Mean and M2 at rtol = 1e-12 (the
   tolerance of test_gpu_policy_stats.py), the fp32 shift and scale bit for bit.  Every case is built so that the
   reference's own float64 values are not within that tolerance of an fp32 rounding boundary or of a floor
   (stats_ref.settled, asserted on the host); the floor cases are built from dyadic numbers instead, where both sides of
   the comparison are exact.

2. Exact arithmetic: integer data under integer shifts (stats_ref.exact_cases), so that every slab entry and every
   partial sum of the workgroup-order loop is an exact float64, against the pooled mean and M2 of everything merged, in
   rational arithmetic, over up to three successive merges.  The bound (stats_ref.exact_merge) follows from the header's
   operation list.  Write u = 2^-53 for one float64 rounding, n = n_a + n_b, and for a launch (S1, S2 exact)
       mu_b = shift + S1 / n_b,   M_b = S2 - S1^2 / n_b >= 0       (exact)
   * mean_b = fl(shift + fl(S1 / n_b)): two roundings, of S1 / n_b and of the sum, so
         E_b = u (|S1| / n_b + |mu_b|).
   * M2_b = fl(S2 - fl(fl(S1 S1) / n_b)): the subtrahend carries two roundings of S1^2 / n_b -- the term S2 cancels
     against -- and the difference one of its own:
         G_b = u (2 S1^2 / n_b + M_b).
     The exact M_b is not negative, so the clamp at 0 moves the result towards it.
   * count == 0: the state is (mean_b, M2_b) with (E_b, G_b).
   * Chan's update of a state (mean_a, M2_a) that is within (E_a, F_a) of the exact (mu_a, M_a), with the exact
     delta = mu_b - mu_a, f = n_a n_b / n and T = f delta^2:
       - the computed delta is fl(mean_b - mean_a): E_d = E_b + E_a + u |delta|;
       - mean = fl(mean_a + fl(delta' fl(n_b / n))): to first order its error is err_a + (n_b / n) (err_b - err_a + 3 u
         delta) + u mu, the three roundings of delta', n_b / n and their product, and one of the sum:
             E_mean = (n_a / n) E_a + (n_b / n) (E_b + 3 u |delta|) + u |mu|;
       - M2 = fl(fl(M2_a + M2_b) + fl(fl(delta' delta') fl(fl(n_a n_b) / n))): the first sum carries F_a + G_b and one
         rounding of M_a + M_b; the product carries four roundings of T and the running mean's error through
         delta'^2 - delta^2, at most E_d (2 |delta| + E_d) -- kept whole, since with delta = 0 its second-order part is
         all there is; the last sum rounds M = M_a + M_b + T once:
             E_M2 = F_a + G_b + u (2 (M_a + M_b) + 5 T) + f E_d (2 |delta| + E_d).
   Every other higher-order term is a first-order term times a few u; u is taken as 2^-53 (1 + 2^-20) to cover them,
   which holds while neither n_a nor n_b is a smaller share of n than 2^-20 (asserted).  stats_ref.merge stays inside
   this bound on every case (test_policy_stats_reference.py, on the host); the device is held to the same bound here.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import stats_ref as SR
from carl_amd import _lib

pytestmark = pytest.mark.gpu

RTOL = 1e-12
CANARY = -7.25  # behind n_in in mean / m2
EPS, MIN_STD = 1e-8, 1e-6  # InputStats' defaults
SHAPES = {1: (), 12: (5,), 32: (7, 3)}  # n_in -> hidden widths: the transform section sits behind other floats
N_OUT = 2


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Merge:
    """the device side of a sequence of merges over one shape: the running state (canaries behind n_in), a policy block
    of `n_sets` packed weight sets the launch reads its shift from (set 0), and the call itself"""

    def __init__(self, device, n_in, n_sets=1, count=0, mean=None, m2=None, seed=0):
        self.device, self.n_in, self.widths = device, n_in, SHAPES[n_in]
        self.p_shift, self.p_scale, self.p_clip, self.S = SR.transform_offsets(n_in, self.widths, N_OUT)
        rng = np.random.default_rng(seed)
        host = rng.normal(size=(n_sets, self.S)).astype(np.float32)
        host[:, self.p_shift: self.p_scale] = 0.0
        host[:, self.p_scale: self.p_clip] = 1.0
        host[:, self.p_clip] = np.inf
        self.block = torch.from_numpy(host).to(device)
        state = np.full((2, SR.MAX_IN), CANARY)
        state[:, :n_in] = 0.0
        if mean is not None:
            state[0, :n_in], state[1, :n_in] = mean, m2
        self.mean, self.m2 = (torch.from_numpy(state[k].copy()).to(device) for k in (0, 1))
        self.count = torch.tensor([count], dtype=torch.int64, device=device)

    def set_shift(self, shift, sets=slice(None)):
        self.block[sets, self.p_shift: self.p_scale] = torch.from_numpy(np.asarray(shift, np.float32)).to(self.device)

    def policy(self, n_lanes):
        p = _lib.Policy()
        p.n_in, p.n_ctx, p.n_hidden, p.n_out = self.n_in, 0, len(self.widths), N_OUT
        for k, w in enumerate(self.widths):
            p.width[k] = w
        p.activation, p.head = _lib.POLICY_TANH, _lib.POLICY_HEAD_ARGMAX
        p.n_sets, p.lanes_per_set, p.params = self.block.shape[0], max(256, n_lanes), self.block.data_ptr()
        return p

    def run(self, partial, steps, out="own", n_write=1, eps=EPS, min_std=MIN_STD):
        """one launch; out: "own" (the policy's block), None, or a float32 [k, S] device tensor"""
        lib = _lib.load()
        assert partial.shape[1:] == (2, SR.MAX_IN) and partial.dtype == np.float64 and steps.dtype == np.int32
        part = torch.from_numpy(np.ascontiguousarray(partial)).to(self.device)
        if part.numel() == 0:
            part = torch.zeros((1, 2, SR.MAX_IN), dtype=torch.float64, device=self.device)
        st = torch.from_numpy(steps).to(self.device)
        target = self.block if isinstance(out, str) else out
        pol = self.policy(int(steps.size))
        stats = _lib.PolicyStats(part.data_ptr(), int(part.shape[0]))
        run = _lib.PolicyRunningStats(self.count.data_ptr(), self.mean.data_ptr(), self.m2.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(lib.carl_policy_stats_merge(
                C.byref(pol), C.byref(stats), int(partial.shape[0]), st.data_ptr(), int(steps.size), C.byref(run),
                eps, min_std, None if target is None else target.data_ptr(), n_write,
                torch.cuda.current_stream(self.device).cuda_stream))
        torch.cuda.synchronize(self.device)

    def state(self):
        """{"count", "mean", "m2"} of the first n_in inputs, after checking that the entries behind them kept their bits"""
        mean, m2 = self.mean.cpu().numpy(), self.m2.cpu().numpy()
        assert (mean[self.n_in:] == CANARY).all() and (m2[self.n_in:] == CANARY).all(), "wrote behind n_in"
        return {"count": int(self.count.item()), "mean": mean[: self.n_in], "m2": m2[: self.n_in]}

    def section(self, block=None):
        b = (self.block if block is None else block).cpu().numpy()
        return b[:, self.p_shift: self.p_scale], b[:, self.p_scale: self.p_clip]


def consistent_slabs(rng, W, n_b, n_in, loc, spread, shift):
    """W slabs that share n_b lane-steps: slab w holds c_w steps of mean m_w and variance v_w of each input, so S1 = c_w
    (m_w - shift) and S2 = c_w (v_w + (m_w - shift)^2) -- non-integers, rounded as they fall; NaN at and beyond n_in"""
    c = rng.multinomial(n_b, np.full(W, 1.0 / W)).astype(np.float64)[:, None]
    m = loc + spread * rng.normal(size=(W, n_in)) * 0.3 - shift.astype(np.float64)
    v = (spread * rng.uniform(0.5, 1.5, (W, n_in))) ** 2
    partial = np.full((W, 2, SR.MAX_IN), np.nan)
    partial[:, 0, :n_in], partial[:, 1, :n_in] = c * m, c * (v + m * m)
    return partial


def spread_steps(rng, n_lanes, top):
    steps = rng.integers(0, top + 1, n_lanes).astype(np.int32)
    steps[0] = max(steps[0], 1)
    return steps


def assert_same_order(mg, ref, sh, sc, eps=EPS, min_std=MIN_STD, sets=slice(0, 1)):
    """the device's state against stats_ref.merge's (ref, sh, sc) at RTOL; the written fp32 shift and scale bit for bit"""
    assert SR.settled(ref, eps, min_std, 4 * RTOL).all(), "the case sits on a rounding boundary: choose another seed"
    got = mg.state()
    assert got["count"] == ref["count"]
    np.testing.assert_allclose(got["mean"], ref["mean"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(got["m2"], ref["m2"], rtol=RTOL, atol=0)
    assert (got["m2"] >= 0).all()
    shift, scale = mg.section()
    for k in range(shift.shape[0])[sets]:
        np.testing.assert_array_equal(as_bits(shift[k]), as_bits(sh))
        np.testing.assert_array_equal(as_bits(scale[k]), as_bits(sc))


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("n_in", [1, 12, 32])
@pytest.mark.parametrize("n_lanes", [1, 255, 257, 1000])
@pytest.mark.parametrize("W", [1, 2, 257])
def test_shapes_against_the_same_order(device, W, n_lanes, n_in):
    """two successive merges (the first into an empty state, the second Chan's update) of W slabs and n_lanes lanes of
    steps: 255 and 257 lanes leave the strided count one thread short and one over, 1000 gives threads 3 or 4 lanes"""
    rng = np.random.default_rng(10000 * W + 10 * n_lanes + n_in)
    loc, spread = rng.uniform(-20, 20, n_in), rng.uniform(0.05, 5, n_in)
    mg = Merge(device, n_in, seed=W + n_lanes)
    ref = SR.fresh(n_in)
    shift = np.zeros(n_in, np.float32)
    for launch in range(2):
        steps = spread_steps(rng, n_lanes, 40)
        n_b = int(steps.sum())
        partial = consistent_slabs(rng, W, n_b, n_in, loc + launch * spread, spread, shift)
        before = mg.block.clone()
        mg.run(partial, steps)
        ref, sh, sc = SR.merge(ref, partial, n_b, shift, EPS, MIN_STD)
        assert_same_order(mg, ref, sh, sc)
        assert (sc > 0).all()
        keep = np.ones(mg.S, bool)
        keep[mg.p_shift: mg.p_clip] = False
        np.testing.assert_array_equal(as_bits(mg.block.cpu().numpy()[:, keep]), as_bits(before.cpu().numpy()[:, keep]))
        shift = sh  # the next launch runs under the shift this one wrote, read from the block it is written to again


# ---------------------------------------------------------------- counts
def test_a_step_count_beyond_int32(device):
    """three lanes of 2^30 steps: n_b = 3 * 2^30 does not fit 32 bits"""
    n_in, rng = 12, np.random.default_rng(1)
    steps = np.array([0, 2 ** 30, 0, 2 ** 30, 2 ** 30] + [0] * 300, np.int32)
    n_b = 3 * 2 ** 30
    shift = rng.normal(size=n_in).astype(np.float32)
    mg = Merge(device, n_in)
    mg.set_shift(shift)
    partial = consistent_slabs(rng, 2, n_b, n_in, rng.uniform(-3, 3, n_in), rng.uniform(0.1, 2, n_in), shift)
    mg.run(partial, steps)
    ref, sh, sc = SR.merge(SR.fresh(n_in), partial, n_b, shift, EPS, MIN_STD)
    assert ref["count"] == n_b > 2 ** 31
    assert_same_order(mg, ref, sh, sc)
    mg.run(partial, steps)  # ... and a running count beyond 2^32 after the second
    ref, sh, sc = SR.merge(ref, partial, n_b, sh, EPS, MIN_STD)
    assert ref["count"] == 6 * 2 ** 30
    assert_same_order(mg, ref, sh, sc)


def test_a_running_count_of_2_to_the_40(device):
    """n_a = 2^40 lane-steps and n_b = 1 234: Chan's update with n_a >> n_b moves the mean by delta n_b / n and keeps
    the running M2's leading bits"""
    n_in, rng, n_a = 12, np.random.default_rng(2), 2 ** 40
    mean_a, var_a = rng.uniform(-5, 5, n_in), rng.uniform(0.1, 4, n_in)
    mg = Merge(device, n_in, count=n_a, mean=mean_a, m2=var_a * n_a)
    shift = mean_a.astype(np.float32)
    mg.set_shift(shift)
    steps = np.zeros(257, np.int32)
    steps[[0, 100, 256]] = [1000, 200, 34]
    partial = consistent_slabs(rng, 2, 1234, n_in, mean_a + 3.0, np.sqrt(var_a), shift)
    mg.run(partial, steps)
    ref, sh, sc = SR.merge({"count": n_a, "mean": mean_a, "m2": var_a * n_a}, partial, 1234, shift, EPS, MIN_STD)
    assert ref["count"] == n_a + 1234
    assert_same_order(mg, ref, sh, sc)
    moved = (ref["mean"] - mean_a) / (3.0 * 1234 / n_a)
    assert np.all(np.abs(moved - 1) < 0.5)  # (the reference itself moved by about delta n_b / n, not by delta)


def test_an_empty_launch_keeps_every_bit(device):
    """n_b == 0 with non-zero slabs: nothing is read further, nothing is written"""
    n_in, rng = 12, np.random.default_rng(3)
    for count in (0, 5000):
        mg = Merge(device, n_in, n_sets=3, count=count, mean=rng.normal(size=n_in), m2=rng.uniform(1, 2, n_in) * count)
        before = [t.clone() for t in (mg.count, mg.mean, mg.m2, mg.block)]
        partial = consistent_slabs(rng, 2, 777, n_in, np.ones(n_in), np.ones(n_in), np.zeros(n_in, np.float32))
        mg.run(partial, np.zeros(300, np.int32), n_write=3)
        mg.run(partial, np.zeros(0, np.int32), n_write=3)
        for a, b in zip(before, (mg.count, mg.mean, mg.m2, mg.block)):
            np.testing.assert_array_equal(as_bits(a.cpu().numpy()), as_bits(b.cpu().numpy()))


# ---------------------------------------------------------------- the floors, from dyadic numbers
def one_column(device, shift, s1, s2, n_b, eps, min_std):
    """a first merge of one input in one slab over n_b lanes of one step -> (state, fp32 shift, fp32 scale)"""
    mg = Merge(device, 1)
    mg.set_shift([shift])
    partial = np.full((1, 2, SR.MAX_IN), np.nan)
    partial[0, 0, 0], partial[0, 1, 0] = s1, s2
    mg.run(partial, np.ones(n_b, np.int32), eps=eps, min_std=min_std)
    sh, sc = mg.section()
    return mg.state(), sh[0, 0], sc[0, 0]


FLOORS = {  # name: (shift, n_b, var at the floor, min_std, eps); S1 = 0, so mean = shift and var = S2 / n_b, exactly
    "min_std": (0.0, 16, 2.0 ** -20, 2.0 ** -10, EPS),              # var == min_std^2
    "relative": (2.0 ** 10, 16, 2.0 ** -16, MIN_STD, EPS),          # var == (2^-18 * 2^10)^2 > min_std^2
    "relative_negative_mean": (-2.0 ** 10, 64, 2.0 ** -16, 0.0, EPS),
    "min_std_eps_0": (0.0, 16, 2.0 ** -40, 2.0 ** -20, 0.0),
}


@pytest.mark.parametrize("name", list(FLOORS))
def test_the_floor_is_inclusive(device, name):
    """var == floor gives scale 0; one ulp of S2 above it gives 1 / sqrt(var + eps) (n_b is a power of two: one ulp of
    S2 is one ulp of var)"""
    shift, n_b, var, min_std, eps = FLOORS[name]
    s2 = var * n_b
    floor = max(min_std * min_std, (SR.REL_FLOOR * abs(shift)) ** 2)
    assert floor == var and s2 / n_b == var and np.nextafter(s2, np.inf) / n_b == np.nextafter(var, np.inf)
    st, sh, sc = one_column(device, shift, 0.0, s2, n_b, eps, min_std)
    assert st["count"] == n_b and st["mean"][0] == shift and st["m2"][0] == s2 and sh == np.float32(shift)
    assert as_bits(np.float32(sc)) == 0  # +0.0
    st, sh, sc = one_column(device, shift, 0.0, np.nextafter(s2, np.inf), n_b, eps, min_std)
    want = np.float32(1.0 / np.sqrt(np.nextafter(var, np.inf) + eps))
    assert st["m2"][0] == np.nextafter(s2, np.inf)
    assert np.isfinite(want) and want > 0 and as_bits(np.float32(sc)) == as_bits(want), (sc, want)
    # one ulp below the floor is constant as well
    st, sh, sc = one_column(device, shift, 0.0, np.nextafter(s2, 0.0), n_b, eps, min_std)
    assert as_bits(np.float32(sc)) == 0


def test_a_zero_floor_and_a_zero_variance(device):
    """min_std = 0, mean = 0, var = 0: 0 <= 0, scale 0 -- with eps > 0 (a strict comparison would give 1 / sqrt(eps))
    and with eps = 0 (it would give inf)"""
    for eps in (EPS, 0.0):
        st, sh, sc = one_column(device, 0.0, 0.0, 0.0, 16, eps, 0.0)
        assert st["m2"][0] == 0 and st["mean"][0] == 0 and as_bits(np.float32(sc)) == 0
        # the smallest variance above a zero floor that still has a finite fp32 scale without eps: 2^-254 -> 2^127
        for var in (2.0 ** -254, 2.0 ** -100):
            st, sh, sc = one_column(device, 0.0, 0.0, var * 16, 16, 0.0, 0.0)
            assert as_bits(np.float32(sc)) == as_bits(np.float32(1.0 / np.sqrt(var))) and np.isfinite(sc) and sc > 0


# ---------------------------------------------------------------- the clamp
@pytest.mark.parametrize("d, n_b", [(3.0, 48), (0.1, 1000), (-9.8, 257)])
def test_a_constant_input_one_ulp_short_clamps_to_zero(device, d, n_b):
    """a constant d whose S2 arrives one ulp below S1^2 / n_b: M2 = 0 and scale 0, never negative, never NaN -- also as
    the second merge of two, where M2 stays what it was"""
    s1 = d * n_b
    s2 = np.nextafter(s1 * s1 / n_b, 0.0)
    assert s2 - s1 * s1 / n_b < 0
    st, sh, sc = one_column(device, 1.0, s1, s2, n_b, EPS, MIN_STD)
    assert as_bits(st["m2"])[0] == 0 and as_bits(np.float32(sc)) == 0
    assert st["mean"][0] == 1.0 + s1 / n_b and sh == np.float32(1.0 + s1 / n_b)
    mean_a = 1.0 + s1 / n_b
    mg = Merge(device, 1, count=1000, mean=[mean_a], m2=[250.0])
    mg.set_shift([1.0])
    partial = np.full((1, 2, SR.MAX_IN), np.nan)
    partial[0, 0, 0], partial[0, 1, 0] = s1, s2
    mg.run(partial, np.full(1, n_b, np.int32))
    st = mg.state()
    assert st["count"] == 1000 + n_b and st["mean"][0] == mean_a and st["m2"][0] == 250.0  # delta == 0, M2_b == 0
    assert mg.section()[1][0, 0] == np.float32(1.0 / np.sqrt(250.0 / (1000 + n_b) + EPS))


# ---------------------------------------------------------------- what is written
@pytest.mark.parametrize("target", ["own", "other", "none"])
@pytest.mark.parametrize("n_write", [0, 1, 3])
def test_what_a_merge_writes(device, n_write, target):
    """n_write of three blocks receive the shift | scale section and nothing else; params_out = NULL writes the state
    only; params_out = the policy's own block reads the shift from the floats it then overwrites"""
    n_in, rng = 12, np.random.default_rng(40 + n_write)
    mg = Merge(device, n_in, n_sets=3, seed=5)
    shift = rng.normal(size=n_in).astype(np.float32)
    mg.set_shift(shift, sets=slice(0, 1))
    mg.set_shift(shift + 100, sets=slice(1, 3))  # (the launch reads set 0's)
    other = torch.from_numpy(rng.normal(size=(3, mg.S)).astype(np.float32)).to(device)
    out = {"own": "own", "other": other, "none": None}[target]
    steps = spread_steps(rng, 257, 20)
    n_b = int(steps.sum())
    partial = consistent_slabs(rng, 2, n_b, n_in, rng.uniform(-3, 3, n_in), rng.uniform(0.1, 2, n_in), shift)
    own_before, other_before = mg.block.cpu().numpy().copy(), other.cpu().numpy().copy()
    mg.run(partial, steps, out=out, n_write=n_write)
    ref, sh, sc = SR.merge(SR.fresh(n_in), partial, n_b, shift, EPS, MIN_STD)
    assert SR.settled(ref, EPS, MIN_STD, 4 * RTOL).all()
    got = mg.state()
    assert got["count"] == n_b
    np.testing.assert_allclose(got["mean"], ref["mean"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(got["m2"], ref["m2"], rtol=RTOL, atol=0)
    want_own, want_other = own_before.copy(), other_before.copy()
    written = {"own": want_own, "other": want_other, "none": None}[target]
    if written is not None:
        written[:n_write, mg.p_shift: mg.p_scale] = sh
        written[:n_write, mg.p_scale: mg.p_clip] = sc
    np.testing.assert_array_equal(as_bits(mg.block.cpu().numpy()), as_bits(want_own))
    np.testing.assert_array_equal(as_bits(other.cpu().numpy()), as_bits(want_other))


# ---------------------------------------------------------------- exact arithmetic
@pytest.fixture(scope="module")
def exact_cases():
    return SR.exact_cases()


def test_integer_data_against_exact_arithmetic(device, exact_cases, capsys):
    """module docstring, 2.: every case of stats_ref.exact_cases, the device held to the derived bound after each of
    its merges"""
    worst = [0.0, 0.0]
    for n_in, launches, (tot_n, _, _) in exact_cases:
        mg = Merge(device, n_in)
        ex = SR.exact_fresh(n_in)
        for partial, steps, shift in launches:
            mg.set_shift(shift)
            mg.run(partial, steps)
            ex = SR.exact_merge(ex, partial, int(steps.astype(np.int64).sum()), shift)
            st = mg.state()
            r = SR.exact_ratio(ex, st["mean"], st["m2"])
            worst = [max(a, b) for a, b in zip(worst, r)]
            assert st["count"] == ex["count"] and (st["m2"] >= 0).all()
            assert max(r) <= 1.0, (n_in, len(launches), r)
        assert st["count"] == tot_n
    with capsys.disabled():
        print(f"\ncarl_policy_stats_merge against exact arithmetic: worst |err| / bound {worst[0]:.3f} (mean), "
              f"{worst[1]:.3f} (M2)")
