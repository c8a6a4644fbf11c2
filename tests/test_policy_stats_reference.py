"""The host reference of the input statistics (stats_ref.py) against plain NumPy, and the Python layer's host-side rules
(InputStats, the transform offsets).  CPU-only."""
import numpy as np
import pytest

import stats_ref as SR
from carl_amd import _lib
from carl_amd.policy import InputStats, MLPPolicy
from policy_cases import HIDDEN_SHAPES, fake_engine, rand_layers


def launch(rng, T, n, n_in, shift, loc, spread):
    """a launch's worth of inputs: x [T, n, n_in], steps [n], its one-workgroup-per-256-lanes partials and n_b"""
    x = (loc + spread * rng.normal(size=(T, n, n_in))).astype(np.float32)
    steps = rng.integers(0, T + 1, n)
    n_wg = (n + 255) // 256
    partial = np.zeros((n_wg, 2, SR.MAX_IN))
    for w in range(n_wg):
        lanes = slice(256 * w, min(n, 256 * w + 256))
        s1, s2, _ = SR.input_sums(x[:, lanes], steps[lanes], shift)
        partial[w, 0, :n_in], partial[w, 1, :n_in] = s1, s2
    return x, steps, partial, int(steps.sum())


def visited(x, steps, shift):
    """the values the statistics are defined over: shift + fp32(x - shift) of the live lane-steps, in float64"""
    live = np.arange(x.shape[0])[:, None] < steps[None, :]
    return shift.astype(np.float64) + (x[live] - shift).astype(np.float32).astype(np.float64)


def test_merging_two_halves_equals_the_whole():
    rng = np.random.default_rng(0)
    n_in = 9
    loc = np.array([9.8, 0.1, 10, 8, 1, 0, -3, 100, 0.5])
    spread = np.array([0.5, 0.01, 1, 2, 1, 1, 4, 30, 0.2])
    shift0 = np.zeros(n_in, np.float32)
    xa, sa, pa, na = launch(rng, 40, 300, n_in, shift0, loc, spread)
    st, shift1, scale1 = SR.merge(SR.fresh(n_in), pa, na, shift0)
    # the second launch runs under the shift the first one produced, as an ES generation does
    xb, sb, pb, nb = launch(rng, 33, 515, n_in, shift1, loc + 0.3 * spread, spread)
    st, shift2, scale2 = SR.merge(st, pb, nb, shift1)
    allx = np.concatenate([visited(xa, sa, shift0), visited(xb, sb, shift1)])
    assert st["count"] == allx.shape[0] == na + nb
    np.testing.assert_allclose(st["mean"], allx.mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(st["m2"], ((allx - allx.mean(axis=0)) ** 2).sum(axis=0), rtol=1e-12)
    np.testing.assert_array_equal(shift2, st["mean"].astype(np.float32))
    np.testing.assert_allclose(scale2, 1 / np.sqrt(allx.var(axis=0) + 1e-8), rtol=1e-6)


def test_a_constant_column_gets_scale_zero():
    rng = np.random.default_rng(1)
    n_in = 4
    x = rng.normal(size=(16, 256, n_in)).astype(np.float32)
    x[:, :, 1] = np.float32(9.8)   # exactly constant
    x[:, :, 3] = np.float32(1e-9) * rng.normal(size=(16, 256)).astype(np.float32)  # below min_std
    steps = np.full(256, 16)
    for shift in (np.zeros(n_in, np.float32), np.array([0.1, 9.5, -1, 0], np.float32)):
        s1, s2, _ = SR.input_sums(x, steps, shift)
        partial = np.zeros((1, 2, SR.MAX_IN))
        partial[0, 0, :n_in], partial[0, 1, :n_in] = s1, s2
        st, sh, sc = SR.merge(SR.fresh(n_in), partial, int(steps.sum()), shift)
        assert sc[1] == 0 and sc[3] == 0 and sc[0] > 0 and sc[2] > 0
        assert sh[1] == np.float32(9.8)
    # the relative term: a spread of 2^-19 of the mean is rounding, one of 2^-16 is not
    big = {"count": 1000, "mean": np.array([1e6, 1e6]), "m2": 1000 * np.array([(1e6 * 2.0 ** -19) ** 2, (1e6 * 2.0 ** -16) ** 2])}
    sh, sc = SR.transform(big)
    assert sc[0] == 0 and sc[1] > 0


def test_an_empty_launch_changes_nothing():
    st = {"count": 7, "mean": np.array([1.0, 2.0]), "m2": np.array([3.0, 4.0])}
    new, sh, sc = SR.merge(st, np.full((2, 2, SR.MAX_IN), np.nan), 0, np.zeros(2, np.float32))
    assert new is st and sh is None and sc is None
    new, sh, sc = SR.merge(SR.fresh(2), np.zeros((0, 2, SR.MAX_IN)), 0, np.zeros(2, np.float32))
    assert new["count"] == 0 and sh is None


def test_the_reference_merge_stays_inside_the_exact_bound(capsys):
    """SR.merge (the header's operations in float64) against the pooled mean and M2 of integer data in exact rational
    arithmetic, over one to three successive merges of up to 257 slabs: inside the bound derived from the operation list
    (test_gpu_policy_stats_merge.py's docstring; SR.exact_merge) on every case.  The exact recursion itself is checked
    against the plain sums of everything merged."""
    worst = [0.0, 0.0]
    cases = SR.exact_cases()
    assert len(cases) == 120
    for n_in, launches, (tot_n, tot_x, tot_xx) in cases:
        st, ex = SR.fresh(n_in), SR.exact_fresh(n_in)
        for partial, steps, shift in launches:
            assert np.isnan(partial[:, :, n_in:]).all()
            n_b = int(steps.astype(np.int64).sum())
            st, _, _ = SR.merge(st, partial, n_b, shift)
            ex = SR.exact_merge(ex, partial, n_b, shift)
            r = SR.exact_ratio(ex, st["mean"], st["m2"])
            assert max(r) <= 1.0, (n_in, r)
            worst = [max(a, b) for a, b in zip(worst, r)]
            assert st["count"] == ex["count"] and np.all(st["m2"] >= 0)
        assert ex["count"] == tot_n
        for i in range(n_in):
            assert ex["mean"][i] == SR.Fraction(tot_x[i], tot_n)
            assert ex["m2"][i] == tot_xx[i] - SR.Fraction(tot_x[i] * tot_x[i], tot_n)
    with capsys.disabled():
        print(f"\nstats_ref.merge against exact arithmetic: worst |err| / bound {worst[0]:.3f} (mean), {worst[1]:.3f} (M2)")
    assert min(worst) > 0.01  # (the bound is of the error's order: a bound a hundred times too wide would check little)


@pytest.mark.parametrize("widths", [()] + HIDDEN_SHAPES, ids=str)
@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.PENDULUM])
def test_offsets_agree_with_the_packing(family, widths):
    eng = fake_engine(family)
    n_out = int(eng.info.n_actions) if eng.info.action_is_discrete else 1
    n_in = eng.F + eng.D
    rng = np.random.default_rng(3)
    shift, scale = rng.normal(size=n_in).astype(np.float32), rng.uniform(1, 2, n_in).astype(np.float32)
    pol = MLPPolicy.for_env(eng, rand_layers(rng, [n_in, *widths, n_out]), "tanh", input_shift=shift, input_scale=scale,
                            input_clip=5.0)
    p_shift, p_scale, p_clip, set_floats = SR.transform_offsets(n_in, widths, n_out)
    assert p_shift == pol.weight_floats and set_floats == pol.set_floats
    flat = pol.params[0]
    np.testing.assert_array_equal(flat[p_shift:p_scale], shift)
    np.testing.assert_array_equal(flat[p_scale:p_clip], scale)
    assert flat[p_clip] == np.float32(5.0) and not flat[p_clip + 1:].any()
    np.testing.assert_array_equal(pol.transform_section()[0], flat[p_shift:p_clip + 1])


def test_input_stats_host_rules():
    eng = fake_engine(_lib.CARTPOLE)
    pol = MLPPolicy.for_env(eng, rand_layers(np.random.default_rng(0), [eng.F + eng.D, 2]), "tanh")
    with pytest.raises(TypeError, match="MLPPolicy"):
        InputStats(object(), "cpu")
    with pytest.raises(ValueError, match="finite and >= 0"):
        InputStats(pol, "cpu", eps=-1.0)
    with pytest.raises(ValueError, match="finite and >= 0"):
        InputStats(pol, "cpu", min_std=float("inf"))
    st = InputStats(pol, "cpu")  # (the running state is three plain tensors: a CPU device holds them, nothing launches)
    assert int(st.count) == 0 and st.mean.shape == (pol.n_in,) and st.var.shape == (pol.n_in,)
    with pytest.raises(ValueError, match="nothing merged"):
        st.apply_to(pol)
    with pytest.raises(ValueError, match="input_partial"):
        st.update({"steps": None})
    # state_dict round trip, and apply_to against the reference's transform
    rng = np.random.default_rng(2)
    ref = {"count": 1234, "mean": rng.normal(size=pol.n_in), "m2": 1234 * rng.uniform(0.5, 2, pol.n_in)}
    ref["m2"][2] = 0.0
    st.load_state_dict(ref)
    back = st.state_dict()
    assert int(back["count"]) == 1234
    np.testing.assert_array_equal(back["mean"].numpy(), ref["mean"])
    np.testing.assert_array_equal(back["m2"].numpy(), ref["m2"])
    np.testing.assert_allclose(st.var.numpy(), ref["m2"] / 1234, rtol=1e-15)
    shift, scale = SR.transform(ref)
    new = st.apply_to(pol)
    np.testing.assert_array_equal(new.shift, shift)
    np.testing.assert_array_equal(new.scale, scale)
    assert new.scale[2] == 0 and new.clip == pol.clip
    off = pol.weight_floats
    np.testing.assert_array_equal(new.params[0, :off].view(np.uint32), pol.params[0, :off].view(np.uint32))
