"""carl_es_perturb / carl_es_gradient on the GPU against the host reference written from the header (es_ref.py): the noise
within the project's bound for the device's Gaussian expression of the float64 z, everything after the noise bit for
bit -- the perturbation (two roundings, antithetic, the tail's bits), the gradient in the header's summation order --
canaries behind every output, and the stream's dependence on seed, generation and pair.  Pair counts up to two slices
and a bit, and then across the rounds of the gradient kernel's slice loop (one round: 8 slices), at parameter counts
around a workgroup's 64; an entry of the gradient does not depend on how many parameters the launch has."""
import ctypes as C

import numpy as np
import pytest
import torch

import es_ref as ER
import sampling_ref as SR
from carl_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567890  # (a high word: both key halves are live)
CANARY = 64
N_NOISY = [1, 2, 3, 26, 4417]  # 26: CartPole linear over 12 inputs; 4 417: several waves, the last Philox block half-used


def slice_pairs():
    return int(_lib.load().carl_es_slice_pairs())


def set_floats_of(n_noisy, tail):
    """the next multiple of 4 at or above n_noisy + 2 * 12 + 1 (a shift | scale | clip section of 12 inputs), or n_noisy
    rounded up to 4 with no section at all"""
    return (n_noisy + (25 if tail else 0) + 3) // 4 * 4


def es_struct(n_pairs, set_floats, n_noisy, sigma=0.1, generation=0, seed=SEED):
    es = _lib.Es()
    es.seed, es.generation, es.n_pairs, es.set_floats, es.n_noisy, es.sigma = seed, generation, n_pairs, set_floats, n_noisy, sigma
    return es


def center_of(set_floats, n_noisy, rng):
    c = rng.normal(size=set_floats).astype(np.float32)
    tail = c[n_noisy:]
    if tail.size >= 3:  # what a clip slot may hold: its bits must come through untouched
        tail.view(np.uint32)[-3:] = [0x7F800000, 0x7FC01234, 0xFF800000]
    elif tail.size:
        tail.view(np.uint32)[-1] = 0x7FC01234
    return c


def perturb(es, center, device, with_noise=True):
    """one carl_es_perturb launch -> (params, noise or None) as NumPy, after checking the canaries behind both"""
    lib = _lib.load()
    n_par, n_noi = 2 * es.n_pairs * es.set_floats, es.n_pairs * es.n_noisy
    fill = -7.25
    params = torch.full((n_par + CANARY,), fill, dtype=torch.float32, device=device)
    noise = torch.full((n_noi + CANARY,), fill, dtype=torch.float32, device=device) if with_noise else None
    c = torch.from_numpy(center).to(device)
    with torch.cuda.device(device):
        _lib.check(lib.carl_es_perturb(C.byref(es), c.data_ptr(), params.data_ptr(),
                                       noise.data_ptr() if with_noise else None,
                                       torch.cuda.current_stream(device).cuda_stream))
    p = params.cpu().numpy()
    assert (p[n_par:] == fill).all(), "carl_es_perturb wrote behind params"
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), center.view(np.uint32))
    z = None
    if with_noise:
        z = noise.cpu().numpy()
        assert (z[n_noi:] == fill).all(), "carl_es_perturb wrote behind noise"
        z = z[:n_noi].reshape(es.n_pairs, es.n_noisy)
    return p[:n_par].reshape(2 * es.n_pairs, es.set_floats), z


def gradient(es, weight, device):
    lib = _lib.load()
    fill = -7.25
    grad = torch.full((es.n_noisy + CANARY,), fill, dtype=torch.float32, device=device)
    w = torch.from_numpy(weight).to(device)
    with torch.cuda.device(device):
        _lib.check(lib.carl_es_gradient(C.byref(es), w.data_ptr(), grad.data_ptr(),
                                        torch.cuda.current_stream(device).cuda_stream))
    g = grad.cpu().numpy()
    assert (g[es.n_noisy:] == fill).all(), "carl_es_gradient wrote behind grad"
    return g[: es.n_noisy]


def pair_counts():
    s = slice_pairs()
    return sorted({1, max(1, s - 1), s, s + 1, 2 * s + 3})


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("tail", [True, False], ids=["section", "no_tail"])
@pytest.mark.parametrize("n_noisy", N_NOISY)
def test_perturb_noise_bound_and_exact_arithmetic(device, n_noisy, tail):
    S = set_floats_of(n_noisy, tail)
    rng = np.random.default_rng(n_noisy)
    for k, n_pairs in enumerate(pair_counts()):
        gen = [0, 7, 2**32 - 1][k % 3]
        es = es_struct(n_pairs, S, n_noisy, sigma=[0.1, 0.02, 1.5][k % 3], generation=gen)
        center = center_of(S, n_noisy, rng)
        params, z = perturb(es, center, device)
        # the noise: the device's fp32 expression of the float64 z, within the project's bound for it
        z64 = ER.z64(SEED, gen, n_pairs, n_noisy)
        err = np.abs(z.astype(np.float64) - z64)
        assert (err <= SR.gaussian_z_bound(z64)).all(), (n_pairs, float((err / SR.gaussian_z_bound(z64)).max()))
        assert np.abs(z).max() <= 5.8
        # everything after the noise is exact
        want = ER.perturb_ref(center, z, es.sigma)
        np.testing.assert_array_equal(bits(params), bits(want))
        np.testing.assert_array_equal(bits(params[:, n_noisy:]), np.tile(bits(center[n_noisy:]), (2 * n_pairs, 1)))
        d = (np.float32(es.sigma) * z).astype(np.float32)
        np.testing.assert_array_equal(bits(params[0::2, :n_noisy]), bits(center[:n_noisy] + d))
        np.testing.assert_array_equal(bits(params[1::2, :n_noisy]), bits(center[:n_noisy] - d))
        # noise = NULL changes nothing; a second launch gives the same bits
        again, none = perturb(es, center, device, with_noise=False)
        assert none is None
        np.testing.assert_array_equal(bits(again), bits(params))


@pytest.mark.parametrize("n_noisy", N_NOISY)
def test_gradient_is_the_header_sum(device, n_noisy):
    S = set_floats_of(n_noisy, True)
    sl = slice_pairs()
    rng = np.random.default_rng(100 + n_noisy)
    for k, n_pairs in enumerate(pair_counts()):
        es = es_struct(n_pairs, S, n_noisy, generation=[0, 7, 2**32 - 1][k % 3])
        _, z = perturb(es, center_of(S, n_noisy, rng), device)
        weights = [rng.normal(size=n_pairs).astype(np.float32)]
        w = rng.normal(size=n_pairs).astype(np.float32)
        w[rng.random(n_pairs) < 0.4] = 0.0
        w[::3] = -np.abs(w[::3])
        weights.append(w)
        w = rng.normal(size=n_pairs).astype(np.float32)
        w[n_pairs // 2] = np.inf
        weights.append(w)
        for w in weights:
            got = gradient(es, w, device)
            want = ER.gradient_ref(w, z, sl)
            np.testing.assert_array_equal(bits(got), bits(want))


# ---------------------------------------------------------------- past one round of the gradient's slice loop
# es_kernels.hip.h: a workgroup of es_gradient_kernel sums kEsGradSlices = 8 slices side by side, so one trip of its s0
# loop covers 8 * carl_es_slice_pairs() pairs; beyond that it goes round again and carries `total` across the trips.
GRAD_SLICES = 8  # kEsGradSlices (not exported)
ROUND_COUNTS = {"R-1": lambda R, s: R - 1, "R": lambda R, s: R, "R+1": lambda R, s: R + 1,  # the round boundary
                "R+s+3": lambda R, s: R + s + 3,   # a second round of two slices, the last one ragged
                "2R": lambda R, s: 2 * R,          # exactly two full rounds
                "2R+1": lambda R, s: 2 * R + 1}    # a third round of one slice holding one pair
# a workgroup owns 64 parameters: below, at and above one workgroup, and three of them with one parameter in the last
ROUND_N_NOISY = [26, 63, 64, 65, 129]
ROUND_CASES = [(n, c) for n in ROUND_N_NOISY for c in ROUND_COUNTS] + [(4417, "R+s+3")]


def round_pairs(count):
    s = slice_pairs()
    return ROUND_COUNTS[count](GRAD_SLICES * s, s), GRAD_SLICES * s


def round_weights(n_pairs, R, rng):
    """the three weight vectors of test_gradient_is_the_header_sum, one with its inf in a pair of the second round (the
    last pair where there is no second round), and one with an inf in each of the first two rounds: wherever the two z
    have opposite signs the total is inf - inf"""
    weights = [rng.normal(size=n_pairs).astype(np.float32)]
    w = rng.normal(size=n_pairs).astype(np.float32)
    w[rng.random(n_pairs) < 0.4] = 0.0
    w[::3] = -np.abs(w[::3])
    weights.append(w)
    w = rng.normal(size=n_pairs).astype(np.float32)
    w[n_pairs // 2] = np.inf
    weights.append(w)
    second = R + (n_pairs - R) // 2 if n_pairs > R else n_pairs - 1
    w = rng.normal(size=n_pairs).astype(np.float32)
    w[second] = np.inf
    weights.append(w)
    w = rng.normal(size=n_pairs).astype(np.float32)
    w[3], w[second] = np.inf, np.inf
    weights.append(w)
    return weights, second


def assert_same_floats(got, want):
    """bit for bit; a NaN must be a NaN at the same index (its sign and payload are the adder's, not the header's)"""
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("n_noisy, count", ROUND_CASES, ids=[f"{n}-{c}" for n, c in ROUND_CASES])
def test_rounds_of_the_gradient_loop(device, n_noisy, count):
    n_pairs, R = round_pairs(count)
    k = list(ROUND_COUNTS).index(count)
    S = set_floats_of(n_noisy, True)
    rng = np.random.default_rng(1000 * n_noisy + k)
    gen = [0, 7, 2**32 - 1][k % 3]
    es = es_struct(n_pairs, S, n_noisy, sigma=[0.1, 0.02, 1.5][k % 3], generation=gen)
    center = center_of(S, n_noisy, rng)
    params, z = perturb(es, center, device)
    if n_noisy == 26:  # (the host Philox dominates the cost: the noise bound at one width only)
        z64 = ER.z64(SEED, gen, n_pairs, n_noisy)
        err = np.abs(z.astype(np.float64) - z64)
        assert (err <= SR.gaussian_z_bound(z64)).all(), (n_pairs, float((err / SR.gaussian_z_bound(z64)).max()))
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.8
    np.testing.assert_array_equal(bits(params), bits(ER.perturb_ref(center, z, es.sigma)))
    np.testing.assert_array_equal(bits(params[:, n_noisy:]), np.tile(bits(center[n_noisy:]), (2 * n_pairs, 1)))
    weights, second = round_weights(n_pairs, R, rng)
    sl = slice_pairs()
    for i, w in enumerate(weights):
        got = gradient(es, w, device)
        want = ER.gradient_ref(w, z, sl)
        assert_same_floats(got, want)
        if i < 2:
            assert np.isfinite(want).all()
        elif i < 4:  # one inf weight: every entry is +-inf by the sign of that pair's z, none is NaN
            at = n_pairs // 2 if i == 2 else second
            assert np.isinf(want).all() and (np.signbit(want) == np.signbit(z[at])).all()
        elif second != 3 and n_noisy >= 26:  # inf - inf wherever the two pairs' z differ in sign, and only there
            np.testing.assert_array_equal(np.isnan(want), np.signbit(z[3]) != np.signbit(z[second]))
            assert np.isnan(want).any() and not np.isnan(want).all()


@pytest.mark.parametrize("count", ["R+s+3", "2R+1"])
def test_an_entry_does_not_depend_on_the_grid(device, count):
    """the counter holds the parameter index, not the launch's shape: the first 26 entries of a three-workgroup launch
    (n_noisy = 129) are the one-workgroup launch (n_noisy = 26) of the same seed, generation, pairs and weights"""
    n_pairs, R = round_pairs(count)
    S = set_floats_of(129, True)
    rng = np.random.default_rng(77)
    center = center_of(S, 129, rng)
    wide, narrow = es_struct(n_pairs, S, 129, generation=5), es_struct(n_pairs, S, 26, generation=5)
    _, z_wide = perturb(wide, center, device)
    _, z_narrow = perturb(narrow, center, device)
    np.testing.assert_array_equal(bits(z_wide[:, :26]), bits(z_narrow))
    for w in round_weights(n_pairs, R, rng)[0]:
        assert_same_floats(gradient(wide, w, device)[:26], gradient(narrow, w, device))


def test_stream_depends_on_seed_generation_and_pair(device):
    n_noisy, n_pairs = 26, 3
    S = set_floats_of(n_noisy, True)
    center = center_of(S, n_noisy, np.random.default_rng(5))
    _, z = perturb(es_struct(n_pairs, S, n_noisy, generation=7), center, device)
    _, z_same = perturb(es_struct(n_pairs, S, n_noisy, generation=7), center, device)
    np.testing.assert_array_equal(bits(z), bits(z_same))
    _, z_gen = perturb(es_struct(n_pairs, S, n_noisy, generation=8), center, device)
    _, z_lo = perturb(es_struct(n_pairs, S, n_noisy, generation=7, seed=SEED ^ 1), center, device)
    _, z_hi = perturb(es_struct(n_pairs, S, n_noisy, generation=7, seed=SEED ^ (1 << 63)), center, device)
    for other in (z_gen, z_lo, z_hi):
        assert (bits(other) != bits(z)).mean() > 0.99
    assert (bits(z[0]) != bits(z[1])).mean() > 0.99 and (bits(z[1]) != bits(z[2])).mean() > 0.99
    # a pair's noise does not depend on how many pairs the launch has
    _, z_one = perturb(es_struct(1, S, n_noisy, generation=7), center, device)
    np.testing.assert_array_equal(bits(z_one[0]), bits(z[0]))
