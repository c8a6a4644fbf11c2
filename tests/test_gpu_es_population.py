"""The population path on the GPU: a perturbed block used through MLPPolicy.on_device gives the bits a host stack() of
the same floats gives; EvolutionStrategy.step re-derived on the host from what it returns (fitness, shaping, gradient,
centre), generation by generation, at 4 sets and at 258 (with and without input statistics); set_fitness and the two
shaping rules on device tensors against float64 NumPy and es_ref; no host synchronisation inside a step; the
constructor's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import es_ref as ER
import stats_ref as SR
from carl_amd import _lib
from carl_amd import es as ES
from carl_amd.policy import MLPPolicy
from policy_cases import make_engine, make_policy, n_outputs
from policy_checks import assert_same_state, engine_state

pytestmark = pytest.mark.gpu

SEED = 0xFEEDFACE00000005


def bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def assert_same_dict(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def noise_of(es_struct, center, device):
    """the noise of a generation, from a carl_es_perturb call of its own with the same struct -> (params, noise) NumPy"""
    params = torch.empty((2 * es_struct.n_pairs, es_struct.set_floats), dtype=torch.float32, device=device)
    noise = torch.empty((es_struct.n_pairs, es_struct.n_noisy), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().carl_es_perturb(C.byref(es_struct), center.data_ptr(), params.data_ptr(), noise.data_ptr(),
                                               torch.cuda.current_stream(device).cuda_stream))
    return params, noise.cpu().numpy()


POPULATIONS = [("cartpole_linear", _lib.CARTPOLE, (), "tanh", 1024, 4, True),
               ("cartpole_33x7_relu", _lib.CARTPOLE, (33, 7), "relu", 1024, 4, True),
               ("pendulum_sampled", _lib.PENDULUM, (33, 7), "relu", 512, 2, False)]


@pytest.mark.parametrize("name,family,widths,act,n,P,deterministic", POPULATIONS, ids=[c[0] for c in POPULATIONS])
def test_device_population_equals_host_stack(device, name, family, widths, act, n, P, deterministic):
    eng = make_engine(family, n, seed=3)
    rng = np.random.default_rng(11)
    box = not eng.info.action_is_discrete
    tmpl = make_policy(eng, widths, act, rng, "all", clip=3.0, log_std=-0.5 if box else None)
    L = n // P
    es = _lib.Es()
    es.seed, es.generation, es.n_pairs, es.set_floats, es.n_noisy, es.sigma = SEED, 2, P // 2, tmpl.set_floats, tmpl.weight_floats, 0.1
    center = torch.from_numpy(tmpl.params[0]).to(device)
    params, _ = noise_of(es, center, device)
    host = params.cpu().numpy()
    assert not np.array_equal(host[0], host[1])
    log_stds = [-0.5 + 0.375 * s for s in range(P)] if box else [None] * P
    sets = [MLPPolicy.unpack(tmpl, host[s], log_std=log_stds[s]) for s in range(P)]
    stacked = MLPPolicy.stack(sets, L)
    np.testing.assert_array_equal(stacked.params.view(np.uint32), host.view(np.uint32))
    ls_dev = torch.tensor(log_stds, dtype=torch.float32, device=device) if box else None
    dev = MLPPolicy.on_device(tmpl, params, L, log_std=ls_dev)
    assert dev.n_sets == P and dev.device_params(eng.device) is params and dev.set_floats == tmpl.set_floats
    assert dev.struct(n).n_sets == P and dev.struct(n).lanes_per_set == L
    np.testing.assert_array_equal(dev.transform_section().view(np.uint32), stacked.transform_section().view(np.uint32))
    if box:
        assert dev.device_log_std(eng.device) is ls_dev
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="live on"):
            dev.device_params(torch.device("cuda", 1))
    with pytest.raises(ValueError, match="live on"):
        dev.device_params("cpu")
    snap = eng.snapshot()
    kw = dict(deterministic=deterministic, sample_seed=9)
    got = eng.evaluate_policy(dev, 2, 200, **kw)
    state = engine_state(eng)
    eng.restore(snap)
    want = eng.evaluate_policy(stacked, 2, 200, **kw)
    assert_same_dict(got, want)
    assert_same_state(state, engine_state(eng))
    assert int(got["episodes"].sum()) > 0
    eng.restore(snap)
    got = eng.rollout_policy(dev, 64, **kw)
    state = engine_state(eng)
    eng.restore(snap)
    want = eng.rollout_policy(stacked, 64, **kw)
    assert_same_dict(got, want)
    assert_same_state(state, engine_state(eng))


def spread_template(eng, seed=0):
    """a linear CartPole policy over every context row whose weights lie in +-[0.5, 1.5]: far enough from 0 that a
    relative comparison of the centre is a comparison of its updates (test_three_generations: the Adam leg)"""
    rng = np.random.default_rng(seed)
    n_in = len(eng.ctx_obs_rows) + eng.D
    W = rng.uniform(0.5, 1.5, (n_outputs(eng), n_in)) * rng.choice([-1.0, 1.0], (n_outputs(eng), n_in))
    b = rng.uniform(0.5, 1.5, n_outputs(eng)) * rng.choice([-1.0, 1.0], n_outputs(eng))
    scale = np.r_[np.zeros(len(eng.ctx_obs_rows)), [10, 2, 10, 2]]
    return MLPPolicy.for_env(eng, [(W, b)], "tanh", input_scale=scale, input_clip=5.0)


def check_generations(device, mode, n, generations, max_steps, every_lane_finishes=True, normalize=False):
    """`generations` steps of EvolutionStrategy over n CartPole lanes in sets of 256, each re-derived on the host: the
    members from the centre (perturb_ref), the fitness from the returned records, the weights, the gradient
    (gradient_ref) and the centre's update bit for bit; normalize: with input statistics, the centre's transform section
    against stats_ref.merge of the returned slabs.  every_lane_finishes: max_steps leaves every lane a finished episode
    (else: every set, and the lanes without one are left out of the fitness)"""
    L, sigma, lr = 256, 0.1, 0.05
    eng = make_engine(_lib.CARTPOLE, n, seed=1)
    tmpl = spread_template(eng)
    P, S, N = n // L, tmpl.set_floats, tmpl.weight_floats
    assert N == 2 * 12 + 2
    if mode == "adam":
        es = ES.EvolutionStrategy(eng, tmpl, lanes_per_set=L, sigma=sigma, seed=SEED,
                                  optimizer=lambda p: torch.optim.Adam([p], lr=0.01))
        cpu_param = torch.from_numpy(tmpl.params[0, :N].copy())
        cpu_opt = torch.optim.Adam([cpu_param], lr=0.01)
    else:
        es = ES.EvolutionStrategy(eng, tmpl, lanes_per_set=L, sigma=sigma, lr=lr, seed=SEED, fitness_shaping=mode,
                                  normalize_inputs=normalize)
    n_in, stats = tmpl.n_in, SR.fresh(tmpl.n_in)
    assert es.generation == 0 and es.n_sets == P and tuple(es.center.shape) == (S,)
    np.testing.assert_array_equal(es.center.cpu().numpy().view(np.uint32), tmpl.params[0].view(np.uint32))
    sl = int(_lib.load().carl_es_slice_pairs())
    for g in range(generations):
        before = es.center.cpu().numpy().copy()
        want_params, z = noise_of(es.struct(), es.center, device)
        info = es.step(n_episodes=1, max_steps=max_steps)
        assert es.generation == g + 1
        # the members that ran are the perturbation of the centre the step started from
        assert torch.equal(bits(es.population.device_params(device)), bits(want_params))
        np.testing.assert_array_equal(want_params.cpu().numpy().view(np.uint32), ER.perturb_ref(before, z, sigma).view(np.uint32))
        # fitness: the same torch ops on the CPU over the returned episode records
        res = {k: v.cpu() for k, v in info["result"].items()}
        fit = ES.set_fitness(res, P)
        assert torch.equal(bits(info["fitness"]), bits(fit))
        if every_lane_finishes:
            assert int(res["episodes"].min()) == 1  # (CartPole ends within 500 steps: every lane finished its episode)
            by_hand = res["return"][0].double().view(P, L).mean(dim=1)
            np.testing.assert_allclose(fit.double().numpy(), by_hand.numpy(), rtol=1e-6)
        else:  # the horizon is cut: every set still has a finished episode, and only those lanes count
            assert bool((res["episodes"].view(P, L) > 0).any(dim=1).all())
            by_hand, _ = fitness64(res["return"].numpy(), res["episodes"].numpy(), P)
            np.testing.assert_array_equal(fit.numpy(), by_hand.astype(np.float32))  # (integer returns, K = 1: exact)
        w = ER.difference_weights(fit.numpy()) if mode == "difference" else ER.centered_rank_weights(fit.numpy())
        np.testing.assert_array_equal(info["weight"].cpu().numpy().view(np.uint32), w.view(np.uint32))
        grad = ER.gradient_ref(w, z, sl)
        np.testing.assert_array_equal(info["grad"].cpu().numpy().view(np.uint32), grad.view(np.uint32))
        after = es.center.cpu().numpy()
        if normalize:  # the statistics of this generation, merged after the centre moved: shift | scale, nothing else
            ran = res["input_partial"].numpy()
            assert ran.shape[0] == P  # one slab per set of 256 lanes
            stats, sh, sc = SR.merge(stats, ran, int(res["steps"].sum()), before[N: N + n_in])
            np.testing.assert_array_equal(after[N: N + n_in].view(np.uint32), sh.view(np.uint32))
            np.testing.assert_array_equal(after[N + n_in: N + 2 * n_in].view(np.uint32), sc.view(np.uint32))
            np.testing.assert_array_equal(after[N + 2 * n_in:].view(np.uint32), before[N + 2 * n_in:].view(np.uint32))
            assert int(es.input_stats.count) == stats["count"] and np.any(sc > 0)
        else:
            np.testing.assert_array_equal(after[N:].view(np.uint32), before[N:].view(np.uint32))
        if mode == "adam":
            cpu_param.grad = torch.from_numpy(grad) * (-1.0 / (P * sigma))
            cpu_opt.step()
            np.testing.assert_allclose(after[:N], cpu_param.numpy(), rtol=1e-6, atol=0)
            assert np.abs(after[:N]).min() > 0.4
        else:
            want = before[:N] + np.float32(lr / (P * sigma)) * grad
            np.testing.assert_array_equal(after[:N].view(np.uint32), want.astype(np.float32).view(np.uint32))
        assert not np.array_equal(after[:N], before[:N])
    return es, tmpl


@pytest.mark.parametrize("mode", ["centered_rank", "difference", "adam"])
def test_three_generations_rederived_on_the_host(device, mode):
    es, tmpl = check_generations(device, mode, n=1024, generations=3, max_steps=500)
    pol = es.policy()
    assert pol.n_sets == 1 and pol.head == "policy"
    np.testing.assert_array_equal(pol.params[0].view(np.uint32), es.center.cpu().numpy().view(np.uint32))
    new = torch.from_numpy(tmpl.params[0])
    es.center = new  # the caller may replace the centre between steps
    np.testing.assert_array_equal(es.center.cpu().numpy().view(np.uint32), tmpl.params[0].view(np.uint32))


# 258 sets are 129 pairs: one more than a round of es_gradient_kernel's slice loop (es_kernels.hip.h: 8 slices of
# carl_es_slice_pairs() = 16 pairs), 258 slabs for the statistics' merge, 258 weight sets for the episodes kernel.  A
# CartPole episode under these policies ends within a few tens of steps; the horizon is cut to that.
MANY_SETS, CUT_STEPS = 258, 12


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
def test_two_generations_of_258_sets(device, normalize):
    check_generations(device, "centered_rank", n=MANY_SETS * 256, generations=2, max_steps=CUT_STEPS,
                      every_lane_finishes=False, normalize=normalize)


# ---------------------------------------------------------------- fitness and shaping on the device
def fitness64(ret, ep, P):
    """set_fitness's rule in float64 NumPy from ret [K, n] and ep [n]: the mean over a set's lanes with ep > 0 of the
    lane's mean over its first ep returns, -inf for a set without such a lane -> (fitness [P], the same mean of the
    lanes' sum |return| / ep: the scale of the fp32 error bound)"""
    K, n = ret.shape
    valid = np.arange(K)[:, None] < ep[None, :]
    r = np.where(valid, ret.astype(np.float64), 0.0)  # (the rows beyond ep are never read as numbers)
    has = (ep > 0).reshape(P, -1)
    div = np.maximum(ep, 1).astype(np.float64)
    lane = np.where(has, (r.sum(axis=0) / div).reshape(P, -1), 0.0)
    lane_abs = np.where(has, (np.abs(r).sum(axis=0) / div).reshape(P, -1), 0.0)
    count = has.sum(axis=1)
    fit = np.where(count > 0, lane.sum(axis=1) / np.maximum(count, 1), -np.inf)
    return fit, lane_abs.sum(axis=1) / np.maximum(count, 1)


def fitness_bound(K, L):
    """|fp32 set_fitness - float64| <= fitness_bound * (fitness64's scale).  A return reaches its set's fitness through
    at most K - 1 additions over the episode rows, one division by the lane's episode count, L - 1 additions over the
    set's lanes -- in whatever order the device sums them: every term goes through at most that many -- and one
    division by the lane count: m = K + L roundings of relative size u = 2^-24 each, so the term comes out times
    (1 + theta) with |theta| <= gamma_m = m u / (1 - m u) (Higham, Accuracy and Stability, lemma 3.1), and the whole sum
    is off by at most gamma_m times the sum of the terms' magnitudes.  The masks, the counts and the conversions are
    exact.  The float64 reference obeys the same bound with u = 2^-53, added."""
    m = K + L
    return sum(m * u / (1 - m * u) for u in (2.0 ** -24, 2.0 ** -53))


def synthetic_result(P, L, K, rng, integer):
    """episode records [K, P * L] as evaluate_policy leaves them -- NaN in the rows at and beyond a lane's episode count
    -- with episode counts in 0 .. K, set 1 without a finished episode and set 2 with one contributing lane"""
    ep = rng.integers(0, K + 1, (P, L))
    ep[1] = 0
    ep[2] = 0
    ep[2, 77] = K
    ep = ep.reshape(-1).astype(np.int32)
    ret = rng.integers(-500, 501, (K, P * L)).astype(np.float32)
    if not integer:
        ret = (ret + rng.normal(size=ret.shape) * 10).astype(np.float32)
    ret[np.arange(K)[:, None] >= ep[None, :]] = np.nan
    return ret, ep


@pytest.mark.parametrize("P", [4, 258])
@pytest.mark.parametrize("K, integer", [(1, True), (3, True), (3, False)], ids=["K1-integer", "K3-integer", "K3"])
def test_set_fitness_on_the_device(device, K, integer, P):
    L = 256
    ret, ep = synthetic_result(P, L, K, np.random.default_rng(100 * P + K), integer)
    assert np.isnan(ret).any() and ep.min() == 0 and ep.max() == K
    res = {"return": torch.from_numpy(ret).to(device), "episodes": torch.from_numpy(ep).to(device)}
    got = ES.set_fitness(res, P)
    assert got.device == res["return"].device and got.dtype == torch.float32 and tuple(got.shape) == (P,)
    got = got.cpu().numpy()
    want, scale = fitness64(ret, ep, P)
    assert not np.isnan(got).any()  # the unused rows' NaN reached no fitness
    assert got[1] == -np.inf and np.isinf(got).sum() == 1
    if K == 1:
        assert got[2] == ret[0, 256 * 2 + 77]  # the single contributing lane's only return, as it is
    fin = np.isfinite(want)
    if K == 1 and integer:  # sums of at most 256 integers below 2^9 are exact, and one division of two such integers
        # rounds the same through float64 (53 >= 2 * 24 + 2 bits)
        np.testing.assert_array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    err = np.abs(got[fin].astype(np.float64) - want[fin])
    bound = fitness_bound(K, L) * scale[fin]
    print(f"set_fitness P = {P}, K = {K}: worst |err| / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


def fitness_vectors(P, rng):
    distinct = (rng.permutation(P) * 0.37 - 11).astype(np.float32)
    assert np.unique(distinct).size == P
    five = rng.choice(np.array([-3, 0, 0.5, 7, 7.25], np.float32), P)
    some_inf = distinct.copy()
    some_inf[rng.permutation(P)[: max(1, P // 3)]] = -np.inf  # sets without a finished episode
    some_nan = five.copy()
    some_nan[rng.permutation(P)[: max(1, P // 50)]] = np.nan
    mixed = some_inf.copy()
    mixed[rng.permutation(P)[: max(1, P // 50)]] = np.nan
    return {"distinct": distinct, "five_values": five, "all_equal": np.full(P, 2.5, np.float32), "minus_inf": some_inf,
            "nan": some_nan, "nan_and_minus_inf": mixed}


@pytest.mark.parametrize("P", [2, 4, 258, 4096])
def test_shaping_on_the_device(device, P):
    """centered_rank_weights (two stable device sorts) and difference_weights on device tensors against es_ref, bit for
    bit, every entry compared; where the reference has a NaN (-inf minus -inf, or a NaN fitness, in the difference) the
    device must have one at the same index"""
    rng = np.random.default_rng(P)
    for name, f in fitness_vectors(P, rng).items():
        t = torch.from_numpy(f).to(device)
        got = ES.centered_rank_weights(t)
        assert got.device == t.device and got.is_contiguous()
        want = ER.centered_rank_weights(f)
        assert np.isfinite(want).all() and want.shape == (P // 2,)
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=name)
        got, want = ES.difference_weights(t).cpu().numpy(), ER.difference_weights(f)
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=name)
        np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=name)
        assert torch.equal(bits(t), bits(torch.from_numpy(f)))  # (the input is left as it was)


def test_step_does_not_synchronise_with_the_host(device):
    from carl_amd.context.selection import StaticSelector
    from carl_amd.envs import CARLCartPole

    n, L = 1024, 256
    probe = torch.zeros(1, device=device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            supported = False
        except RuntimeError:
            supported = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not supported:
        pytest.skip("this torch build does not report synchronising calls under set_sync_debug_mode('error') on ROCm")
    for kind in ("engine", "env"):
        if kind == "engine":
            env = make_engine(_lib.CARTPOLE, n, seed=2)
        else:
            env = CARLCartPole(num_envs=n, device="cuda:0", context_selector=StaticSelector, seed=0)
            env.reset(seed=0)
        es = ES.EvolutionStrategy(env, spread_template(env.env if kind == "env" else env), lanes_per_set=L, seed=SEED)
        es.step(n_episodes=1, max_steps=500)  # warm-up: first uploads, code objects
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            info = es.step(n_episodes=1, max_steps=500)
            es.step(n_episodes=2, max_steps=100, deterministic=False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert es.generation == 3 and bool(torch.isfinite(info["fitness"]).all())


def test_constructor_refusals(device):
    from carl_amd.envs import CARLBraxAnt

    eng = make_engine(_lib.CARTPOLE, 1024)
    tmpl = spread_template(eng)
    ES.EvolutionStrategy(eng, tmpl, lanes_per_set=256)
    with pytest.raises(ValueError, match="even and at least 2"):
        ES.EvolutionStrategy(make_engine(_lib.CARTPOLE, 768), tmpl, lanes_per_set=256)  # P = 3
    with pytest.raises(ValueError, match="even and at least 2"):
        ES.EvolutionStrategy(eng, tmpl, lanes_per_set=1024)  # P = 1
    with pytest.raises(ValueError, match="lanes beyond"):
        ES.EvolutionStrategy(make_engine(_lib.CARTPOLE, 1100), tmpl, lanes_per_set=256)
    with pytest.raises(ValueError, match="multiple of"):
        ES.EvolutionStrategy(eng, tmpl, lanes_per_set=100)
    with pytest.raises(ValueError, match="auto_reset"):
        ES.EvolutionStrategy(make_engine(_lib.CARTPOLE, 1024, auto_reset=False), tmpl, lanes_per_set=256)
    with pytest.raises(TypeError, match="classic-control families only"):
        ES.EvolutionStrategy(CARLBraxAnt(batch_size=512, device=device), tmpl, lanes_per_set=256)
    pend = make_engine(_lib.PENDULUM, 1024)
    with pytest.raises(ValueError, match="built for family"):
        ES.EvolutionStrategy(pend, tmpl, lanes_per_set=256)
    with pytest.raises(ValueError, match="one-set"):
        ES.EvolutionStrategy(eng, MLPPolicy.stack([tmpl, tmpl], 256), lanes_per_set=256)
    with pytest.raises(ValueError, match="fitness_shaping"):
        ES.EvolutionStrategy(eng, tmpl, lanes_per_set=256, fitness_shaping="ranks")
    with pytest.raises(ValueError, match="sigma"):
        ES.EvolutionStrategy(eng, tmpl, lanes_per_set=256, sigma=0.0)
