"""EvolutionStrategy over the Brax families on the GPU (carl_amd/es.py with a BraxMLPPolicy template): every generation
re-derived on the host as tests/test_gpu_es_population.py's check_generations re-derives the classic one -- the members
from the centre (es_ref.perturb_ref), the evaluation against evaluate_episodes of a host stack of the unpacked members on a
second engine built from the same arguments and taken through the same resets, the fitness, the shaping, the gradient
(es_ref.gradient_ref) and the centre's update, bit for bit; no host synchronisation inside a step; policy() through
BraxMLPPolicy.unpack; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import brax_episodes_cases as BE
import es_ref as ER
from carl_amd import _lib
from carl_amd import es as ES
from carl_amd.brax_policy import BraxMLPPolicy

pytestmark = pytest.mark.gpu

SEED = 0xFEEDFACE00000006
TIME_LIMIT, MAX_STEPS, L = 8, 20, 256
# model, lanes per env, envs, population, hidden widths, activation
CASES = [("inverted_pendulum", 2, 1024, 4, (8,), "tanh"), ("ant", 9, 512, 2, (16,), "relu")]


def bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def noise_of(es_struct, center, device):
    """the noise of a generation, from a carl_es_perturb call of its own with the same struct -> (params, noise NumPy)"""
    params = torch.empty((2 * es_struct.n_pairs, es_struct.set_floats), dtype=torch.float32, device=device)
    noise = torch.empty((es_struct.n_pairs, es_struct.n_noisy), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().carl_es_perturb(C.byref(es_struct), center.data_ptr(), params.data_ptr(), noise.data_ptr(),
                                               torch.cuda.current_stream(device).cuda_stream))
    return params, noise.cpu().numpy()


def engine(model, width, n, device):
    return BE.make_engine(model, width, n, device, 71, max_episode_steps=TIME_LIMIT)


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("model,width,n,P,widths,act", CASES, ids=[c[0] for c in CASES])
def test_two_generations_rederived_on_the_host(device, model, width, n, P, widths, act, K):
    sigma, lr = 0.1, 0.05
    eng, eng2 = engine(model, width, n, device), engine(model, width, n, device)
    tmpl = BE.make_policy(eng, widths, act, 72)
    es = ES.EvolutionStrategy(eng, tmpl, lanes_per_set=L, sigma=sigma, lr=lr, seed=SEED)
    S, N = tmpl.set_floats, tmpl.weight_floats
    assert es.n_sets == P and type(es.population) is BraxMLPPolicy and tuple(es.center.shape) == (S,)
    sl = int(_lib.load().carl_es_slice_pairs())
    for g in range(2):
        before = es.center.cpu().numpy().copy()
        want_params, z = noise_of(es.struct(), es.center, device)
        info = es.step(n_episodes=K, max_steps=MAX_STEPS)
        assert es.generation == g + 1
        assert torch.equal(bits(es.population.device_params(device)), bits(want_params))
        host = want_params.cpu().numpy()
        np.testing.assert_array_equal(host.view(np.uint32), ER.perturb_ref(before, z, sigma).view(np.uint32))
        # the evaluation, independently: the members unpacked and stacked on the host, on the second engine
        stacked = BraxMLPPolicy.stack([BraxMLPPolicy.unpack(tmpl, host[s]) for s in range(P)], L)
        np.testing.assert_array_equal(stacked.params.view(np.uint32), host.view(np.uint32))
        eng2.reset()
        want = eng2.evaluate_episodes(stacked, K, MAX_STEPS)
        assert sorted(info["result"]) == sorted(want)
        for k in want:
            assert torch.equal(bits(info["result"][k]), bits(want[k])), k
        assert int(want["episodes"].min()) == K  # TimeLimit 8: K episodes fit into 20 steps for every env
        assert int(want["steps"].max()) <= K * TIME_LIMIT < MAX_STEPS
        # fitness: set_fitness of the independent result, on the device its tensors live on (the returns are no integers
        # here: a host sum adds them in another order than the device's reduction and may round the last bit differently)
        fit = ES.set_fitness(want, P).cpu()
        assert torch.equal(bits(info["fitness"]), bits(fit)) and bool(torch.isfinite(fit).all())
        w = ER.centered_rank_weights(fit.numpy())
        np.testing.assert_array_equal(info["weight"].cpu().numpy().view(np.uint32), w.view(np.uint32))
        grad = ER.gradient_ref(w, z, sl)
        np.testing.assert_array_equal(info["grad"].cpu().numpy().view(np.uint32), grad.view(np.uint32))
        after = es.center.cpu().numpy()
        np.testing.assert_array_equal(after[N:].view(np.uint32), before[N:].view(np.uint32))
        moved = before[:N] + np.float32(lr / (P * sigma)) * grad
        np.testing.assert_array_equal(after[:N].view(np.uint32), moved.astype(np.float32).view(np.uint32))
        assert not np.array_equal(after[:N], before[:N])
    pol = es.policy()  # the centre through BraxMLPPolicy.unpack
    assert type(pol) is BraxMLPPolicy and pol.n_sets == 1 and pol.lanes_per_set is None
    np.testing.assert_array_equal(pol.params[0].view(np.uint32), es.center.cpu().numpy().view(np.uint32))
    assert [W.shape for W, _ in pol.layers] == [W.shape for W, _ in tmpl.layers]


def test_step_does_not_synchronise_with_the_host(device):
    from carl_amd.envs import CARLBraxInvertedPendulum

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
            env = eng = engine("inverted_pendulum", 2, 1024, device)
        else:
            env = CARLBraxInvertedPendulum(batch_size=1024, obs_context_features=["gravity", "friction"], device=device)
            env.reset(seed=0)
            eng = env.env
        es = ES.EvolutionStrategy(env, BE.make_policy(eng, (8,), "tanh", 73), lanes_per_set=L, seed=SEED)
        es.step(n_episodes=1, max_steps=MAX_STEPS)  # warm-up: first uploads, code objects
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            info = es.step(n_episodes=2, max_steps=MAX_STEPS)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert es.generation == 2 and tuple(info["fitness"].shape) == (4,)


def test_refusals(device):
    from carl_amd.policy import MLPPolicy
    from policy_cases import fake_engine, rand_layers

    eng = engine("inverted_pendulum", 2, 1024, device)
    tmpl = BE.make_policy(eng, (8,), "tanh", 74)
    ES.EvolutionStrategy(eng, tmpl, lanes_per_set=L)
    with pytest.raises(NotImplementedError, match="normalize_inputs"):
        ES.EvolutionStrategy(eng, tmpl, lanes_per_set=L, normalize_inputs=True)
    with pytest.raises(ValueError, match="deterministic=False"):
        ES.EvolutionStrategy(eng, tmpl, lanes_per_set=L).step(1, MAX_STEPS, deterministic=False)
    with pytest.raises(ValueError, match="even and at least 2"):
        ES.EvolutionStrategy(eng, tmpl, lanes_per_set=1024)
    with pytest.raises(ValueError, match="multiple of"):
        ES.EvolutionStrategy(eng, tmpl, lanes_per_set=100)
    with pytest.raises(ValueError, match="lanes beyond"):
        ES.EvolutionStrategy(engine("inverted_pendulum", 2, 1100, device), tmpl, lanes_per_set=L)
    with pytest.raises(ValueError, match="auto_reset"):
        ES.EvolutionStrategy(BE.make_engine("inverted_pendulum", 2, 1024, device, 71, auto_reset=False), tmpl, lanes_per_set=L)
    with pytest.raises(ValueError, match="one-set"):
        ES.EvolutionStrategy(eng, BraxMLPPolicy.stack([tmpl, tmpl], L), lanes_per_set=L)
    ant = engine("ant", 9, 512, device)
    with pytest.raises(ValueError, match="observations and 1 actuators"):
        ES.EvolutionStrategy(ant, tmpl, lanes_per_set=L)
    rng = np.random.default_rng(0)
    with pytest.raises(TypeError, match="not a CARLBraxEnv or BraxVecEngine"):  # a Brax template on a classic engine
        ES.EvolutionStrategy(fake_engine(_lib.CARTPOLE, [0, 3]), tmpl, lanes_per_set=L)
    classic = MLPPolicy.for_env(fake_engine(_lib.CARTPOLE, [0, 3]), rand_layers(rng, [6, 2]))
    with pytest.raises(TypeError, match="classic-control families only"):  # a classic template on a Brax engine: as ever
        ES.EvolutionStrategy(ant, classic, lanes_per_set=L)
    with pytest.raises(NotImplementedError, match="log_std"):
        BraxMLPPolicy.unpack(tmpl, tmpl.params[0], log_std=0.0)
