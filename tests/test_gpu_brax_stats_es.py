"""Normalised evolution strategies (ARS V2) over the Brax families on the GPU: EvolutionStrategy with a BraxMLPPolicy template
and input_stats=InputStats(template, device).  Two generations, re-derived on the host as tests/test_gpu_brax_es.py re-derives
the unnormalised ones (es_ref), plus what the statistics add: the centre's transform after a generation is the host merge
(stats_ref.merge) of that generation's slabs, the next generation's members all carry it, and its evaluation is
evaluate_episodes of the same population on a second engine from the same reset, bit for bit.  No host synchronisation
inside a step."""
import ctypes as C

import numpy as np
import pytest
import torch

import brax_episodes_cases as BE
import es_ref as ER
import stats_ref as SR
from carl_amd import _lib
from carl_amd import es as ES
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import InputStats

pytestmark = pytest.mark.gpu

SEED = 0xFEEDFACE00000007
TIME_LIMIT, MAX_STEPS, L, K = 8, 20, 256, 1
# model, lanes per env, envs, population, hidden widths, activation
CASES = [("inverted_pendulum", 2, 1024, 4, (8,), "tanh"), ("ant", 9, 512, 2, (16,), "relu")]


def bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


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


@pytest.mark.parametrize("model,width,n,P,widths,act", CASES, ids=[c[0] for c in CASES])
def test_two_normalised_generations_rederived_on_the_host(device, model, width, n, P, widths, act):
    sigma, lr, rtol = 0.1, 0.05, 1e-12
    eng, eng2 = engine(model, width, n, device), engine(model, width, n, device)
    tmpl = BE.make_policy(eng, widths, act, 72)
    stats = InputStats(tmpl, device)
    es = ES.EvolutionStrategy(eng, tmpl, lanes_per_set=L, sigma=sigma, lr=lr, seed=SEED, input_stats=stats)
    assert es.input_stats is stats and es.n_sets == P
    S, N, n_in = tmpl.set_floats, tmpl.weight_floats, tmpl.n_in
    sl = int(_lib.load().carl_es_slice_pairs())
    ref = SR.fresh(n_in)
    sections = []
    for g in range(2):
        before = es.center.cpu().numpy().copy()
        want_params, z = noise_of(es.struct(), es.center, device)
        info = es.step(n_episodes=K, max_steps=MAX_STEPS)
        assert es.generation == g + 1
        host = want_params.cpu().numpy()
        assert torch.equal(bits(es.population.device_params(device)), bits(want_params))
        np.testing.assert_array_equal(host.view(np.uint32), ER.perturb_ref(before, z, sigma).view(np.uint32))
        # every member carries the centre's transform section as it was before this step: carl_es_perturb copies it
        for k in range(P):
            np.testing.assert_array_equal(host[k, N:].view(np.uint32), before[N:].view(np.uint32))
        if g == 1:
            np.testing.assert_array_equal(before[N: N + 2 * n_in].view(np.uint32), sections[0].view(np.uint32))
        # the evaluation, independently: the members unpacked and stacked on the host, on the second engine
        stacked = BraxMLPPolicy.stack([BraxMLPPolicy.unpack(tmpl, host[s]) for s in range(P)], L)
        eng2.reset()
        want = eng2.evaluate_episodes(stacked, K, MAX_STEPS, input_stats=True)
        assert sorted(info["result"]) == sorted(want) and "input_partial" in want
        for k in want:
            assert torch.equal(bits(info["result"][k]), bits(want[k])), k
        assert int(want["episodes"].min()) == K
        fit = ES.set_fitness(want, P).cpu()
        assert torch.equal(bits(info["fitness"]), bits(fit)) and bool(torch.isfinite(fit).all())
        w = ER.centered_rank_weights(fit.numpy())
        np.testing.assert_array_equal(info["weight"].cpu().numpy().view(np.uint32), w.view(np.uint32))
        grad = ER.gradient_ref(w, z, sl)
        np.testing.assert_array_equal(info["grad"].cpu().numpy().view(np.uint32), grad.view(np.uint32))
        after = es.center.cpu().numpy()
        moved = before[:N] + np.float32(lr / (P * sigma)) * grad
        np.testing.assert_array_equal(after[:N].view(np.uint32), moved.astype(np.float32).view(np.uint32))
        # the statistics: the host merge of this generation's slabs under the shift it ran under
        res = info["result"]
        n_b = int(res["steps"].sum())
        ref, sh, sc = SR.merge(ref, res["input_partial"].cpu().numpy(), n_b, before[N: N + n_in])
        assert int(stats.count) == ref["count"] and n_b > 0
        np.testing.assert_allclose(stats.mean.cpu().numpy(), ref["mean"], rtol=rtol, atol=0)
        ok = SR.settled(ref, stats.eps, stats.min_std, 4 * rtol)
        assert ok.sum() >= n_in - 2, ok
        sec = after[N: N + 2 * n_in]
        np.testing.assert_array_equal(sec[:n_in][ok].view(np.uint32), sh[ok].view(np.uint32))
        np.testing.assert_array_equal(sec[n_in:][ok].view(np.uint32), sc[ok].view(np.uint32))
        np.testing.assert_array_equal(after[N + 2 * n_in:].view(np.uint32), before[N + 2 * n_in:].view(np.uint32))  # clip, padding
        sections.append(sec.copy())
    assert not np.array_equal(sections[0], sections[1])
    # a run resumed from a checkpoint's statistics starts from them
    resumed = InputStats(tmpl, device)
    resumed.load_state_dict(stats.state_dict())
    es2 = ES.EvolutionStrategy(eng2, tmpl, lanes_per_set=L, sigma=sigma, lr=lr, seed=SEED, input_stats=resumed)
    es2.step(n_episodes=K, max_steps=MAX_STEPS)
    assert int(resumed.count) > int(ref["count"])


def test_a_normalised_step_does_not_synchronise_with_the_host(device):
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
    eng = engine("inverted_pendulum", 2, 1024, device)
    tmpl = BE.make_policy(eng, (8,), "tanh", 73)
    es = ES.EvolutionStrategy(eng, tmpl, lanes_per_set=L, seed=SEED, input_stats=InputStats(tmpl, device))
    es.step(n_episodes=1, max_steps=MAX_STEPS)  # warm-up: first uploads, code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        info = es.step(n_episodes=2, max_steps=MAX_STEPS)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert es.generation == 2 and "input_partial" in info["result"] and int(es.input_stats.count) > 0
