"""Input statistics inside the episodes launch (VecEngine.evaluate_policy(..., input_stats=True) /
carl_evaluate_policy_stats) and their merge (InputStats / carl_policy_stats_merge) on the GPU, against stats_ref.py.

Shapes: 300 lanes (two workgroups, the last one of 44 lanes: a partial wave), K = 2 episodes, max_steps = 40 (no
multiple of a chunk once lanes freeze), a table of 7 contexts under the static and the round-robin selector.  CartPole
lanes under random weights end episodes at their own pace; the other families' episodes are cut at 17 steps, so their
lanes freeze at step 34, two steps into a chunk, and the waves leave the loop there.

The bound on the sums is derived, not measured: a lane adds in fp32 over at most one chunk of CHUNK steps (8; Acrobot
4), everything after that is float64, so |S - exact| <= (CHUNK + 2) * 2^-24 * sum |terms| (include/carl_amd.h)."""
import numpy as np
import pytest
import torch

import stats_ref as SR
from carl_amd import _lib
from carl_amd.es import EvolutionStrategy
from carl_amd.policy import InputStats, MLPPolicy
from policy_cases import SELECTORS, STEP_TYPES, make_engine, make_policy, n_outputs, rand_layers
from policy_checks import assert_same_state, engine_state, teacher

pytestmark = pytest.mark.gpu

N, K, T, N_CTX = 300, 2, 40, 7
H_SHAPES = {0: ((), "identity"), 32: ((31,), "tanh"), 64: ((33, 7), "relu")}
SEED = 0x51A7


def chunk_of(family):
    return 4 if family == _lib.ACROBOT else 8  # policy_kernels.hip.h: policy_chunk<Fam>()


def engine_for(step_type, selector, seed=0, n=N, n_contexts=N_CTX):
    family, opts = STEP_TYPES[step_type]
    if family != _lib.CARTPOLE:
        opts = dict(opts, max_episode_steps=17)
    return make_engine(family, n, selector=SELECTORS[selector], n_contexts=n_contexts, seed=seed, **opts)


def policy_for(eng, H, seed, identity=False):
    widths, act = H_SHAPES[H]
    box = not eng.info.action_is_discrete
    if identity:
        rng = np.random.default_rng(seed)
        return MLPPolicy.for_env(eng, rand_layers(rng, [eng.F + eng.D, *widths, n_outputs(eng)]), act,
                                 log_std=-0.5 if box else None)
    return make_policy(eng, widths, act, np.random.default_rng(seed), "all", clip=2.0, log_std=-0.5 if box else None)


def same_bits(a, b):
    if a.is_floating_point():
        a, b = a.view(torch.int64 if a.dtype == torch.float64 else torch.int32), b.view(
            torch.int64 if b.dtype == torch.float64 else torch.int32)
    return torch.equal(a, b)


def check_launch(eng, pol, sampled):
    """from one snapshot: evaluate_policy without and with statistics give the same records and state; the statistics
    launch twice gives the same slabs; each workgroup's slab is the reference sum over that workgroup's live lane-steps,
    rebuilt from a transitions launch (the episodes launch is its prefix), within the derived bound"""
    kw = dict(deterministic=False, sample_seed=SEED) if sampled else {}
    snap = eng.snapshot()
    plain = eng.evaluate_policy(pol, K, T, **kw)
    state_plain = engine_state(eng)
    eng.restore(snap)
    res = eng.evaluate_policy(pol, K, T, input_stats=True, **kw)
    for k in plain:
        assert same_bits(plain[k], res[k]), k
    assert_same_state(state_plain, engine_state(eng))
    eng.restore(snap)
    again = eng.evaluate_policy(pol, K, T, input_stats=True, **kw)
    assert same_bits(res["input_partial"], again["input_partial"])
    # the reference
    eng.restore(snap)
    out = eng.rollout_policy(pol, T, **kw)
    x = teacher(eng, pol, snap, out["action"][:T])[0]
    steps = res["steps"].cpu().numpy()
    partial = res["input_partial"].cpu().numpy()
    n_in, q = pol.n_in, 256
    assert partial.shape == ((eng.n + q - 1) // q, 2, SR.MAX_IN)
    assert not partial[:, :, n_in:].any()
    u = (chunk_of(eng.family) + 2) * 2.0 ** -24
    for w in range(partial.shape[0]):
        lanes = slice(q * w, min(eng.n, q * w + q))
        s1, s2, a1 = SR.input_sums(x[:, lanes], steps[lanes], pol.shift)
        e1, e2 = np.abs(partial[w, 0, :n_in] - s1), np.abs(partial[w, 1, :n_in] - s2)
        print(f"wg {w}: max |dS1| / (u sum|d|) = {np.max(e1 / np.maximum(u * a1, 1e-300)):.3f}, "
              f"max |dS2| / (u sum d^2) = {np.max(e2 / np.maximum(u * s2, 1e-300)):.3f}")
        assert np.all(e1 <= u * a1), (w, e1, u * a1)
        assert np.all(e2 <= u * s2), (w, e2, u * s2)
    return res, steps


CASES = [(s, H, smp) for s in STEP_TYPES for H in (0, 32, 64) for smp in (False, True)]


@pytest.mark.parametrize("step_type, H, sampled", CASES,
                         ids=[f"{s}-H{H}-{'sampled' if m else 'mode'}" for s, H, m in CASES])
def test_every_instance_keeps_the_records_and_sums_the_inputs(step_type, H, sampled):
    """all 36 kernel instances, under a transform with non-zero shift, scale != 1 and a clip that binds: d is taken
    before the scale and the clip.  Round-robin selector for the deterministic instances, static for the sampled ones."""
    c = CASES.index((step_type, H, sampled))
    eng = engine_for(step_type, "static" if sampled else "round_robin", seed=c)
    pol = policy_for(eng, H, seed=100 + c)
    assert pol.shift.any() and np.any(pol.scale != 1) and np.isfinite(pol.clip)
    res, steps = check_launch(eng, pol, sampled)
    assert steps.min() < T or eng.family == _lib.CARTPOLE  # lanes froze before max_steps
    assert steps.sum() > 0


@pytest.mark.parametrize("selector", ["static", "round_robin"])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_identity_transform(step_type, selector):
    """shift 0, scale 1, clip inf: d is the raw input"""
    eng = engine_for(step_type, selector, seed=77)
    pol = policy_for(eng, 0, seed=7, identity=True)
    check_launch(eng, pol, sampled=False)


def test_liveness_and_an_empty_launch():
    """n_b == steps.sum(): a policy whose inputs are all 1 after the shift (observation-free: d = ctx - shift with a
    constant context column) makes S1 the count of live lane-steps of each workgroup exactly; max_steps = 0 writes
    all-zero slabs over whatever the buffer held"""
    eng = engine_for("cartpole", "static", seed=5)
    tab = eng.ctx_table.cpu().numpy()
    one = np.float32(1)
    # a feature the table does not vary, whose fp32 value v has an exact v - 1 (so d = v - (v - 1) is exactly 1)
    row = next(r for r in eng.ctx_obs_rows if np.all(tab[r] == tab[r][0]) and tab[r][0] - (tab[r][0] - one) == one)
    layers = rand_layers(np.random.default_rng(1), [1 + eng.D, 2])
    shift = np.concatenate([[tab[row][0] - one], np.zeros(eng.D)]).astype(np.float32)
    pol = MLPPolicy.for_env(eng, layers, "identity", input_shift=shift, context_features=[row])
    snap = eng.snapshot()
    res = eng.evaluate_policy(pol, K, T, input_stats=True)
    steps = res["steps"].cpu().numpy().astype(np.int64)
    partial = res["input_partial"].cpu().numpy()
    assert 0 < steps.min() and steps.min() < steps.max()  # lanes froze at their own steps
    for w, lanes in enumerate((slice(0, 256), slice(256, N))):  # the padding lanes of the last workgroup add nothing
        assert partial[w, 0, 0] == float(one) * steps[lanes].sum()
        assert partial[w, 1, 0] == float(one) * float(one) * steps[lanes].sum()
    eng.restore(snap)
    buf = eng.alloc_policy_episodes(K)
    buf["input_partial"] = torch.full((2, 2, SR.MAX_IN), float("nan"), dtype=torch.float64, device=eng.device)
    res0 = eng.evaluate_policy(pol, K, 0, out=buf, input_stats=True)
    assert res0["input_partial"] is buf["input_partial"] and not bool(res0["input_partial"].any())
    assert int(res0["steps"].sum()) == 0
    with pytest.raises(ValueError, match="input_partial"):
        buf["input_partial"] = buf["input_partial"][:1]
        eng.evaluate_policy(pol, K, 0, out=buf, input_stats=True)


def section(block, pol):
    off = pol.weight_floats
    return block[:, off: off + 2 * pol.n_in].cpu().numpy()


def test_merge_on_the_device():
    """two successive launches merged by carl_policy_stats_merge equal the reference merge of the same slabs; the
    block's shift / scale are fp32 of the reference, every other float and the set beyond n_write keep their bits"""
    eng = engine_for("cartpole", "round_robin", seed=11)
    tmpl = policy_for(eng, 32, seed=12)
    S, n_in, off = tmpl.set_floats, tmpl.n_in, tmpl.weight_floats
    rng = np.random.default_rng(13)
    host = np.stack([policy_for(eng, 32, seed=20 + k).params[0] for k in range(3)])
    host[:, off: off + 2 * n_in + 1] = tmpl.params[0, off: off + 2 * n_in + 1]  # one transform for every set
    block = torch.as_tensor(host).to(eng.device).contiguous()
    pol = MLPPolicy.on_device(tmpl, block, 256)
    stats = InputStats(tmpl, eng.device)
    ref = SR.fresh(n_in)
    for launch in range(2):
        before = block.clone()
        shift = before[0, off: off + n_in].cpu().numpy()
        res = eng.evaluate_policy(pol, K, T, input_stats=True, deterministic=bool(launch), sample_seed=3)
        stats.update(res, pol, n_write=2)
        n_b = int(res["steps"].sum())
        ref, sh, sc = SR.merge(ref, res["input_partial"].cpu().numpy(), n_b, shift)
        assert int(stats.count) == ref["count"] and n_b > 0
        np.testing.assert_allclose(stats.mean.cpu().numpy(), ref["mean"], rtol=1e-12, atol=0)
        np.testing.assert_allclose((stats.var * stats.count).cpu().numpy(), ref["m2"], rtol=1e-12, atol=0)
        sec = section(block, tmpl)
        for k in range(2):
            np.testing.assert_array_equal(sec[k, :n_in].view(np.uint32), sh.view(np.uint32))
            np.testing.assert_array_equal(sec[k, n_in:].view(np.uint32), sc.view(np.uint32))
        keep = torch.ones(S, dtype=torch.bool, device=eng.device)
        keep[off: off + 2 * n_in] = False
        assert same_bits(block[:2, keep], before[:2, keep]) and same_bits(block[2], before[2])
        assert np.any(sc > 0) and np.any(sc == 0)  # the observation moves; all but one context column are constant
    # an empty launch changes nothing: not the running state, not the block
    state = {k: v.clone() for k, v in stats.state_dict().items()}
    before = block.clone()
    res = eng.evaluate_policy(pol, K, 0, input_stats=True)
    stats.update(res, pol)
    for k, v in stats.state_dict().items():
        assert same_bits(v, state[k]), k
    assert same_bits(block, before)
    # running state only
    res = eng.evaluate_policy(pol, K, T, input_stats=True)
    stats.update(res, policy=pol)
    assert int(stats.count) > ref["count"] and same_bits(block, before)
    # apply_to: one copy, the host policy carries the same transform the device would write
    sh, sc = SR.transform({k: v.numpy() if k != "count" else int(v) for k, v in stats.state_dict().items()})
    applied = stats.apply_to(tmpl)
    np.testing.assert_array_equal(applied.shift, sh)
    np.testing.assert_array_equal(applied.scale, sc)


def test_constant_context_inputs_get_scale_zero():
    """a one-context static table: every context input is constant over the launch -> scale == 0 exactly, under the
    identity transform (d = the raw value, up to 9.8 and 10) and under the test policies' shift (the defaults: d = 0 for all
    but the varied feature)"""
    eng = engine_for("cartpole", "static", seed=21, n_contexts=1)
    for identity in (True, False):
        tmpl = policy_for(eng, 0, seed=22, identity=identity)
        block = torch.as_tensor(tmpl.params).to(eng.device).contiguous().clone()
        pol = MLPPolicy.on_device(tmpl, block, 512)
        stats = InputStats(tmpl, eng.device)
        res = eng.evaluate_policy(pol, K, T, input_stats=True)
        stats.update(res, pol)
        sec = section(block, tmpl)[0]
        n_ctx = len(tmpl.ctx_rows)
        assert n_ctx > 0 and not sec[tmpl.n_in: tmpl.n_in + n_ctx].any()
        assert np.all(sec[tmpl.n_in + n_ctx:] > 0)
        np.testing.assert_allclose(sec[:n_ctx], eng.ctx_table.cpu().numpy()[tmpl.ctx_rows, 0], rtol=2.0 ** -21, atol=0)


def test_es_normalises_from_the_next_generation():
    """two generations of EvolutionStrategy(normalize_inputs=True), CartPole x 512 lanes = 2 sets of 256, linear"""
    def make(normalize):
        eng = make_engine(_lib.CARTPOLE, 512, selector=SELECTORS["static"], n_contexts=N_CTX, seed=31)
        tmpl = MLPPolicy.for_env(eng, rand_layers(np.random.default_rng(32), [eng.F + eng.D, 2]), "identity")
        return EvolutionStrategy(eng, tmpl, lanes_per_set=256, sigma=0.3, lr=0.1, seed=33, normalize_inputs=normalize), tmpl

    es, tmpl = make(True)
    plain, _ = make(False)
    assert plain.input_stats is None and es.input_stats is not None
    n_in, off = tmpl.n_in, tmpl.weight_floats
    ref = SR.fresh(n_in)
    centre_sections = []
    for g in range(2):
        shift = es.center[off: off + n_in].cpu().numpy()
        r = es.step(n_episodes=K, max_steps=T)
        members = section(es.population.params, tmpl)
        for k in range(2):  # the members ran under the centre's section as it was before this step
            np.testing.assert_array_equal(members[k, :n_in].view(np.uint32), shift.view(np.uint32))
            if g > 0:
                np.testing.assert_array_equal(members[k].view(np.uint32), centre_sections[-1].view(np.uint32))
        res = r["result"]
        ref, sh, sc = SR.merge(ref, res["input_partial"].cpu().numpy(), int(res["steps"].sum()), shift)
        sec = es.center[off: off + 2 * n_in].cpu().numpy()
        np.testing.assert_array_equal(sec[:n_in].view(np.uint32), sh.view(np.uint32))
        np.testing.assert_array_equal(sec[n_in:].view(np.uint32), sc.view(np.uint32))
        assert es.center[off + 2 * n_in].item() == float("inf")  # clip kept
        centre_sections.append(sec)
        if g == 0:  # generation 0's statistics have not acted yet: the same generation as without them
            p = plain.step(n_episodes=K, max_steps=T)
            for k in ("fitness", "weight", "grad"):
                assert same_bits(r[k], p[k]), k
            assert same_bits(es.center[:off], plain.center[:off])
            assert "input_partial" not in p["result"]
    assert int(es.input_stats.count) == ref["count"]
    assert not np.array_equal(centre_sections[0], centre_sections[1])


def test_refusals():
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.mixed import MixedVecEngine

    with pytest.raises(NotImplementedError):
        object.__new__(BraxVecEngine).evaluate_policy(None, 1, 1, input_stats=True)
    with pytest.raises(NotImplementedError):
        object.__new__(MixedVecEngine).evaluate_policy(None, 1, 1, input_stats=True)
    eng = make_engine(_lib.CARTPOLE, N, n_contexts=N_CTX, auto_reset=False)
    pol = policy_for(eng, 0, seed=1)
    with pytest.raises(ValueError, match="auto_reset"):
        eng.evaluate_policy(pol, K, T, input_stats=True)
    eng = engine_for("cartpole", "static")
    stats = InputStats(pol, eng.device)
    res = eng.evaluate_policy(pol, K, T, input_stats=True)
    with pytest.raises(ValueError, match="host-built"):
        stats.update(res, pol)
    with pytest.raises(ValueError, match="policy="):
        stats.update(res)
    with pytest.raises(ValueError, match="input_partial"):
        stats.update(eng.evaluate_policy(pol, K, T), policy=pol)


def test_a_reused_result_drops_stale_partials():
    """a result dict reused with input_stats=False loses 'input_partial': the sums of an earlier launch cannot be merged
    beside the later launch's steps (InputStats.update refuses a result without the key)"""
    eng = engine_for("cartpole", "static", seed=5)
    pol = policy_for(eng, 0, seed=3)
    snap = eng.snapshot()
    res = eng.evaluate_policy(pol, K, T, input_stats=True)
    assert "input_partial" in res
    eng.restore(snap)
    again = eng.evaluate_policy(pol, K, T, out=res)
    assert again is res and "input_partial" not in res
    with pytest.raises(ValueError, match="input_partial"):
        InputStats(pol, eng.device).update(res, policy=pol)
