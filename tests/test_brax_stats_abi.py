"""Host side of the input statistics of the Brax closed-loop rollout (include/carl_amd.h: carl_brax_evaluate_policy_stats,
carl_brax_policy_stats_slabs, carl_brax_policy_stats_merge): everything that runs before a HIP call.  The refusals of both
new entry points by their messages (fake device pointers: nothing is enqueued), the slab count against
carl_brax_policy_launch_shape, InputStats' offsets with an Ant template, and the keyword rules of EvolutionStrategy on fake
engines.  (The kernel table: test_brax_policy_abi.py, with the other two.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import brax_policy_abi_util as U
import brax_policy_cases as BP
import stats_ref as SR
from brax_policy_abi_util import (ant_policy as _ant_policy, batch as _batch, episodes_out as _out,
                                  fake_brax_engine as _fake_brax_engine, policy as _policy)
from carl_amd import _lib
from carl_amd import es as ES
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import InputStats, MLPPolicy
from policy_cases import fake_engine, rand_layers

_refused = functools.partial(U.refused, b"carl_brax_evaluate_policy_stats: ")
PTR = 0x6000


def _slabs(b, s, p, max_steps=10):
    return int(_lib.load().carl_brax_policy_stats_slabs(C.byref(b), C.byref(s), C.byref(p), max_steps))


def _call(b, s, p, out="all", n_episodes=2, max_steps=10, obs=0x5000, stats="enough"):
    out = _out() if out == "all" else out
    if stats == "enough":
        stats = _lib.PolicyStats(PTR, max(_slabs(b, s, p, max(max_steps, 0)), 0))
    return _lib.load().carl_brax_evaluate_policy_stats(
        C.byref(b), 0x4000, C.byref(s), obs, C.byref(p), n_episodes, max_steps, None if out is None else C.byref(out),
        None if stats is None else C.byref(stats), None)


def test_evaluate_stats_refusals_by_their_messages():
    ant = BP.build_model("ant")[0]
    hum = BP.build_model("humanoid")[0]
    uns = _lib.ERR_UNSUPPORTED
    # everything carl_brax_evaluate_policy checks, in its order, spot-checked -- each with a NULL stats, whose refusal
    # comes last
    _refused(_call(_batch(n_contexts=0), ant, _policy(ant), stats=None), b"n_contexts 0 / ctx_stride 4 invalid")
    _refused(_call(_batch(), ant, _policy(ant), obs=None, stats=None), b"policy / obs is NULL")
    _refused(_call(_batch(flags=_lib.FLAG_AUTORESET | _lib.FLAG_BRAX_FP32), ant, _policy(ant), stats=None),
             b"CARL_FLAG_BRAX_FP32 is not built for the closed-loop rollout (the float64 kernel classes only)", uns)
    _refused(_call(_batch(), hum, _policy(hum), stats=None),
             b"2 context inputs + 244 observations are more than CARL_POLICY_MAX_IN = 32 policy inputs "
             b"(Humanoid-size observations are out of scope)")
    _refused(_call(_batch(), ant, _policy(ant, n_out=1), out=None, stats=None), b"head width 1, the model has 8 actuators")
    _refused(_call(_batch(), ant, _policy(ant, params=0x2004), stats=None),
             b"params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)")
    _refused(_call(_batch(), ant, _policy(ant), out=None, stats=None), b"out and its six arrays must not be NULL")
    _refused(_call(_batch(), ant, _policy(ant), out=_out(steps=None), stats=None), b"out and its six arrays must not be NULL")
    _refused(_call(_batch(), ant, _policy(ant), n_episodes=0, stats=None), b"n_episodes 0 < 1")
    _refused(_call(_batch(), ant, _policy(ant), max_steps=-1, stats=None), b"max_steps -1 < 0")
    _refused(_call(_batch(n=1 << 20), ant, _policy(ant, lanes_per_set=1 << 20), n_episodes=1 << 11, stats=None),
             b"2048 episodes x 1048576 lanes: more than 2^31 - 1 records")
    _refused(_call(_batch(flags=0), ant, _policy(ant), stats=None),
             b"needs CARL_FLAG_AUTORESET (without auto-reset a finished lane reports done on every later step, and its "
             b"episode would be counted on each of them)", uns)
    # then the statistics output
    b, p = _batch(), _policy(ant)
    n_slabs = _slabs(b, ant, p)
    assert n_slabs > 0
    _refused(_call(b, ant, p, stats=None), b"stats / stats->partial is NULL")
    _refused(_call(b, ant, p, stats=_lib.PolicyStats(None, n_slabs)), b"stats / stats->partial is NULL")
    for off in (4, 8, 12):
        _refused(_call(b, ant, p, stats=_lib.PolicyStats(PTR + off, n_slabs)), b"stats->partial is not on a 16-byte boundary")
    _refused(_call(b, ant, p, stats=_lib.PolicyStats(PTR, n_slabs - 1)),
             b"stats->partial_capacity %d < %d slabs (carl_brax_policy_stats_slabs)" % (n_slabs - 1, n_slabs))
    # max_steps == 0 has the slabs of a one-step launch, and they are asked for
    n0 = _slabs(b, ant, p, 0)
    assert n0 == _slabs(b, ant, p, 1) > 0
    _refused(_call(b, ant, p, max_steps=0, stats=_lib.PolicyStats(PTR, n0 - 1)),
             b"stats->partial_capacity %d < %d slabs (carl_brax_policy_stats_slabs)" % (n0 - 1, n0))
    # nothing to do: valid, nothing enqueued, no slab -- but the statistics output is still checked
    assert _call(_batch(n=0), ant, p, stats=_lib.PolicyStats(PTR, 0)) == 0
    assert _call(_batch(n=0), ant, p, max_steps=0, stats=_lib.PolicyStats(PTR, 0)) == 0
    _refused(_call(_batch(n=0), ant, p, stats=None), b"stats / stats->partial is NULL")


@pytest.mark.parametrize("model", ["ant", "hopper", "halfcheetah", "inverted_pendulum", "reacher"])
def test_slab_count_is_the_launch_shape(model):
    s = BP.build_model(model)[0]
    p = _policy(s, lanes_per_set=1 << 20)
    for n in (1, 77, 1000, 32768, 100000):
        for steps in (1, 3, 12, 1000):
            b = _batch(n=n)
            code, sh = BP.launch_shape(b, s, p, steps)
            assert code == 0
            assert _slabs(b, s, p, steps) == sh.grid * sh.waves_per_workgroup > 0
        assert _slabs(_batch(n=n), s, p, 0) == _slabs(_batch(n=n), s, p, 1)
    lib = _lib.load()
    assert _slabs(_batch(n=0), s, p) == 0 and _slabs(_batch(n=-3), s, p) == 0
    assert lib.carl_brax_policy_stats_slabs(None, C.byref(s), C.byref(p), 10) == -1
    assert lib.carl_brax_policy_stats_slabs(C.byref(_batch()), None, C.byref(p), 10) == -1
    assert lib.carl_brax_policy_stats_slabs(C.byref(_batch()), C.byref(s), None, 10) == -1
    assert _slabs(_batch(), s, p, -1) == -1
    assert _slabs(_batch(flags=_lib.FLAG_AUTORESET | _lib.FLAG_BRAX_FP32), s, p) == -1


def _running(**kw):
    r = _lib.PolicyRunningStats(PTR, PTR, PTR)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _stats(partial=PTR, capacity=4):
    return _lib.PolicyStats(partial, capacity)


def _merge(p="default", stats="default", n_slabs=4, steps=PTR, n=1000, running="default", eps=1e-8, min_std=1e-6,
           out=PTR, n_write=1, entry="carl_brax_policy_stats_merge"):
    p = _policy(BP.build_model("ant")[0]) if p == "default" else p
    stats = _stats() if stats == "default" else stats
    running = _running() if running == "default" else running
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    return getattr(_lib.load(), entry)(ref(p), ref(stats), n_slabs, steps, n, ref(running), eps, min_std, out, n_write, None)


_ANT = BP.build_model("ant")[0]


@pytest.mark.parametrize("kw, msg", [
    (dict(p=None), b"policy is NULL"),
    (dict(p=_policy(_ANT, width=(65, 64))), b"shape is outside the limits"),
    (dict(p=_policy(_ANT, n_in=33)), b"shape is outside the limits"),
    (dict(p=_policy(_ANT, n_out=_lib.BRAX_MAX_ACT + 1)), b"shape is outside the limits"),
    (dict(p=_policy(_ANT, params=None)), b"params is NULL"),
    (dict(n_slabs=-1), b"n_workgroups -1 < 0"),
    (dict(stats=None), b"stats / stats->partial is NULL"),
    (dict(stats=_stats(partial=None)), b"stats / stats->partial is NULL"),
    (dict(stats=_stats(partial=PTR + 8)), b"not on a 16-byte boundary"),
    (dict(n_slabs=5), b"partial_capacity 4 < 5 slabs (carl_brax_policy_stats_slabs)"),
    (dict(n=-1), b"n_lanes -1 < 0"),
    (dict(steps=None), b"steps is NULL"),
    (dict(running=None), b"running and its three arrays"),
    (dict(running=_running(count=None)), b"running and its three arrays"),
    (dict(running=_running(mean=None)), b"running and its three arrays"),
    (dict(running=_running(m2=None)), b"running and its three arrays"),
    (dict(eps=-1e-9), b"eps -1e-09 is not finite and >= 0"),
    (dict(eps=float("nan")), b"is not finite and >= 0"),
    (dict(min_std=float("inf")), b"min_std inf is not finite and >= 0"),
    (dict(min_std=-1.0), b"min_std -1 is not finite and >= 0"),
    (dict(n_write=-1), b"n_write -1 < 0"),
], ids=lambda v: None if isinstance(v, dict) else v.decode()[:28])
def test_merge_refusals(kw, msg):
    assert _merge(**kw) == _lib.ERR_INVALID_ARGUMENT
    err = _lib.load().carl_last_error()
    assert err.startswith(b"carl_brax_policy_stats_merge:") and msg in err, err


def test_the_classic_merge_keeps_refusing_a_brax_shape():
    """8 outputs are outside carl_policy_set_floats' limits: carl_policy_stats_merge refuses what the Brax entry point takes
    (and that one gets past the shape check: its next refusal is the NULL params)"""
    assert _merge(entry="carl_policy_stats_merge") == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().carl_last_error() == b"carl_policy_stats_merge: the policy's shape is outside the limits"
    assert _merge(p=_policy(_ANT, params=None)) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().carl_last_error() == b"carl_brax_policy_stats_merge: params is NULL"


@pytest.mark.parametrize("widths", [(64, 64), (32,), ()])
def test_input_stats_with_an_ant_template(widths):
    """29 inputs, 8 outputs: the offsets the merge writes at are the packing's, and the Brax entry point is the one called"""
    rng = np.random.default_rng(7)
    tmpl = _ant_policy(rng, widths, rows=(0, 3))
    assert (tmpl.n_in, tmpl.n_out) == (29, 8)
    p_shift, p_scale, p_clip, S = SR.transform_offsets(29, widths, 8)
    assert (tmpl.weight_floats, tmpl.set_floats) == (p_shift, S)
    st = tmpl.struct(1000, 0x2000)
    assert int(_lib.load().carl_brax_policy_set_floats(C.byref(st))) == S
    assert int(_lib.load().carl_policy_set_floats(C.byref(st))) == -1  # (the classic rule refuses 8 outputs)
    assert type(tmpl)._STATS_MERGE == "carl_brax_policy_stats_merge" and MLPPolicy._STATS_MERGE == "carl_policy_stats_merge"
    stats = InputStats(tmpl, "cpu")
    assert stats.n_in == 29
    state = {"count": torch.tensor([5]), "mean": torch.arange(29, dtype=torch.float64), "m2": torch.full((29,), 20.0).double()}
    state["m2"][3] = 0.0
    stats.load_state_dict(state)
    shift, scale = stats.transform()
    np.testing.assert_array_equal(shift, np.arange(29, dtype=np.float32))
    assert scale[3] == 0.0 and np.all(np.delete(scale, 3) == np.float32(1.0 / np.sqrt(4.0 + 1e-8)))
    applied = stats.apply_to(tmpl)
    assert type(applied) is BraxMLPPolicy
    flat = applied.params[0]
    np.testing.assert_array_equal(flat[p_shift: p_scale], shift)
    np.testing.assert_array_equal(flat[p_scale: p_clip], scale)
    keep = np.ones(S, bool)
    keep[p_shift: p_clip] = False
    assert flat[keep].tobytes() == tmpl.params[0][keep].tobytes()
    for k, v in stats.state_dict().items():
        assert torch.equal(v.double().reshape(-1), state[k].double().reshape(-1)), k


def _fake_classic_engine():
    eng = fake_engine(_lib.CARTPOLE, [0, 3])
    eng.b = _lib.Batch()  # (auto_reset is a flag of the batch)
    eng.n, eng.auto_reset, eng.device = 1024, True, torch.device("cpu")
    return eng


def test_evolution_strategy_keyword_rules():
    rng = np.random.default_rng(2)
    eng = _fake_brax_engine()
    pol = _ant_policy(rng, rows=())
    # On a fake engine (a CPU "device") a constructor that has passed every check of its arguments stops where it wraps the
    # population's device block: that refusal, and no other, is "accepted" here.  The GPU tests construct for real.
    def accepted(*a, **kw):
        with pytest.raises(ValueError, match=r"on_device\(\): params must live on a GPU"):
            ES.EvolutionStrategy(*a, **kw)

    # a Brax template: input_stats= is the route, normalize_inputs=True still refused and says so
    stats = InputStats(pol, "cpu")
    accepted(eng, pol)
    accepted(eng, pol, input_stats=stats)
    with pytest.raises(NotImplementedError, match="normalize_inputs.*input_stats="):
        ES.EvolutionStrategy(eng, pol, normalize_inputs=True)
    with pytest.raises(NotImplementedError, match="normalize_inputs"):
        ES.EvolutionStrategy(eng, pol, normalize_inputs=True, input_stats=stats)
    # a classic template: both routes, not at once
    ceng = _fake_classic_engine()
    classic = MLPPolicy.for_env(ceng, rand_layers(rng, [6, 2]))
    cstats = InputStats(classic, "cpu")
    accepted(ceng, classic, lanes_per_set=256, input_stats=cstats)
    accepted(ceng, classic, lanes_per_set=256, normalize_inputs=True)
    with pytest.raises(ValueError, match="one of the two"):
        ES.EvolutionStrategy(ceng, classic, lanes_per_set=256, normalize_inputs=True, input_stats=cstats)
    # a wrong shape, a wrong family, a wrong object
    with pytest.raises(ValueError, match="input_stats: an InputStats built for a BraxMLPPolicy"):
        ES.EvolutionStrategy(eng, pol, input_stats=InputStats(_ant_policy(rng, widths=(16,), rows=()), "cpu"))
    with pytest.raises(ValueError, match="input_stats: an InputStats built for a BraxMLPPolicy"):
        ES.EvolutionStrategy(eng, pol, input_stats=cstats)
    with pytest.raises(ValueError, match="input_stats: an InputStats built for a MLPPolicy"):
        ES.EvolutionStrategy(ceng, classic, lanes_per_set=256, input_stats=stats)
    with pytest.raises(ValueError, match="input_stats: an InputStats built for"):
        ES.EvolutionStrategy(eng, pol, input_stats=object())


def test_python_refusals_of_the_keyword_before_any_launch():
    rng = np.random.default_rng(1)
    eng = _fake_brax_engine()
    pol = _ant_policy(rng, rows=())
    with pytest.raises(ValueError, match="evaluate_episodes needs auto_reset=True"):
        _fake_brax_engine(auto_reset=False).evaluate_episodes(pol, 1, 10, input_stats=True)
    with pytest.raises(ValueError, match="n_episodes 0 < 1"):
        eng.evaluate_episodes(pol, 0, 10, input_stats=True)
    with pytest.raises(ValueError, match="input_partial"):
        InputStats(pol, "cpu").update({"steps": torch.zeros(4, dtype=torch.int32)}, policy=pol)
