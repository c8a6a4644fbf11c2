"""Host side of the episodes mode of the Brax closed-loop rollout (include/carl_amd.h: carl_brax_evaluate_policy):
everything that runs before a HIP call.  The entry point's refusals by their messages (fake device pointers: nothing is
enqueued), BraxMLPPolicy.unpack against the packing, and the Python refusals of BraxVecEngine.evaluate_episodes and of
EvolutionStrategy with a Brax template on fake engines.  (Its kernel table: test_brax_policy_abi.py, with the other two.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import brax_policy_abi_util as U
import brax_policy_cases as BP
from brax_policy_abi_util import (ant_policy as _ant_policy, batch as _batch, episodes_out as _out,
                                  fake_brax_engine as _fake_brax_engine, info as _info, policy as _policy)
from carl_amd import _lib
from carl_amd import es as ES
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import MLPPolicy
from policy_cases import fake_engine, rand_layers

_refused = functools.partial(U.refused, b"carl_brax_evaluate_policy: ")


def _call(b, s, p, out="all", n_episodes=2, max_steps=10, obs=0x5000):
    out = _out() if out == "all" else out
    return _lib.load().carl_brax_evaluate_policy(C.byref(b), 0x4000, C.byref(s), obs, C.byref(p), n_episodes, max_steps,
                                                 None if out is None else C.byref(out), None)


def test_refusals_by_their_messages():
    ant = BP.build_model("ant")[0]
    hum = BP.build_model("humanoid")[0]
    uns = _lib.ERR_UNSUPPORTED
    # everything carl_brax_rollout_policy checks, in its order: the batch, policy / obs, the kernel class, the policy
    _refused(_call(_batch(n_contexts=0), ant, _policy(ant)), b"n_contexts 0 / ctx_stride 4 invalid")
    _refused(_call(_batch(), ant, _policy(ant), obs=None), b"policy / obs is NULL")
    _refused(_call(_batch(flags=_lib.FLAG_AUTORESET | _lib.FLAG_BRAX_FP32), ant, _policy(ant, n_out=1)),
             b"CARL_FLAG_BRAX_FP32 is not built for the closed-loop rollout (the float64 kernel classes only)", uns)
    _refused(_call(_batch(), hum, _policy(hum)),
             b"2 context inputs + 244 observations are more than CARL_POLICY_MAX_IN = 32 policy inputs "
             b"(Humanoid-size observations are out of scope)")
    _refused(_call(_batch(), ant, _policy(ant, n_out=1)), b"head width 1, the model has 8 actuators")
    _refused(_call(_batch(), ant, _policy(ant, head=_lib.POLICY_HEAD_ARGMAX)),
             b"head kind 0: the Brax families take Box actions (CARL_POLICY_HEAD_BOX)")
    _refused(_call(_batch(), ant, _policy(ant, lanes_per_set=256, n_sets=3)), b"3 sets x 256 lanes do not cover 1000 lanes")
    _refused(_call(_batch(), ant, _policy(ant, lanes_per_set=300)),
             b"lanes_per_set 300 is not a positive multiple of 256 (carl_policy_lane_quantum)")
    _refused(_call(_batch(), ant, _policy(ant, params=0x2004)),
             b"params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)")
    # then the call's own: the policy is checked first (a bad policy with a NULL out is the policy's refusal)
    _refused(_call(_batch(), ant, _policy(ant, n_out=1), out=None), b"head width 1, the model has 8 actuators")
    _refused(_call(_batch(), ant, _policy(ant), out=None), b"out and its six arrays must not be NULL")
    for f, _ in _lib.PolicyEpisodes._fields_:
        _refused(_call(_batch(), ant, _policy(ant), out=_out(**{f: None})), b"out and its six arrays must not be NULL")
    _refused(_call(_batch(), ant, _policy(ant), n_episodes=0), b"n_episodes 0 < 1")
    _refused(_call(_batch(), ant, _policy(ant), max_steps=-1), b"max_steps -1 < 0")
    _refused(_call(_batch(n=1 << 20), ant, _policy(ant, lanes_per_set=1 << 20), n_episodes=1 << 11),
             b"2048 episodes x 1048576 lanes: more than 2^31 - 1 records")
    _refused(_call(_batch(flags=0), ant, _policy(ant)),
             b"needs CARL_FLAG_AUTORESET (without auto-reset a finished lane reports done on every later step, and its "
             b"episode would be counted on each of them)", uns)
    # the argument checks come before the auto-reset refusal
    _refused(_call(_batch(flags=0), ant, _policy(ant), n_episodes=0), b"n_episodes 0 < 1")
    # nothing to do: valid, nothing enqueued
    assert _call(_batch(n=0), ant, _policy(ant)) == 0
    assert _call(_batch(n=0), ant, _policy(ant), max_steps=0) == 0


@pytest.mark.parametrize("widths,act", BP.NETWORKS)
def test_unpack_is_the_inverse_of_the_packing(widths, act):
    rng = np.random.default_rng(5)
    rows = [0, 3]
    tmpl = BraxMLPPolicy(_info(27, 8), rows, BP.make_layers(rng, 29, widths, 8), act)
    layers = BP.make_layers(rng, 29, widths, 8)
    shift, scale, clip = BP.transform(rng, 29)
    packed = BP.pack(layers, shift, scale, clip)  # (written out independently of carl_amd.policy)
    assert packed.size == tmpl.set_floats
    pol = BraxMLPPolicy.unpack(tmpl, packed)
    assert type(pol) is BraxMLPPolicy and pol.n_sets == 1 and pol.lanes_per_set is None and not pol._on_device
    assert pol.params[0].tobytes() == packed.tobytes()
    for (W, b), (W0, b0) in zip(pol.layers, layers):
        assert W.tobytes() == W0.tobytes() and b.tobytes() == b0.tobytes()
    assert pol.shift.tobytes() == shift.tobytes() and pol.scale.tobytes() == scale.tobytes() and pol.clip == np.float32(clip)
    assert (pol.n_in, pol.n_out, pol.widths, pol.activation, pol.ctx_rows) == (29, 8, list(widths), act, rows)
    st, st0 = pol.struct(1000), tmpl.struct(1000)
    for f, _ in _lib.Policy._fields_:
        if f not in ("ctx_rows", "width", "params"):
            assert getattr(st, f) == getattr(st0, f), f
    assert tmpl.params[0].tobytes() != packed.tobytes()  # (the template's own weights are not used, nor changed)
    two = BraxMLPPolicy.stack([pol, BraxMLPPolicy.unpack(tmpl, tmpl.params[0])], 256)
    assert two.params.tobytes() == packed.tobytes() + tmpl.params[0].tobytes()
    with pytest.raises(ValueError, match="floats, the template's weight set has"):
        BraxMLPPolicy.unpack(tmpl, packed[:-4])
    with pytest.raises(ValueError, match="one-set"):
        BraxMLPPolicy.unpack(two, packed)
    with pytest.raises(NotImplementedError, match="log_std"):
        BraxMLPPolicy.unpack(tmpl, packed, log_std=-0.5)
    with pytest.raises(TypeError, match="not a BraxMLPPolicy"):
        BraxMLPPolicy.unpack(MLPPolicy(_lib.PENDULUM, 3, rows, BP.make_layers(rng, 5, widths, 1), act), packed)


def test_python_refusals_of_evaluate_episodes_before_any_launch():
    rng = np.random.default_rng(1)
    eng = _fake_brax_engine()
    pol = _ant_policy(rng)
    with pytest.raises(TypeError, match="evaluate_episodes takes a carl_amd.brax_policy.BraxMLPPolicy, not MLPPolicy"):
        eng.evaluate_episodes(MLPPolicy.for_env(fake_engine(_lib.CARTPOLE, [0, 3]), rand_layers(rng, [6, 2])), 1, 10)
    with pytest.raises(ValueError, match="11 observations and 3 actuators"):
        eng.evaluate_episodes(BraxMLPPolicy(_info(11, 3), [], BP.make_layers(rng, 11, (8,), 3), "relu"), 1, 10)
    with pytest.raises(ValueError, match="evaluate_episodes needs auto_reset=True"):
        _fake_brax_engine(auto_reset=False).evaluate_episodes(pol, 1, 10)
    with pytest.raises(ValueError, match="n_episodes 0 < 1"):
        eng.evaluate_episodes(pol, 0, 10)
    with pytest.raises(ValueError, match="max_steps -1 < 0"):
        eng.evaluate_episodes(pol, 1, -1)
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 records"):
        eng.evaluate_episodes(pol, 1 << 21, 10)
    with pytest.raises(ValueError, match="n_episodes 0 < 1"):
        eng.alloc_policy_episodes(0)
    good = eng.alloc_policy_episodes(2)  # (a CPU "device": buffers only)
    assert {k: (tuple(v.shape), v.dtype) for k, v in good.items()} == {
        "episodes": ((1024,), torch.int32), "steps": ((1024,), torch.int32), "return": ((2, 1024), torch.float32),
        "length": ((2, 1024), torch.int32), "context_id": ((2, 1024), torch.int32), "terminated": ((2, 1024), torch.uint8)}
    for key, spoil in (("return", lambda t: t.double()), ("length", lambda t: t[:1]), ("steps", lambda t: t[::2]),
                       ("terminated", lambda t: None)):
        bad = dict(good)
        bad[key] = spoil(good[key])
        with pytest.raises(ValueError, match=f"evaluate_episodes output '{key}' must be a contiguous"):
            eng.evaluate_episodes(pol, 2, 10, out=bad)
    # the pinned refusal stays, and now names the method that does it
    with pytest.raises(NotImplementedError, match="evaluate_episodes"):
        eng.evaluate_policy(pol, 1, 1)


def test_python_refusals_of_the_brax_evolution_strategy():
    rng = np.random.default_rng(2)
    eng = _fake_brax_engine()
    pol = _ant_policy(rng)
    with pytest.raises(NotImplementedError, match="normalize_inputs"):
        ES.EvolutionStrategy(eng, pol, normalize_inputs=True)
    with pytest.raises(ValueError, match="auto_reset"):
        ES.EvolutionStrategy(_fake_brax_engine(auto_reset=False), pol)
    with pytest.raises(ValueError, match="one-set"):
        ES.EvolutionStrategy(eng, BraxMLPPolicy.stack([pol, pol], 256))
    with pytest.raises(ValueError, match="11 observations and 3 actuators"):
        ES.EvolutionStrategy(eng, BraxMLPPolicy(_info(11, 3), [], BP.make_layers(rng, 11, (8,), 3), "relu"))
    with pytest.raises(ValueError, match="lanes_per_set 100 is not a positive multiple of 256"):
        ES.EvolutionStrategy(eng, pol, lanes_per_set=100)
    with pytest.raises(ValueError, match="lanes beyond"):
        ES.EvolutionStrategy(_fake_brax_engine(n=1100), pol)
    with pytest.raises(ValueError, match="even and at least 2"):
        ES.EvolutionStrategy(_fake_brax_engine(n=768), pol)  # P = 3
    with pytest.raises(ValueError, match="even and at least 2"):
        ES.EvolutionStrategy(eng, pol, lanes_per_set=1024)  # P = 1
    with pytest.raises(ValueError, match="sigma"):
        ES.EvolutionStrategy(eng, pol, sigma=0.0)
    with pytest.raises(ValueError, match="fitness_shaping"):
        ES.EvolutionStrategy(eng, pol, fitness_shaping="ranks")
    with pytest.raises(TypeError, match="not a CARLBraxEnv or BraxVecEngine"):  # a Brax template on a classic engine
        ES.EvolutionStrategy(fake_engine(_lib.CARTPOLE, [0, 3]), pol)
    # a classic template on a Brax engine: today's path, today's refusal
    classic = MLPPolicy.for_env(fake_engine(_lib.CARTPOLE, [0, 3]), rand_layers(rng, [6, 2]))
    with pytest.raises(TypeError, match="classic-control families only"):
        ES.EvolutionStrategy(eng, classic, lanes_per_set=256)
