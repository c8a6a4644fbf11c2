"""Host side of the Brax closed-loop rollout with a critic (include/carl_amd.h: carl_brax_rollout_policy_valued):
everything that runs before a HIP call.  The refusals by their messages and in the header's order (fake device pointers:
nothing is enqueued); the new unit as one expansion of the instance list with its own kernel and the build flags of
carl_brax_policy.hip; the launch shape, which does not know about the critic; the packing of head="value" against a block
written out by hand; and the keyword rules of BraxVecEngine.rollout_policy on a fake engine."""
import ctypes as C
import functools
import inspect
import re

import numpy as np
import pytest

import brax_policy_abi_util as U
import brax_policy_cases as BP
from brax_policy_abi_util import policy as _policy
from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy

WHO = b"carl_brax_rollout_policy_valued: "
_refused = functools.partial(U.refused, WHO)
_critic_refused = functools.partial(U.refused, WHO + b"critic: ")
UNS = _lib.ERR_UNSUPPORTED


def _batch(n=1000, **kw):
    kw.setdefault("max_episode_steps", 1000)
    return U.batch(n, **kw)


def _io():
    io = _lib.StepIO()
    io.action, io.obs, io.reward, io.terminated, io.truncated = 0x1000, 0x1000, 0x1000, 0x1000, 0x1000
    io.action_dtype = _lib.ACTION_F32
    return io


def _critic(s, **kw):
    """a valid critic beside brax_policy_abi_util.policy(s): 1 x 32 relu, one output, a block of its own"""
    kw = {"n_out": 1, "n_hidden": 1, "activation": _lib.POLICY_RELU, "params": 0x6000, **kw}
    c = _policy(s, **kw)
    c.width[0] = 32
    return c


def _smp(log_std=0x7000, log_prob=0x8000, seed=1):
    return _lib.PolicySampling(seed, log_std, log_prob)


def _out(value=0x9000, last_value=0xA000, boot_value=0xB000):
    return _lib.PolicyValue(value, last_value, boot_value)


def _call(b, s, p, c="default", smp="default", io="default", out="default", summary=False, n_steps=10, obs=0x5000):
    c = _critic(s) if c == "default" else c
    smp = _smp() if smp == "default" else smp
    io = _io() if io == "default" else io
    out = _out() if out == "default" else out
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    return _lib.load().carl_brax_rollout_policy_valued(C.byref(b), 0x4000, C.byref(s), obs, C.byref(p), ref(c), ref(smp),
                                                       ref(io), n_steps, C.byref(summ) if summary else None, ref(out), None)


def test_refusals_by_their_messages_in_order():
    ant = BP.build_model("ant")[0]
    hum = BP.build_model("humanoid")[0]
    p = _policy(ant)
    bad = dict(c=None, smp=None, out=None)  # everything behind a check is spoiled too: the order is the header's
    # 1. validate_closed_loop
    _refused(_call(_batch(n_contexts=0), ant, p, **bad), b"n_contexts 0 / ctx_stride 4 invalid")
    _refused(_call(_batch(), ant, p, obs=None, **bad), b"policy / obs is NULL")
    _refused(_call(_batch(flags=_lib.FLAG_AUTORESET | _lib.FLAG_BRAX_FP32), ant, p, **bad),
             b"CARL_FLAG_BRAX_FP32 is not built for the closed-loop rollout (the float64 kernel classes only)", UNS)
    _refused(_call(_batch(), hum, _policy(hum), **bad),
             b"2 context inputs + 244 observations are more than CARL_POLICY_MAX_IN = 32 policy inputs "
             b"(Humanoid-size observations are out of scope)")
    _refused(_call(_batch(), ant, _policy(ant, n_out=1), **bad), b"head width 1, the model has 8 actuators")
    _refused(_call(_batch(), ant, _policy(ant, params=0x2004), **bad),
             b"params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)")
    # 2. validate_rollout
    _refused(_call(_batch(), ant, p, n_steps=-1, **bad), b"n_steps -1 < 0")
    io = _io()
    io.row_pitch = 1008
    _refused(_call(_batch(), ant, p, io=io, **bad), b"Brax families take dense rows (io.row_pitch = 0)")
    _refused(_call(_batch(flags=0), ant, p, summary=True, **bad),
             b"a summary needs CARL_FLAG_AUTORESET (without auto-reset a finished lane reports done on every later "
             b"step, and its episode would be counted on each of them)", UNS)
    # 3. transitions mode only: a summary launch is refused, whatever else it passes
    _refused(_call(_batch(), ant, p, io=None, summary=True, **bad),
             b"io is NULL -- transitions mode only (a summary has no use for values)")
    _refused(_call(_batch(), ant, p, io=None, summary=True),
             b"io is NULL -- transitions mode only (a summary has no use for values)")
    # 4. the sampling checks, sampling and log_prob required
    _refused(_call(_batch(), ant, p, c=None, smp=None, out=None), b"sampling is NULL")
    _refused(_call(_batch(), ant, p, c=None, smp=_smp(log_std=None), out=None),
             b"sampling->log_std is NULL (one value per weight set and actuator)")
    wide = BP.build_model("ant")[0]
    wide.n_act = 9
    _refused(_call(_batch(), wide, _policy(wide), c=None, out=None),
             b"9 actuators: the draws' counter holds the Philox block in two bits (at most 8 actuators)")
    _refused(_call(_batch(max_episode_steps=0), ant, p, c=None, out=None),
             b"max_episode_steps 0 outside [1, 2^28]: the draws' counter holds the step count of an episode in 28 bits")
    _refused(_call(_batch(), ant, p, c=None, smp=_smp(log_prob=None), out=None),
             b"sampling->log_prob is NULL (a valued launch always stores the log-probabilities)")
    # 5. the critic, each refusal with a message of its own
    _refused(_call(_batch(), ant, p, c=None, out=None), b"critic is NULL")
    c = _critic(ant)
    c.width[0] = 65
    assert _call(_batch(), ant, p, c=c, out=None) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().carl_last_error().startswith(WHO + b"critic: ")
    _critic_refused(_call(_batch(), ant, p, c=_critic(ant, n_out=2), out=None), b"head width 2, a value network has 1")
    _critic_refused(_call(_batch(), ant, p, c=_critic(ant, n_in=28), out=None),
                    b"n_in 28 / n_ctx 2, the actor has 29 / 2 (the critic reads the actor's inputs)")
    c = _critic(ant)
    c.ctx_rows[1] = 0
    _critic_refused(_call(_batch(), ant, p, c=c, out=None), b"ctx_rows[1] = 0, the actor's is 1")
    assert _call(_batch(), ant, p, c=_critic(ant, activation=7), out=None) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().carl_last_error().startswith(WHO + b"critic: ")
    _critic_refused(_call(_batch(), ant, p, c=_critic(ant, n_sets=2), out=None), b"2 sets x 1024 lanes, the actor has 1 x 1024")
    _critic_refused(_call(_batch(), ant, p, c=_critic(ant, lanes_per_set=2048), out=None),
                    b"1 sets x 2048 lanes, the actor has 1 x 1024")
    assert _call(_batch(), ant, p, c=_critic(ant, params=None), out=None) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().carl_last_error().startswith(WHO + b"critic: ")
    _critic_refused(_call(_batch(), ant, p, c=_critic(ant, params=0x6004), out=None),
                    b"params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)")
    # head is not read
    assert _call(_batch(n=0), ant, p, c=_critic(ant, head=_lib.POLICY_HEAD_ARGMAX)) == 0
    # 6. the output columns
    for out in (None, _out(value=None), _out(last_value=None)):
        _refused(_call(_batch(), ant, p, out=out), b"out, out->value and out->last_value are required")
    _refused(_call(_batch(flags=0), ant, p),
             b"out->boot_value needs CARL_FLAG_AUTORESET (without auto-reset no terminal observation is kept apart from "
             b"the next one)", UNS)
    # nothing to do: valid, nothing enqueued
    assert _call(_batch(n=0), ant, p) == 0
    assert _call(_batch(n=0), ant, p, summary=True) == 0
    assert _call(_batch(n=0, flags=0), ant, p, out=_out(boot_value=None)) == 0
    _refused(_call(_batch(n=0), ant, p, out=None), b"out, out->value and out->last_value are required")


def test_the_unit_is_one_expansion_of_the_instance_list_with_its_own_kernel():
    src = U.source("carl_brax_policy_value.hip", comments=False)
    table = re.search(r"#define X\(M, K, T, P\) \{\{M, T, P, false\}, K, carl::brax::(\w+)<M, K, T, P>\},\n"
                      r"const [\w:<>]+ \w+\[\] = \{\s*CARL_BRAX_CLOSED_LOOP_INSTANCES\(X\)\};\n#undef X\n", src)
    assert table is not None and table.group(1) == "brax_policy_valued_kernel"
    rest = src.replace(table.group(0), "")
    assert "CARL_BRAX_CLOSED_LOOP_INSTANCES" not in rest
    assert not re.search(r"brax_\w*_kernel\s*<", rest)
    assert not re.search(r"\((true|false), \d+, (true|false), (true|false)\)", rest)
    assert "launch_closed_loop(kBraxValuedKernels" in rest
    # boot_value == NULL is a runtime branch: one kernel template; the step text is run()'s, not a copy
    hdr = U.source("brax_value_kernels.hip.h", comments=False)
    assert len(re.findall(r"__global__", hdr)) == 1 and "brax_policy_valued_kernel(" in hdr
    assert "struct BraxValuedPolicy : BraxSampledPolicy" in hdr and "kValued = true" in hdr
    assert "substep" not in hdr and "select_context" not in hdr
    assert len(re.findall(r"__global__", U.source("brax_sample_kernels.hip.h", comments=False))) == 1
    for unit in ("carl_brax.hip", "carl_brax_policy.hip", "carl_brax_episodes.hip", "carl_brax_policy_stats.hip",
                 "carl_brax_policy_sample.hip"):
        other = U.source(unit)
        assert "brax_policy_valued_kernel" not in other and "BraxValuedPolicy" not in other, unit
        assert "brax_value_kernels.hip.h" not in other, unit
    from carl_amd.build import SOURCES

    assert SOURCES["carl_brax_policy_value.hip"] == SOURCES["carl_brax_policy.hip"]


def test_launch_shape_is_unchanged():
    """no new LDS rows: the policy rows are still 32 + 64 + 64 + 4 per env, and the query takes no critic"""
    assert len(_lib.EXPORTS["carl_brax_policy_launch_shape"][1]) == 5
    assert _lib.EXPORTS["carl_brax_rollout_policy_valued"][1][5]._type_ is _lib.Policy
    assert _lib.EXPORTS["carl_brax_rollout_policy_valued"][1][10]._type_ is _lib.PolicyValue
    s = BP.build_model("ant")[0]
    for n, T in ((300, 8), (32768, 100)):
        code, sh = BP.launch_shape(_batch(n), s, _policy(s), T)
        code2, op = BP.open_launch_shape(_batch(n), s, 1, T)
        assert code == 0 and code2 == 0 and op.lanes_per_env == sh.lanes_per_env
        envs = 64 // sh.lanes_per_env
        assert (sh.lds_bytes // sh.waves_per_workgroup) - (op.lds_bytes // op.waves_per_workgroup) == 164 * 4 * envs
    src = U.source("brax_kernels.hip.h", comments=False)
    assert "kPolicyXRows = 32, kPolicyHRows = 64, kPolicySumRows = 4;" in src
    assert "brax_value_kernels" not in U.source("brax_launch.hpp") and "kValued" not in U.source("brax_launch.hpp")


def test_packing_of_a_value_head_against_a_block_written_by_hand():
    rng = np.random.default_rng(5)
    layers = BP.make_layers(rng, 29, (5, 3), 1)
    shift, scale, clip = BP.transform(rng, 29)
    c = BraxMLPPolicy(U.info(27, 8), [0, 1], layers, "tanh", shift, scale, clip, head="value")
    assert c.head == "value" and c.n_out == 1 and c.log_std.shape == (1, 0)
    (W0, b0), (W1, b1), (W2, b2) = layers
    by_hand = np.concatenate([W0.reshape(-1), b0, W1.reshape(-1), b1, W2.reshape(-1), b2, shift, scale, [clip]]).astype(np.float32)
    assert by_hand.size == 5 * 29 + 5 + 3 * 5 + 3 + 3 + 1 + 29 + 29 + 1
    by_hand = np.concatenate([by_hand, np.zeros((-by_hand.size) % 4, np.float32)])
    np.testing.assert_array_equal(c.params[0].view(np.int32), by_hand.view(np.int32))
    st = c.struct(1000, 0x6000)
    assert (st.n_out, st.n_in, st.n_ctx, st.n_hidden, st.width[0], st.width[1]) == (1, 29, 2, 2, 5, 3)
    assert _lib.load().carl_brax_policy_set_floats(C.byref(st)) == by_hand.size == c.set_floats
    # stack keeps the head and the empty log_std; a wrong head width and a log_std are refused
    two = BraxMLPPolicy.stack([c, c], 256, head="value")
    assert two.n_sets == 2 and two.head == "value" and two.log_std.shape == (2, 0)
    with pytest.raises(ValueError, match="a value network has one output"):
        BraxMLPPolicy(U.info(27, 8), [0, 1], BP.make_layers(rng, 29, (5,), 8), "tanh", head="value")
    with pytest.raises(ValueError, match="a value network samples nothing"):
        BraxMLPPolicy(U.info(27, 8), [0, 1], layers, "tanh", head="value", log_std=0.0)
    for fn in (BraxMLPPolicy.__init__, BraxMLPPolicy.for_env):
        assert inspect.signature(fn).parameters["head"].default == "policy"
    assert BraxMLPPolicy.unpack(c, c.params[0]).head == "value"


def test_python_keyword_rules_before_any_launch():
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.engine import VecEngine
    from carl_amd.envs.brax.carl_brax_env import CARLBraxEnv
    from carl_amd.policy import MLPPolicy

    for fn in (BraxVecEngine.rollout_policy, CARLBraxEnv.rollout_policy):
        par = inspect.signature(fn).parameters
        ref = inspect.signature(VecEngine.rollout_policy).parameters
        for k in ("value_net", "bootstrap_truncated", "gae"):
            assert par[k].kind is inspect.Parameter.KEYWORD_ONLY and par[k].default == ref[k].default, k
    rng = np.random.default_rng(1)
    eng = U.fake_brax_engine()
    pol = U.ant_policy(rng, rows=(0, 1))

    def mk(rows=(0, 1), **kw):
        return BraxMLPPolicy(U.info(27, 8), list(rows), BP.make_layers(rng, 27 + len(rows), (8,), 1), "tanh",
                             head="value", **kw)

    crit = mk()
    go = dict(deterministic=False, value_net=crit)
    with pytest.raises(ValueError, match="value_net: sampled launches only"):
        eng.rollout_policy(pol, 4, value_net=crit)
    with pytest.raises(ValueError, match="value_net: transitions mode only"):
        eng.rollout_policy(pol, 4, mode="summary", **go)
    with pytest.raises(ValueError, match="gae=.* needs value_net"):
        eng.rollout_policy(pol, 4, deterministic=False, gae=(0.99, 0.95))
    # not a one-output BraxMLPPolicy of this model
    with pytest.raises(ValueError, match="value_net must be a carl_amd.brax_policy.BraxMLPPolicy built with head='value'"):
        eng.rollout_policy(pol, 4, deterministic=False, value_net=pol)
    classic = object.__new__(MLPPolicy)
    classic.head, classic.n_out, classic.obs_dim = "value", 1, 27
    with pytest.raises(ValueError, match="value_net must be a carl_amd.brax_policy.BraxMLPPolicy"):
        eng.rollout_policy(pol, 4, deterministic=False, value_net=classic)
    other = BraxMLPPolicy(U.info(17, 6), [0, 1], BP.make_layers(rng, 19, (8,), 1), "tanh", head="value")
    with pytest.raises(ValueError, match="for this engine's model"):
        eng.rollout_policy(pol, 4, deterministic=False, value_net=other)
    # context rows, set layout, transform
    with pytest.raises(ValueError, match="value_net reads context rows"):
        eng.rollout_policy(pol, 4, deterministic=False, value_net=mk(rows=[1, 0]))
    with pytest.raises(ValueError, match="weight sets"):
        eng.rollout_policy(pol, 4, deterministic=False, value_net=BraxMLPPolicy.stack([crit, crit], 512))
    with pytest.raises(ValueError, match="weight sets"):
        eng.rollout_policy(BraxMLPPolicy.stack([pol, pol], 512), 4, deterministic=False,
                           value_net=BraxMLPPolicy.stack([crit, crit], 1024))
    with pytest.raises(ValueError, match="bit for bit"):
        eng.rollout_policy(pol, 4, deterministic=False, value_net=mk(input_shift=np.full(29, 1e-3)))
    with pytest.raises(ValueError, match="bit for bit"):
        eng.rollout_policy(pol, 4, deterministic=False, value_net=mk(input_clip=5.0))
    # the timeout bootstrap needs auto-reset, and says how to do without
    with pytest.raises(ValueError, match=r"bootstrap_truncated=True needs auto_reset=True.*bootstrap_truncated=False"):
        U.fake_brax_engine(auto_reset=False).rollout_policy(pol, 4, **go)
