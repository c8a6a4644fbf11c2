"""Host side of the sampled Brax closed-loop rollout (include/carl_amd.h: carl_brax_rollout_policy_sampled): everything
that runs before a HIP call.  The refusals by their messages, the deterministic call's first (fake device pointers:
nothing is enqueued); the new unit as one expansion of the instance list with the build flags of carl_brax_policy.hip;
the helper's counter and word selection against oracle.philox4x32_10; BraxMLPPolicy's log_std shapes; the launch shape,
which does not know whether a launch samples; the keyword rules of BraxVecEngine.rollout_policy on a fake engine; and
the float64 draws of the GPU independence check inside their own 5-sigma bounds."""
import ctypes as C
import functools
import inspect
import re

import numpy as np
import pytest

import brax_policy_abi_util as U
import brax_policy_cases as BP
import brax_sampling_cases as BS
from brax_policy_abi_util import policy as _policy
from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy
from oracle import oracle as O

_refused = functools.partial(U.refused, b"carl_brax_rollout_policy_sampled: ")
UNS = _lib.ERR_UNSUPPORTED


def _batch(n=1000, **kw):
    kw.setdefault("max_episode_steps", 1000)  # (the sampled call needs a TimeLimit: its counter holds elapsed in 28 bits)
    return U.batch(n, **kw)


def _io():
    io = _lib.StepIO()
    io.action, io.obs, io.reward, io.terminated, io.truncated = 0x1000, 0x1000, 0x1000, 0x1000, 0x1000
    io.action_dtype = _lib.ACTION_F32
    return io


def _smp(log_std=0x7000, log_prob=None, seed=1):
    return _lib.PolicySampling(seed, log_std, log_prob)


def _call(b, s, p, smp="default", io=None, summary=True, n_steps=10, obs=0x5000):
    smp = _smp() if smp == "default" else smp
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    return _lib.load().carl_brax_rollout_policy_sampled(
        C.byref(b), 0x4000, C.byref(s), obs, C.byref(p), None if smp is None else C.byref(smp),
        None if io is None else C.byref(io), n_steps, C.byref(summ) if summary else None, None)


def test_refusals_by_their_messages():
    ant = BP.build_model("ant")[0]
    hum = BP.build_model("humanoid")[0]
    # everything carl_brax_rollout_policy checks, in its order and with its codes -- each with a NULL sampling, whose
    # refusal comes after them
    _refused(_call(_batch(n_contexts=0), ant, _policy(ant), smp=None), b"n_contexts 0 / ctx_stride 4 invalid")
    _refused(_call(_batch(), ant, _policy(ant), smp=None, obs=None), b"policy / obs is NULL")
    _refused(_call(_batch(flags=_lib.FLAG_AUTORESET | _lib.FLAG_BRAX_FP32), ant, _policy(ant), smp=None),
             b"CARL_FLAG_BRAX_FP32 is not built for the closed-loop rollout (the float64 kernel classes only)", UNS)
    _refused(_call(_batch(), hum, _policy(hum), smp=None),
             b"2 context inputs + 244 observations are more than CARL_POLICY_MAX_IN = 32 policy inputs "
             b"(Humanoid-size observations are out of scope)")
    _refused(_call(_batch(), ant, _policy(ant, n_out=1), smp=None), b"head width 1, the model has 8 actuators")
    _refused(_call(_batch(), ant, _policy(ant, head=_lib.POLICY_HEAD_ARGMAX), smp=None),
             b"head kind 0: the Brax families take Box actions (CARL_POLICY_HEAD_BOX)")
    _refused(_call(_batch(), ant, _policy(ant, lanes_per_set=256, n_sets=3), smp=None),
             b"3 sets x 256 lanes do not cover 1000 lanes")
    _refused(_call(_batch(), ant, _policy(ant, params=0x2004), smp=None),
             b"params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)")
    _refused(_call(_batch(), ant, _policy(ant), smp=None, n_steps=-1), b"n_steps -1 < 0")
    _refused(_call(_batch(), ant, _policy(ant), smp=None, io=None, summary=False),
             b"summary mode (io NULL) needs all three summary arrays")
    io = _io()
    io.row_pitch = 1008
    _refused(_call(_batch(), ant, _policy(ant), smp=None, io=io, summary=False),
             b"Brax families take dense rows (io.row_pitch = 0)")
    for io in (None, _io()):  # a summary without auto-reset, in either mode
        _refused(_call(_batch(flags=0), ant, _policy(ant), smp=None, io=io),
                 b"a summary needs CARL_FLAG_AUTORESET (without auto-reset a finished lane reports done on every later "
                 b"step, and its episode would be counted on each of them)", UNS)
    # then the sampling argument, in this order
    _refused(_call(_batch(), ant, _policy(ant), smp=None), b"sampling is NULL")
    _refused(_call(_batch(), ant, _policy(ant), smp=_smp(log_std=None, log_prob=0x8000)),
             b"sampling->log_std is NULL (one value per weight set and actuator)")
    _refused(_call(_batch(), ant, _policy(ant), smp=_smp(log_prob=0x8000), io=None),
             b"log_prob in summary mode (io NULL): a summary stores nothing per step")
    for steps, shown in ((0, b"0"), (-1, b"-1"), ((1 << 28) + 1, b"268435457")):
        _refused(_call(_batch(max_episode_steps=steps), ant, _policy(ant), io=_io()),
                 b"max_episode_steps " + shown + b" outside [1, 2^28]: the draws' counter holds the step count of an "
                 b"episode in 28 bits")
    # a model table with more actuators than the counter's two block bits hold
    wide = BP.build_model("ant")[0]
    wide.n_act = 9
    _refused(_call(_batch(), wide, _policy(wide), io=_io()),
             b"9 actuators: the draws' counter holds the Philox block in two bits (at most 8 actuators)")
    # nothing to do: valid, nothing enqueued -- in either mode, at the bound of max_episode_steps too
    assert _call(_batch(n=0), ant, _policy(ant)) == 0
    assert _call(_batch(n=0, max_episode_steps=1 << 28), ant, _policy(ant), smp=_smp(log_prob=0x8000), io=_io()) == 0
    _refused(_call(_batch(n=0), ant, _policy(ant), smp=None), b"sampling is NULL")


def test_the_unit_is_one_expansion_of_the_instance_list_with_its_own_kernel():
    src = U.source("carl_brax_policy_sample.hip", comments=False)
    table = re.search(r"#define X\(M, K, T, P\) \{\{M, T, P, false\}, K, carl::brax::(\w+)<M, K, T, P>\},\n"
                      r"const [\w:<>]+ \w+\[\] = \{\s*CARL_BRAX_CLOSED_LOOP_INSTANCES\(X\)\};\n#undef X\n", src)
    assert table is not None and table.group(1) == "brax_policy_sampled_kernel"
    rest = src.replace(table.group(0), "")
    assert "CARL_BRAX_CLOSED_LOOP_INSTANCES" not in rest
    assert not re.search(r"brax_\w*_kernel\s*<", rest)
    assert not re.search(r"\((true|false), \d+, (true|false), (true|false)\)", rest)
    assert "launch_closed_loop(kBraxSampledKernels" in rest
    # log_prob == NULL is a runtime branch: one kernel template, and no other unit instantiates the sampled variant
    hdr = U.source("brax_sample_kernels.hip.h", comments=False)
    assert len(re.findall(r"__global__", hdr)) == 1 and "brax_policy_sampled_kernel(" in hdr
    for unit in ("carl_brax.hip", "carl_brax_policy.hip", "carl_brax_episodes.hip", "carl_brax_policy_stats.hip"):
        other = U.source(unit)
        assert "brax_policy_sampled_kernel" not in other and "BraxSampledPolicy" not in other, unit
        assert "brax_sample_kernels.hip.h" not in other, unit
    from carl_amd.build import SOURCES

    assert SOURCES["carl_brax_policy_sample.hip"] == SOURCES["carl_brax_policy.hip"]


@pytest.mark.parametrize("actuator", range(8))
def test_counter_and_word_selection_against_the_oracle(actuator):
    """blocks 0 .. 3, even and odd actuators: the helper's vectorised draw is oracle.philox4x32_10 on the counter the
    header spells out"""
    seed = 0x0123456789ABCDEF
    rng = np.random.default_rng(actuator)
    genv = np.concatenate([[0, 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 12345], rng.integers(0, 1 << 48, 11)]).astype(np.uint64)
    e = np.concatenate([[0, 1, (1 << 32) - 1], rng.integers(0, 1 << 32, 13)]).astype(np.uint64)
    el = np.concatenate([[0, 1, (1 << 28) - 1], rng.integers(0, 1 << 28, 13)]).astype(np.uint64)
    wa, wb = BS.actuator_words(seed, genv, e, el, actuator)
    c = BS.counter(genv, e, el, actuator)
    block = actuator >> 1
    for i in range(genv.size):
        tag = 0x40000000 | (block << 28) | int(el[i])
        assert [int(v[i]) if np.ndim(v) else int(v) for v in c] == [int(genv[i]) & 0xFFFFFFFF, int(genv[i]) >> 32,
                                                                    int(e[i]), tag]
        assert tag >> 30 == 1  # the block never reaches the tag's bits: neither the reset draws' 0x8... nor plain counters
        w = O.philox4x32_10([int(genv[i]) & 0xFFFFFFFF, int(genv[i]) >> 32, int(e[i]), tag],
                            [seed & 0xFFFFFFFF, seed >> 32])
        assert (int(wa[i]), int(wb[i])) == ((int(w[2]), int(w[3])) if actuator & 1 else (int(w[0]), int(w[1])))
    z = BS.draws64(seed, genv, e, el, 8)
    u1 = ((wa >> 8).astype(np.float64) + 1) * 2.0 ** -24
    np.testing.assert_array_equal(z[:, actuator], np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * (wb >> 8) * 2.0 ** -24))


def test_log_std_shapes():
    rng = np.random.default_rng(0)
    assert U.ant_policy(rng).log_std.shape == (1, 8) and not U.ant_policy(rng).log_std.any()
    layers = BP.make_layers(rng, 27, (8,), 8)
    p = BraxMLPPolicy(U.info(27, 8), [], layers, "relu", log_std=-0.5)  # a scalar is every actuator's
    assert p.log_std.dtype == np.float32 and p.log_std.shape == (1, 8) and (p.log_std == np.float32(-0.5)).all()
    row = np.linspace(-1, 1, 8)
    q = BraxMLPPolicy(U.info(27, 8), [], layers, "relu", log_std=row)
    np.testing.assert_array_equal(q.log_std, row.astype(np.float32)[None])
    import torch

    np.testing.assert_array_equal(BraxMLPPolicy(U.info(27, 8), [], layers, "relu", log_std=torch.tensor(row)).log_std, q.log_std)
    st = BraxMLPPolicy.stack([p, q, p], 256)
    assert st.log_std.shape == (3, 8) and st.n_sets == 3
    np.testing.assert_array_equal(st.log_std, np.concatenate([p.log_std, q.log_std, p.log_std]))
    assert st.device_log_std("cpu").shape == (3, 8) and st.device_log_std("cpu").dtype == torch.float32
    for bad in (np.zeros(7), np.zeros(9), np.zeros((2, 8)), []):
        with pytest.raises(ValueError, match="log_std"):
            BraxMLPPolicy(U.info(27, 8), [], layers, "relu", log_std=bad)
    for fn in (BraxMLPPolicy.__init__, BraxMLPPolicy.for_env):
        assert inspect.signature(fn).parameters["log_std"].default is None
    # unpack keeps refusing a log_std; what it builds carries the default
    with pytest.raises(NotImplementedError, match="log_std"):
        BraxMLPPolicy.unpack(p, p.params[0], log_std=0.0)
    assert BraxMLPPolicy.unpack(q, q.params[0]).log_std.shape == (1, 8)


def test_launch_shape_does_not_know_whether_a_launch_samples():
    """one shape rule and the same instances for both entry points: the query takes no sampling argument, and the unit's
    table is the list the deterministic unit expands (above); so a sampled launch of a batch has the deterministic shape"""
    fn = _lib.load().carl_brax_policy_launch_shape
    assert len(_lib.EXPORTS["carl_brax_policy_launch_shape"][1]) == 5
    assert _lib.EXPORTS["carl_brax_rollout_policy_sampled"][1][5]._type_ is _lib.PolicySampling
    s = BP.build_model("ant")[0]
    for n, T in ((300, 8), (32768, 100)):
        code, sh = BP.launch_shape(_batch(n), s, _policy(s), T)
        assert code == 0 and fn is not None
        # LDS per env is MODE 2's: the open-loop slice plus the policy's rows, nothing for the sampling
        code, op = BP.open_launch_shape(_batch(n), s, 1, T)
        assert code == 0 and op.lanes_per_env == sh.lanes_per_env
        envs = 64 // sh.lanes_per_env
        per_wave = (sh.lds_bytes // sh.waves_per_workgroup) - (op.lds_bytes // op.waves_per_workgroup)
        assert per_wave == 164 * 4 * envs  # 32 + 64 + 64 + 4 policy rows
    assert "brax_sample_kernels" not in U.source("brax_launch.hpp") and "kSampled" not in U.source("brax_launch.hpp")


def test_python_keyword_rules_before_any_launch():
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.engine import LaneEngine, VecEngine
    from carl_amd.envs.brax.carl_brax_env import CARLBraxEnv

    for fn in (BraxVecEngine.rollout_policy, CARLBraxEnv.rollout_policy):
        par = inspect.signature(fn).parameters
        ref = inspect.signature(VecEngine.rollout_policy).parameters
        for k in ("deterministic", "sample_seed", "log_prob"):
            assert par[k].kind is inspect.Parameter.KEYWORD_ONLY and par[k].default == ref[k].default, k
    eng = U.fake_brax_engine()
    pol = U.ant_policy(np.random.default_rng(1))
    with pytest.raises(ValueError, match="log_prob=True: sampled launches only"):
        eng.rollout_policy(pol, 4, log_prob=True)
    with pytest.raises(ValueError, match="log_prob=True: transitions mode only"):
        eng.rollout_policy(pol, 4, mode="summary", deterministic=False, log_prob=True)
    # gae is the lane engine's: one body for the classic and the Brax engine
    assert "gae" in LaneEngine.__dict__ and "gae" not in VecEngine.__dict__ and "gae" not in BraxVecEngine.__dict__
    assert BraxVecEngine.gae is LaneEngine.gae and VecEngine.gae is LaneEngine.gae


def test_reference_draws_of_the_independence_case_are_inside_their_bounds():
    """the float64 draws the GPU test pools (Ant x 300 envs, 8 steps, 8 actuators, BS.SEED; here under the nominal
    counters of a TimeLimit of 3 from a fresh reset: e = t // 3, elapsed = t % 3) meet the four 5-sigma bounds"""
    t = np.arange(8)[:, None] + np.zeros((1, 300), np.int64)
    z = BS.draws64(BS.SEED, np.arange(300)[None] + 0 * t, t // 3, t % 3, 8)
    assert z.shape == (8, 300, 8) and z.size == 300 * 8 * 8
    stats = BS.assert_independent(z)
    print("mean %.4f var %.4f pair corr %.4f env corr %.4f" % stats)
    # and a dependent stream is caught: every actuator pair sharing one draw
    zz = z.copy()
    zz[:, :, 1::2] = zz[:, :, 0::2]
    with pytest.raises(AssertionError):
        BS.assert_independent(zz)
