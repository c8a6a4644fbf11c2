"""Sampled closed-loop rollout, host side: the carl_policy_sampling_t layout, every new refusal of
carl_rollout_policy_sampled / carl_evaluate_policy_sampled and of the Python layer, log_std through the constructors and
stack(), and the host reference of the sampling rule (sampling_ref.py) against oracle.philox4x32_10 and
torch.distributions.  CPU-only: nothing here launches a kernel (the C entry points refuse before they would enqueue)."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import sampling_ref as SR
from carl_amd import _lib
from carl_amd.policy import MLPPolicy
from oracle import oracle as O
from policy_cases import (HEADER, SAMPLING_LOG_PROB_REFUSED, SAMPLING_LOG_PROB_UNALIGNED, SAMPLING_LOG_STD,
                          SAMPLING_NULL, c_batch, c_io, c_policy, check_first_of_two, fake_engine, rand_layers)


def test_sampling_struct_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    fs = [f[0] for f in _lib.PolicySampling._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("%zu\\n", sizeof(carl_policy_sampling_t));']
    lines += [f'printf("%zu\\n", offsetof(carl_policy_sampling_t, {f}));' for f in fs]
    lines += ["return 0;}"]
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [C.sizeof(_lib.PolicySampling)] + [getattr(_lib.PolicySampling, f).offset for f in fs]


def _io():
    io = _lib.StepIO()
    io.action, io.obs, io.reward, io.terminated, io.truncated = 0x1000, 0x1000, 0x1000, 0x1000, 0x1000
    io.action_dtype = _lib.ACTION_I32
    return io


def _episodes():
    return _lib.PolicyEpisodes(0x3000, 0x3000, 0x3000, 0x3000, 0x3000, 0x3000)


def _flags(b):
    b.flags = _lib.FLAG_AUTORESET
    return b


def test_sampled_entry_points_refuse_what_their_twins_refuse():
    """the deterministic twin's checks come first, same codes, messages naming the sampled entry point"""
    lib = _lib.load()
    smp = _lib.PolicySampling(1, None, None)
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    b, p = _flags(c_batch()), c_policy(width=(65, 64))
    assert lib.carl_rollout_policy_sampled(C.byref(b), C.byref(p), C.byref(smp), None, 10, C.byref(summ), None) == -1
    assert b"carl_rollout_policy_sampled: hidden width[0] = 65" in lib.carl_last_error()
    assert lib.carl_evaluate_policy_sampled(C.byref(b), C.byref(p), C.byref(smp), 2, 10, C.byref(_episodes()), None) == -1
    assert b"carl_evaluate_policy_sampled: hidden width[0] = 65" in lib.carl_last_error()
    # the batch checks (Brax family), io layout, summary without auto-reset
    bb = c_batch(family=_lib.CARL_N_FAMILIES)
    assert lib.carl_rollout_policy_sampled(C.byref(bb), C.byref(c_policy()), C.byref(smp), None, 10, C.byref(summ),
                                           None) == -1
    assert b"Brax family" in lib.carl_last_error()
    io = _io()
    io.row_pitch = 1004
    assert lib.carl_rollout_policy_sampled(C.byref(b), C.byref(c_policy()), C.byref(smp), C.byref(io), 10, None,
                                           None) == _lib.ERR_UNSUPPORTED
    assert lib.carl_rollout_policy_sampled(C.byref(c_batch()), C.byref(c_policy()), C.byref(smp), None, 10, C.byref(summ),
                                           None) == _lib.ERR_UNSUPPORTED
    assert lib.carl_evaluate_policy_sampled(C.byref(b), C.byref(c_policy()), C.byref(smp), 0, 10, C.byref(_episodes()),
                                            None) == -1
    assert b"n_episodes 0 < 1" in lib.carl_last_error()


def test_sampled_entry_points_refuse_bad_sampling():
    lib = _lib.load()
    b, p = _flags(c_batch()), c_policy()
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    for fn, args in ((lib.carl_rollout_policy_sampled, lambda s: (C.byref(b), C.byref(p), s, None, 10, C.byref(summ), None)),
                     (lib.carl_evaluate_policy_sampled, lambda s: (C.byref(b), C.byref(p), s, 2, 10, C.byref(_episodes()),
                                                                   None))):
        assert fn(*args(None)) == _lib.ERR_INVALID_ARGUMENT
        assert b"sampling is NULL" in lib.carl_last_error()
        assert fn(*args(C.byref(_lib.PolicySampling(1, None, 0x4000)))) == _lib.ERR_INVALID_ARGUMENT  # summary / episodes
        assert b"log_prob" in lib.carl_last_error()
    # a Box family without log_std
    bp = _flags(c_batch(family=_lib.PENDULUM))
    pp = c_policy(n_in=5, n_out=1, head=_lib.POLICY_HEAD_BOX)
    assert lib.carl_rollout_policy_sampled(C.byref(bp), C.byref(pp), C.byref(_lib.PolicySampling(1, None, None)), None, 10,
                                           C.byref(summ), None) == _lib.ERR_INVALID_ARGUMENT
    assert b"log_std" in lib.carl_last_error()
    assert lib.carl_evaluate_policy_sampled(C.byref(bp), C.byref(pp), C.byref(_lib.PolicySampling(1, None, None)), 2, 10,
                                            C.byref(_episodes()), None) == _lib.ERR_INVALID_ARGUMENT
    assert b"log_std" in lib.carl_last_error()
    # transitions mode takes a log_prob, on a 16-byte boundary
    io = _io()
    assert lib.carl_rollout_policy_sampled(C.byref(b), C.byref(p), C.byref(_lib.PolicySampling(1, None, 0x4004)),
                                           C.byref(io), 10, None, None) == _lib.ERR_UNSUPPORTED
    assert b"16-byte" in lib.carl_last_error()


def test_sampled_entry_points_word_the_sampling_checks_alike_and_in_one_order():
    """the whole message of every sampling check under both entry points' names, and which of two spoilt fields answers:
    sampling NULL, then log_std, then a log_prob where none is stored, then its alignment"""
    lib = _lib.load()
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    bp, pp = _flags(c_batch(family=_lib.PENDULUM)), c_policy(n_in=5, n_out=1, head=_lib.POLICY_HEAD_BOX)
    bd, pd = _flags(c_batch()), c_policy()
    io_f = c_io(action_dtype=_lib.ACTION_F32)

    def rollout(b, p, smp, io=None):
        return lib.carl_rollout_policy_sampled(C.byref(b), C.byref(p), None if smp is None else C.byref(smp),
                                               None if io is None else C.byref(io), 10, None if io else C.byref(summ), None)

    def evaluate(b, p, smp, io=None):
        return lib.carl_evaluate_policy_sampled(C.byref(b), C.byref(p), None if smp is None else C.byref(smp), 2, 10,
                                                C.byref(_episodes()), None)

    S = _lib.PolicySampling
    for who, fn in ((b"carl_rollout_policy_sampled: ", rollout), (b"carl_evaluate_policy_sampled: ", evaluate)):
        for b, p, smp, code, msg in [
                (bp, pp, None, -1, SAMPLING_NULL),
                (bp, pp, S(1, None, None), -1, SAMPLING_LOG_STD),
                (bp, pp, S(1, None, 0x4004), -1, SAMPLING_LOG_STD),  # log_std before either log_prob check
                (bp, pp, S(1, 0x6000, 0x4004), -1, SAMPLING_LOG_PROB_REFUSED),  # a column refused before its alignment
                (bd, pd, S(1, None, 0x4000), -1, SAMPLING_LOG_PROB_REFUSED)]:
            assert fn(b, p, smp) == code
            assert lib.carl_last_error() == who + msg
    # transitions mode stores the column: log_std first, then the alignment
    who = b"carl_rollout_policy_sampled: "
    assert rollout(bp, pp, S(1, None, 0x4004), io_f) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == who + SAMPLING_LOG_STD
    assert rollout(bp, pp, S(1, 0x6000, 0x4004), io_f) == _lib.ERR_UNSUPPORTED
    assert lib.carl_last_error() == who + SAMPLING_LOG_PROB_UNALIGNED
    assert rollout(bd, pd, S(1, None, 0x4008), c_io()) == _lib.ERR_UNSUPPORTED
    assert lib.carl_last_error() == who + SAMPLING_LOG_PROB_UNALIGNED
    # the deterministic twin's checks answer before any sampling check (sampling NULL, or a misaligned log_prob)
    for smp in (None, S(1, None, 0x4004)):
        check_first_of_two(b"carl_rollout_policy_sampled", lambda b, p: rollout(b, p, smp))
        check_first_of_two(b"carl_evaluate_policy_sampled", lambda b, p: evaluate(b, p, smp))
    assert rollout(bd, pd, None, c_io(row_pitch=999)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == who + b"io.row_pitch 999 < n_lanes 1000"
    assert lib.carl_evaluate_policy_sampled(C.byref(bd), C.byref(pd), None, 0, 10, C.byref(_episodes()), None) == -1
    assert lib.carl_last_error() == b"carl_evaluate_policy_sampled: n_episodes 0 < 1"


def test_python_refusals():
    from carl_amd.engine import VecEngine
    from carl_amd.mixed import MixedVecEngine

    eng = fake_engine(_lib.PENDULUM)
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="Box families only"):
        cp = fake_engine()
        MLPPolicy.for_env(cp, rand_layers(rng, [cp.F + cp.D, 2]), log_std=0.5)
    with pytest.raises(ValueError, match="one value"):
        MLPPolicy.for_env(eng, rand_layers(rng, [eng.F + 3, 1]), log_std=[0.1, 0.2])
    pol = MLPPolicy.for_env(eng, rand_layers(rng, [eng.F + 3, 1]), log_std=torch.tensor([-0.5]))
    assert pol.log_std.dtype == np.float32 and pol.log_std.tolist() == [-0.5]
    # a launch's refusals before anything reaches the C ABI
    class Eng:  # what rollout_policy reads before its launch
        _policy_rollout, family, D, n, device, auto_reset = True, eng.family, eng.D, 1000, torch.device("cpu"), True

    with pytest.raises(ValueError, match="log_prob=True: sampled launches only"):
        VecEngine.rollout_policy(Eng(), pol, 8, log_prob=True)
    with pytest.raises(ValueError, match="transitions mode only"):
        VecEngine.rollout_policy(Eng(), pol, 8, mode="summary", deterministic=False, log_prob=True)
    with pytest.raises(NotImplementedError, match="pair launch"):
        MixedVecEngine.rollout_policy(object.__new__(MixedVecEngine), pol, 8, deterministic=False)
    with pytest.raises(NotImplementedError, match="pair launch"):
        MixedVecEngine.evaluate_policy(object.__new__(MixedVecEngine), pol, 2, 8, deterministic=False)


def test_stack_carries_log_std():
    eng = fake_engine(_lib.MOUNTAINCAR_CONT)
    rng = np.random.default_rng(1)
    pols = [MLPPolicy.for_env(eng, rand_layers(rng, [eng.F + eng.D, 8, 1]), log_std=v) for v in (-1.0, 0.25, 0.0)]
    s = MLPPolicy.stack(pols, 512)
    np.testing.assert_array_equal(s.log_std, np.float32([-1.0, 0.25, 0.0]))
    assert s.n_sets == 3
    assert MLPPolicy.for_env(eng, rand_layers(rng, [eng.F + eng.D, 1])).log_std.tolist() == [0.0]


def test_host_philox_matches_the_oracle():
    rng = np.random.default_rng(2)
    for _ in range(20):
        ctr = rng.integers(0, 2**32, 4, dtype=np.uint64)
        key = rng.integers(0, 2**32, 2, dtype=np.uint64)
        got = SR.philox(*ctr, int(key[0]), int(key[1]))
        np.testing.assert_array_equal(np.array([int(g) for g in got], np.uint32), O.philox4x32_10(ctr, key))
    seed, glane, e, el = 0x123456789ABCDEF0, 70000, 5, 17
    w = SR.sample_words(seed, np.array([glane]), np.array([e]), np.array([el]))
    want = O.philox4x32_10([glane & 0xFFFFFFFF, glane >> 32, e, 0x80000000 | el], [seed & 0xFFFFFFFF, seed >> 32])
    np.testing.assert_array_equal(np.array([int(v[0]) for v in w], np.uint32), want)


def test_host_rule_agrees_with_torch_distributions():
    """inverse-CDF categorical and Box-Muller z: the frequencies / moments of torch's distributions, and log-probs equal"""
    rng = np.random.default_rng(3)
    n = 400_000
    w = [rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    y = np.array([[0.3, -1.2, 1.1]])
    a, _ = SR.categorical64(np.repeat(y, n, 0), SR.u_categorical(w[0]).astype(np.float64))
    p = torch.distributions.Categorical(logits=torch.tensor(y[0])).probs.numpy()
    freq = np.bincount(a, minlength=3) / n
    assert np.all(np.abs(freq - p) < 5 * np.sqrt(p * (1 - p) / n)), (freq, p)
    lp = torch.distributions.Categorical(logits=torch.tensor(y[0])).log_prob(torch.tensor(a[:5])).numpy()
    np.testing.assert_allclose(lp, (y[0] - y.max())[a[:5]] - np.log(np.exp(y[0] - y.max()).sum()), rtol=1e-12)
    z = SR.z_gaussian64(w[0], w[1])
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    mu, ls = 0.7, -0.4
    a = mu + np.exp(ls) * z[:5]
    lp = torch.distributions.Normal(torch.tensor(mu, dtype=torch.float64), torch.tensor(np.exp(ls))).log_prob(torch.tensor(a)).numpy()
    np.testing.assert_allclose(lp, -z[:5] ** 2 / 2 - ls - 0.5 * np.log(2 * np.pi), rtol=1e-12, atol=1e-12)
    # equal logits: the fp32 mirror is the float64 rule wherever t is not on a boundary
    u = SR.u_categorical(w[0][:1000])
    a32 = SR.categorical_equal_logits(u, 3)
    a64, margin = SR.categorical64(np.zeros((1000, 3)), u.astype(np.float64))
    assert np.array_equal(a32[margin > 1e-6], a64[margin > 1e-6])


def test_sample_words_take_the_lane_offset():
    """glane = lane_offset + lane, split into the counter's lo and hi words (hi non-zero past 2^32)"""
    seed, L = 0x0123456789ABCDEF, 5_000_000_000
    lanes, e, el = np.array([0, 1, 4111]), np.array([0, 3, 7]), np.array([0, 11, 499])
    got = SR.sample_words(seed, lanes, e, el, lane_offset=L)
    for j in range(lanes.size):
        g = L + int(lanes[j])
        want = O.philox4x32_10([g & 0xFFFFFFFF, g >> 32, int(e[j]), 0x80000000 | int(el[j])],
                               [seed & 0xFFFFFFFF, seed >> 32])
        np.testing.assert_array_equal(np.array([int(v[j]) for v in got], np.uint32), want)
    same = SR.sample_words(seed, np.uint64(L) + lanes.astype(np.uint64), e, el)
    assert all(np.array_equal(a, b) for a, b in zip(got, same))
    lo = SR.sample_words(seed, lanes, e, el, lane_offset=L & 0xFFFFFFFF)  # the hi word matters
    assert not any(np.array_equal(a, b) for a, b in zip(got, lo))


def test_log_prob_references_agree_with_torch():
    rng = np.random.default_rng(4)
    y = rng.normal(0, 1, (2000, 3)) * rng.choice([0.1, 1.0, 30.0, 90.0], (2000, 1))  # gaps up to ~300: exp underflows
    a = rng.integers(0, 3, 2000)
    want = torch.distributions.Categorical(logits=torch.tensor(y)).log_prob(torch.tensor(a)).numpy()
    np.testing.assert_allclose(SR.categorical_log_prob64(y, a), want, rtol=1e-12, atol=1e-12)
    z = rng.normal(0, 1.5, 2000)
    for ls in (-20.0, -0.5, 0.0, 2.0):
        ls32 = np.float32(ls)
        sigma = np.exp(np.float64(ls32))
        want = torch.distributions.Normal(torch.tensor(0.3, dtype=torch.float64), torch.tensor(sigma)).log_prob(
            torch.tensor(0.3 + sigma * z)).numpy()
        np.testing.assert_allclose(SR.gaussian_log_prob64(z, ls32), want, rtol=1e-9, atol=1e-9 if ls > -1 else 1e-6)


def _categorical_fp32(y32, u):
    """the device's categorical rule and log_prob in fp32 (include/carl_amd.h), one lane-step per row"""
    f = np.float32
    m = y32.max(axis=1)
    s = np.zeros(len(y32), f)
    c = np.empty_like(y32)
    for k in range(y32.shape[1]):
        s = (s + np.exp((y32[:, k] - m).astype(f)).astype(f)).astype(f)
        c[:, k] = s
    t = (u.astype(f) * s).astype(f)
    a = np.full(len(y32), y32.shape[1] - 1)
    for k in range(y32.shape[1] - 2, -1, -1):
        a = np.where(t < c[:, k], k, a)
    ya = y32[np.arange(len(y32)), a]
    return a, ((ya - m).astype(f) - np.log(s).astype(f)).astype(f)


def test_fp32_mirrors_stay_within_the_bounds():
    """an fp32 evaluation from outputs within the forward bound of y64 meets categorical_tolerance /
    categorical_log_prob_bound, and one of the Gaussian rule meets gaussian_log_prob_bound: the bounds are not tighter
    than fp32 arithmetic allows"""
    rng = np.random.default_rng(5)
    N = 200_000
    for na in (2, 3):
        y64 = rng.normal(0, 1, (N, na)) * rng.choice([0.3, 3.0, 30.0, 90.0], (N, 1))
        bound = np.abs(y64) * 2.0 ** -20 + 1e-7  # a forward pass's bound
        y32 = (y64 + rng.uniform(-0.9, 0.9, y64.shape) * bound).astype(np.float32)
        w = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
        u = SR.u_categorical(w)
        a32, lp32 = _categorical_fp32(y32, u)
        a64, margin = SR.categorical64(y64, u.astype(np.float64))
        clear = margin > SR.categorical_tolerance(y64, bound)
        assert (~clear).mean() < 1e-3
        np.testing.assert_array_equal(a32[clear], a64[clear])
        err = np.abs(lp32 - SR.categorical_log_prob64(y64, a32))
        assert np.all(err <= SR.categorical_log_prob_bound(y64, bound, a32)), err.max()
    wx, wy = (rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    z64 = SR.z_gaussian64(wx, wy)
    f = np.float32
    u1 = (((wx >> 8) + 1).astype(f) * f(2.0 ** -24)).astype(f)
    u2 = ((wy >> 8).astype(f) * f(2.0 ** -24)).astype(f)
    z32 = (np.sqrt(f(-2) * np.log(u1)).astype(f) * np.cos(np.float64(2 * u2) * np.pi).astype(f)).astype(f)
    assert np.all(np.abs(z32 - z64) <= SR.gaussian_z_bound(z64))
    for ls in (-20.0, -0.5, 0.0, 2.0):
        lp0 = f(-f(ls) - f(0.918938533204672742))
        lp32 = (np.float64(f(-0.5) * z32) * np.float64(z32) + np.float64(lp0)).astype(f)  # one fma: round once
        err = np.abs(lp32 - SR.gaussian_log_prob64(z64, f(ls)))
        assert np.all(err <= SR.gaussian_log_prob_bound(z64, f(ls))), err.max()
