"""Input statistics, C ABI on the host: the layouts of carl_policy_stats_t / carl_policy_running_stats_t, the exported
symbols, and every refusal of carl_evaluate_policy_stats / carl_policy_stats_merge (validated before anything is
enqueued, so they run without a GPU), plus the engines that refuse the keyword.  CPU-only."""
import ctypes as C
import subprocess

import pytest

from carl_amd import _lib
from policy_cases import (HEADER, REFUSALS, SAMPLING_LOG_PROB_REFUSED, SAMPLING_LOG_STD,
                          c_batch, c_policy, check_first_of_two)

PTR = 0x10000  # a 16-byte-aligned "device pointer" that is never dereferenced: every call here is refused first


@pytest.mark.parametrize("cname, struct", [("carl_policy_stats_t", _lib.PolicyStats),
                                           ("carl_policy_running_stats_t", _lib.PolicyRunningStats)])
def test_struct_layouts_match_c(tmp_path, cname, struct):
    prog = tmp_path / "layout.c"
    fs = [f[0] for f in struct._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             f'printf("%zu\\n", sizeof({cname}));']
    lines += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fs]
    lines += ["return 0;}"]
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [C.sizeof(struct)] + [getattr(struct, f).offset for f in fs]


def test_symbols_and_abi_version():
    lib = _lib.load()
    for name in ("carl_policy_stats_workgroups", "carl_evaluate_policy_stats", "carl_policy_stats_merge"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.carl_abi_version() == 9 == _lib.CARL_ABI_VERSION
    q = lib.carl_policy_lane_quantum()
    assert [lib.carl_policy_stats_workgroups(n) for n in (-5, 0, 1, q, q + 1, 300, 65536)] == [0, 0, 1, 1, 2, 2, 65536 // q]


def _eps(**kw):
    e = _lib.PolicyEpisodes(*([0x5000] * 6))
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _stats(partial=PTR, capacity=4):
    return _lib.PolicyStats(partial, capacity)


def _call(b, p, smp=None, K=3, T=100, out="default", stats="default"):
    out = _eps() if out == "default" else out
    stats = _stats() if stats == "default" else stats
    return _lib.load().carl_evaluate_policy_stats(C.byref(b), C.byref(p), None if smp is None else C.byref(smp), K, T,
                                                  None if out is None else C.byref(out),
                                                  None if stats is None else C.byref(stats), None)


@pytest.mark.parametrize("case, batch_kw, pol_kw, msg", [
    ("width over the limit", {}, {"width": (65, 64)}, b"hidden width[0] = 65"),
    ("too many layers", {}, {"n_hidden": 3}, b"n_hidden 3"),
    ("discrete head width", {}, {"n_out": 3}, b"head width 3"),
    ("Brax family", {"family": _lib.CARL_N_FAMILIES}, {}, b"Brax family"),
    ("lanes_per_set not a multiple", {}, {"lanes_per_set": 300}, b"lanes_per_set 300"),
    ("sets do not cover", {}, {"lanes_per_set": 256, "n_sets": 3}, b"do not cover"),
    ("context row >= F", {}, {"ctx_rows": (0, 8)}, b"ctx_rows[1] = 8"),
    ("n_in mismatch", {}, {"n_in": 7}, b"n_in 7"),
    ("head kind", {}, {"head": _lib.POLICY_HEAD_BOX}, b"head kind"),
    ("activation", {}, {"activation": 7}, b"unknown activation"),
    ("no params", {}, {"params": None}, b"params is NULL"),
    ("no contexts", {"n_contexts": 0}, {}, b"n_contexts"),
])
def test_evaluate_stats_validates_what_evaluate_policy_validates(case, batch_kw, pol_kw, msg):
    """the same refusal, the same code, under this entry point's name -- and before the stats checks: stats is NULL here"""
    lib = _lib.load()
    b, p = c_batch(flags=_lib.FLAG_AUTORESET, **batch_kw), c_policy(**pol_kw)
    want = lib.carl_evaluate_policy(C.byref(b), C.byref(p), 3, 100, C.byref(_eps()), None)
    assert want == _lib.ERR_INVALID_ARGUMENT
    assert _call(b, p, stats=None) == want, case
    err = lib.carl_last_error()
    assert msg in err and err.startswith(b"carl_evaluate_policy_stats:"), (case, err)
    assert err == b"carl_evaluate_policy_stats: " + REFUSALS[case]


def test_evaluate_stats_reports_the_earlier_of_two_bad_arguments():
    """the batch / policy checks in their order before everything else (sampling, output struct, counts and stats spoilt
    too); then the sampling checks, whole and in their order, before the stats checks"""
    lib = _lib.load()
    who = b"carl_evaluate_policy_stats: "
    for smp in (None, _lib.PolicySampling(1, None, PTR + 4)):
        check_first_of_two(who[:-2], lambda b, p: _call(b, p, smp=smp, K=0, T=-1, out=None, stats=None))
    assert lib.carl_evaluate_policy_stats(None, C.byref(c_policy(params=None)), None, 0, -1, None, None, None) == -1
    assert lib.carl_last_error() == who + b"batch / policy is NULL"
    bp = c_batch(family=_lib.PENDULUM, flags=_lib.FLAG_AUTORESET)
    pp = c_policy(n_in=5, n_out=1, head=_lib.POLICY_HEAD_BOX)
    for smp, b, p, code, msg in [
            (_lib.PolicySampling(1, None, PTR + 4), bp, pp, _lib.ERR_INVALID_ARGUMENT, SAMPLING_LOG_STD),
            (_lib.PolicySampling(1, None, PTR), bp, pp, _lib.ERR_INVALID_ARGUMENT, SAMPLING_LOG_STD),
            (_lib.PolicySampling(1, PTR, PTR + 4), bp, pp, _lib.ERR_INVALID_ARGUMENT, SAMPLING_LOG_PROB_REFUSED),
            (_lib.PolicySampling(1, None, PTR + 4), c_batch(flags=_lib.FLAG_AUTORESET), c_policy(), _lib.ERR_INVALID_ARGUMENT,
             SAMPLING_LOG_PROB_REFUSED)]:
        assert _call(b, p, smp=smp, stats=None) == code
        assert lib.carl_last_error() == who + msg
    # the evaluate checks before the sampling checks
    assert _call(bp, pp, smp=_lib.PolicySampling(1, None, None), K=0, stats=None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == who + b"n_episodes 0 < 1"


def test_evaluate_stats_refusals_in_order():
    lib = _lib.load()
    b, p = c_batch(flags=_lib.FLAG_AUTORESET), c_policy()
    assert lib.carl_evaluate_policy_stats(None, C.byref(p), None, 1, 1, C.byref(_eps()), C.byref(_stats()), None) == -1
    assert lib.carl_evaluate_policy_stats(C.byref(b), None, None, 1, 1, C.byref(_eps()), C.byref(_stats()), None) == -1
    assert _call(b, p, out=None) == _lib.ERR_INVALID_ARGUMENT and b"six" in lib.carl_last_error()
    assert _call(b, p, out=_eps(steps=None)) == _lib.ERR_INVALID_ARGUMENT and b"six" in lib.carl_last_error()
    assert _call(b, p, K=0) == _lib.ERR_INVALID_ARGUMENT and b"n_episodes 0" in lib.carl_last_error()
    assert _call(b, p, T=-1) == _lib.ERR_INVALID_ARGUMENT and b"max_steps -1" in lib.carl_last_error()
    assert _call(c_batch(), p) == _lib.ERR_UNSUPPORTED and b"CARL_FLAG_AUTORESET" in lib.carl_last_error()
    # the sampling checks come before the stats checks (stats is NULL here): a log_prob column in episodes mode, and a
    # Box family without log_std
    assert _call(b, p, smp=_lib.PolicySampling(1, None, PTR), stats=None) == _lib.ERR_INVALID_ARGUMENT
    assert b"log_prob is a transitions-mode output" in lib.carl_last_error()
    bp = c_batch(family=_lib.PENDULUM, flags=_lib.FLAG_AUTORESET)
    pp = c_policy(n_in=5, n_out=1, head=_lib.POLICY_HEAD_BOX)
    assert _call(bp, pp, smp=_lib.PolicySampling(1, None, None), stats=None) == _lib.ERR_INVALID_ARGUMENT
    assert b"log_std" in lib.carl_last_error()
    # then the stats struct, deterministic and sampled alike
    for smp in (None, _lib.PolicySampling(1, None, None)):
        assert _call(b, p, smp=smp, stats=None) == _lib.ERR_INVALID_ARGUMENT
        assert b"carl_evaluate_policy_stats: stats / stats->partial is NULL" in lib.carl_last_error()
        assert _call(b, p, smp=smp, stats=_stats(partial=None)) == _lib.ERR_INVALID_ARGUMENT
        assert b"stats / stats->partial is NULL" in lib.carl_last_error()
        for off in (4, 8, 12):
            assert _call(b, p, smp=smp, stats=_stats(partial=PTR + off)) == _lib.ERR_INVALID_ARGUMENT
            assert b"not on a 16-byte boundary" in lib.carl_last_error()
        assert _call(b, p, smp=smp, stats=_stats(capacity=3)) == _lib.ERR_INVALID_ARGUMENT  # 1000 lanes: 4 workgroups
        assert b"partial_capacity 3 < 4 workgroups" in lib.carl_last_error()
    # n_lanes == 0: valid, nothing to do, nothing enqueued -- with no slab at all
    assert _call(c_batch(n=0, flags=_lib.FLAG_AUTORESET), p, stats=_stats(capacity=0)) == 0


def _running(**kw):
    r = _lib.PolicyRunningStats(PTR, PTR, PTR)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _merge(p="default", stats="default", n_wg=4, steps=PTR, n=1000, running="default", eps=1e-8, min_std=1e-6,
           out=PTR, n_write=1):
    p = c_policy() if p == "default" else p
    stats = _stats() if stats == "default" else stats
    running = _running() if running == "default" else running
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    return _lib.load().carl_policy_stats_merge(ref(p), ref(stats), n_wg, steps, n, ref(running), eps, min_std, out,
                                               n_write, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(p=None), b"policy is NULL"),
    (dict(p=c_policy(width=(65, 64))), b"shape is outside the limits"),
    (dict(p=c_policy(n_in=33)), b"shape is outside the limits"),
    (dict(p=c_policy(params=None)), b"params is NULL"),
    (dict(n_wg=-1), b"n_workgroups -1 < 0"),
    (dict(stats=None), b"stats / stats->partial is NULL"),
    (dict(stats=_stats(partial=None)), b"stats / stats->partial is NULL"),
    (dict(stats=_stats(partial=PTR + 8)), b"not on a 16-byte boundary"),
    (dict(n_wg=5), b"partial_capacity 4 < 5 workgroups"),
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
    assert err.startswith(b"carl_policy_stats_merge:") and msg in err, err


def test_out_of_scope_engines_refuse_the_keyword():
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.mixed import MixedVecEngine

    with pytest.raises(NotImplementedError):
        object.__new__(BraxVecEngine).evaluate_policy(None, 1, 1, input_stats=True)
    with pytest.raises(NotImplementedError):
        object.__new__(MixedVecEngine).evaluate_policy(None, 1, 1, input_stats=True)
