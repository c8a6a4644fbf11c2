"""The episodes mode of the closed-loop rollout on the host: the ctypes layout of carl_policy_episodes_t, every refusal
of carl_evaluate_policy before it would enqueue anything, the engines that refuse it, and episode_stats against a
float64 NumPy reduction of synthetic records.  CPU-only: nothing here launches a kernel."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from carl_amd import _lib
from carl_amd.policy import MLPPolicy, episode_stats
from policy_cases import HEADER, REFUSALS, c_batch, c_policy, check_first_of_two, fake_engine, rand_layers


def test_episodes_struct_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    fe = [f[0] for f in _lib.PolicyEpisodes._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("%zu\\n", sizeof(carl_policy_episodes_t));']
    lines += [f'printf("%zu\\n", offsetof(carl_policy_episodes_t, {f}));' for f in fe]
    lines += ["return 0;}"]
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [C.sizeof(_lib.PolicyEpisodes)] + [getattr(_lib.PolicyEpisodes, f).offset for f in fe]
    assert fe == ["episodes", "steps", "ret", "length", "context_id", "terminated"]


def _eps(**kw):
    e = _lib.PolicyEpisodes(*([0x5000] * 6))
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _call(b, p, K=3, T=100, out="default"):
    lib = _lib.load()
    out = _eps() if out == "default" else out
    return lib.carl_evaluate_policy(C.byref(b), C.byref(p), K, T, None if out is None else C.byref(out), None)


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
    ("context observation feature >= F", {"n_ctx_obs": 1, "ctx_obs": 0x4000, "ctx_obs_feat": (8,)}, {},
     b"ctx_obs_feat[0] = 8"),
    ("no contexts", {"n_contexts": 0}, {}, b"n_contexts"),
])
def test_c_entry_point_validates_batch_and_policy(case, batch_kw, pol_kw, msg):
    """the checks and messages of carl_rollout_policy, under this entry point's name"""
    b, p = c_batch(flags=_lib.FLAG_AUTORESET, **batch_kw), c_policy(**pol_kw)
    assert _call(b, p) == _lib.ERR_INVALID_ARGUMENT, case
    err = _lib.load().carl_last_error()
    assert msg in err and err.startswith(b"carl_evaluate_policy"), (case, err)
    assert err == b"carl_evaluate_policy: " + REFUSALS[case]


def test_c_entry_point_reports_the_earlier_of_two_bad_arguments():
    """the batch / policy checks in their order, and all of them before the output struct and the counts"""
    lib = _lib.load()
    for out in (None, _eps(steps=None)):
        check_first_of_two(b"carl_evaluate_policy", lambda b, p: _call(b, p, K=0, T=-1, out=out))
    assert lib.carl_evaluate_policy(None, C.byref(c_policy(params=None)), 0, -1, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == b"carl_evaluate_policy: batch / policy is NULL"
    assert lib.carl_evaluate_policy(C.byref(c_batch(family=_lib.CARL_N_FAMILIES)), None, 0, -1, None, None) == -1
    assert lib.carl_last_error() == b"carl_evaluate_policy: batch / policy is NULL"
    # past the shared checks: the output struct before the counts, the counts before the auto-reset flag
    assert _call(c_batch(), c_policy(), K=0, out=None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == b"carl_evaluate_policy: out and all six of its arrays are required"
    assert _call(c_batch(), c_policy(), K=0, T=-1) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == b"carl_evaluate_policy: n_episodes 0 < 1"


@pytest.mark.parametrize("field", ["episodes", "steps", "ret", "length", "context_id", "terminated"])
def test_c_entry_point_needs_every_output_array(field):
    b, p = c_batch(flags=_lib.FLAG_AUTORESET), c_policy()
    assert _call(b, p, out=_eps(**{field: None})) == _lib.ERR_INVALID_ARGUMENT
    assert b"six" in _lib.load().carl_last_error()


def test_c_entry_point_refuses_bad_counts_and_no_auto_reset():
    lib = _lib.load()
    b, p = c_batch(flags=_lib.FLAG_AUTORESET), c_policy()
    assert lib.carl_evaluate_policy(None, C.byref(p), 1, 1, C.byref(_eps()), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_evaluate_policy(C.byref(b), None, 1, 1, C.byref(_eps()), None) == _lib.ERR_INVALID_ARGUMENT
    assert _call(b, p, out=None) == _lib.ERR_INVALID_ARGUMENT
    assert _call(b, p, K=0) == _lib.ERR_INVALID_ARGUMENT and b"n_episodes 0" in lib.carl_last_error()
    assert _call(b, p, K=-2) == _lib.ERR_INVALID_ARGUMENT
    assert _call(b, p, T=-1) == _lib.ERR_INVALID_ARGUMENT and b"max_steps -1" in lib.carl_last_error()
    big = c_batch(n=1 << 20, flags=_lib.FLAG_AUTORESET)
    assert _call(big, c_policy(lanes_per_set=1 << 20), K=2048) == _lib.ERR_INVALID_ARGUMENT  # 2^31 records
    assert b"2^31" in lib.carl_last_error()
    assert _call(c_batch(), p) == _lib.ERR_UNSUPPORTED  # no CARL_FLAG_AUTORESET
    assert b"CARL_FLAG_AUTORESET" in lib.carl_last_error()
    # n_lanes == 0: valid, nothing to do, nothing enqueued
    assert _call(c_batch(n=0, flags=_lib.FLAG_AUTORESET), p) == 0


def test_out_of_scope_engines_refuse():
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.mixed import MixedVecEngine

    with pytest.raises(NotImplementedError):
        object.__new__(BraxVecEngine).evaluate_policy(None, 1, 1)
    with pytest.raises(NotImplementedError):
        object.__new__(MixedVecEngine).evaluate_policy(None, 1, 1)


def test_python_refuses_bad_output_buffers_in_their_order():
    """the whole messages of evaluate_policy's own refusals on an engine that is never launched, and which of two answers"""
    rng = np.random.default_rng(0)
    eng = fake_engine()
    eng.device, eng.b = torch.device("cpu"), c_batch(flags=_lib.FLAG_AUTORESET)
    pol = MLPPolicy.for_env(eng, rand_layers(rng, [eng.F + eng.D, 8, 2]))
    other = fake_engine(_lib.MOUNTAINCAR)
    stranger = MLPPolicy.for_env(other, rand_layers(rng, [other.F + other.D, 3]))
    K, n = 2, eng.n

    def out(**kw):
        o = {k: torch.empty((K, n) if rows else (n,), dtype=dt) for k, dt, rows in eng._EPISODE_KEYS}
        o.update(kw)
        return o

    bad_first = torch.empty(n, dtype=torch.int64)
    for args, kw, msg in [
            ((stranger, 0, -1), {}, f"the policy was built for family {_lib.MOUNTAINCAR}, this engine runs family {_lib.CARTPOLE}"),
            ((pol, 0, -1), {}, "n_episodes 0 < 1"),
            ((pol, K, -1), {"out": out(episodes=bad_first)}, "max_steps -1 < 0"),
            ((pol, K, 5), {"out": out(episodes=bad_first, length=torch.empty((K, n)))},
             f"evaluate_policy output 'episodes' must be a contiguous torch.int32 [{n}] tensor on cpu"),
            ((pol, K, 5), {"out": out(length=torch.empty((K, n), dtype=torch.int32).t().contiguous().t(),
                                      terminated=torch.empty((K, n), dtype=torch.bool))},
             f"evaluate_policy output 'length' must be a contiguous torch.int32 [{K}, {n}] tensor on cpu"),
            ((pol, K, 5), {"out": out(terminated=torch.empty((K + 1, n), dtype=torch.uint8))},
             f"evaluate_policy output 'terminated' must be a contiguous torch.uint8 [{K}, {n}] tensor on cpu")]:
        with pytest.raises(ValueError) as e:
            eng.evaluate_policy(*args, **kw)
        assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        eng.rollout_policy(stranger, 4, gae=(0.9, 0.9))  # (gae without value_net: refused after the family)
    assert str(e.value) == f"the policy was built for family {_lib.MOUNTAINCAR}, this engine runs family {_lib.CARTPOLE}"


# ---------------------------------------------------------------- episode_stats
def synthetic(rng, K, n, n_ctx, empty=()):
    """evaluate_policy-shaped records: each lane's first episodes[lane] slots real, the rest sentinels"""
    episodes = rng.integers(0, K + 1, n).astype(np.int32)
    ctx_pool = np.array([c for c in range(n_ctx) if c not in empty])
    res = {"episodes": episodes, "steps": rng.integers(0, 1000, n).astype(np.int32),
           "return": rng.normal(50, 30, (K, n)).astype(np.float32), "length": rng.integers(1, 500, (K, n)).astype(np.int32),
           "context_id": rng.choice(ctx_pool, (K, n)).astype(np.int32), "terminated": rng.integers(0, 2, (K, n)).astype(np.uint8)}
    pad = np.arange(K)[:, None] >= episodes[None, :]
    res["return"][pad], res["length"][pad], res["context_id"][pad], res["terminated"][pad] = np.nan, 0, -1, 0
    return {k: torch.as_tensor(v) for k, v in res.items()}


def reference(res, n_ctx):
    ep = res["episodes"].numpy()
    K = res["return"].shape[0]
    valid = np.arange(K)[:, None] < ep[None, :]
    r = res["return"].numpy()[valid].astype(np.float64)
    ln = res["length"].numpy()[valid].astype(np.float64)
    c = res["context_id"].numpy()[valid]
    te = res["terminated"].numpy()[valid].astype(np.float64)
    out = {k: np.full(n_ctx, np.nan) for k in ("mean", "std", "len", "term")}
    count = np.zeros(n_ctx)
    for j in range(n_ctx):
        m = c == j
        count[j] = m.sum()
        if m.any():
            out["mean"][j], out["std"][j] = r[m].mean(), r[m].std(ddof=0)
            out["len"][j], out["term"][j] = ln[m].mean(), te[m].mean()
    return count, out, r


@pytest.mark.parametrize("K, n, n_ctx, empty", [(1, 300, 5, ()), (3, 1000, 16, (0, 7, 15)), (4, 17, 40, (3,))])
def test_episode_stats_against_numpy(K, n, n_ctx, empty):
    rng = np.random.default_rng(K * n)
    res = synthetic(rng, K, n, n_ctx, empty)
    s = episode_stats(res, n_contexts=n_ctx)
    count, ref, r = reference(res, n_ctx)
    np.testing.assert_array_equal(s["context_count"], count)
    for key, k in (("context_mean_return", "mean"), ("context_std_return", "std"), ("context_mean_length", "len"),
                   ("context_terminated_share", "term")):
        assert s[key].dtype == np.float64 and s[key].shape == (n_ctx,)
        np.testing.assert_allclose(s[key], ref[k], rtol=1e-12, atol=1e-12, err_msg=key)  # NaN where empty, on both sides
    for j in empty:
        assert count[j] == 0 and np.isnan(s["context_mean_return"][j]) and np.isnan(s["context_std_return"][j])
    np.testing.assert_allclose(s["mean_return"], r.mean(), rtol=1e-13)
    np.testing.assert_allclose(s["std_return"], r.std(ddof=0), rtol=1e-12)
    assert s["count"] == r.size == int(res["episodes"].sum())


def test_episode_stats_ignores_sentinels_and_defaults_its_context_count():
    res = {"episodes": torch.tensor([2, 0, 1], dtype=torch.int32), "steps": torch.tensor([9, 4, 7], dtype=torch.int32),
           "return": torch.tensor([[1.0, np.nan, 5.0], [3.0, np.nan, np.nan]]),
           "length": torch.tensor([[1, 0, 5], [3, 0, 0]], dtype=torch.int32),
           "context_id": torch.tensor([[2, -1, 2], [0, -1, -1]], dtype=torch.int32),
           "terminated": torch.tensor([[1, 0, 0], [0, 0, 0]], dtype=torch.uint8)}
    s = episode_stats(res)
    np.testing.assert_array_equal(s["context_count"], [1, 0, 2])
    np.testing.assert_array_equal(s["context_mean_return"], [3.0, np.nan, 3.0])
    np.testing.assert_array_equal(s["context_std_return"], [0.0, np.nan, 2.0])  # ddof 0: |1 - 5| / 2
    np.testing.assert_array_equal(s["context_terminated_share"], [0.0, np.nan, 0.5])
    assert s["mean_return"] == 3.0 and s["std_return"] == np.std([1.0, 5.0, 3.0]) and s["count"] == 3
    none = dict(res, episodes=torch.zeros(3, dtype=torch.int32))
    s = episode_stats(none, n_contexts=2)
    np.testing.assert_array_equal(s["context_count"], [0, 0])
    assert np.isnan(s["mean_return"]) and np.isnan(s["std_return"]) and np.isnan(s["context_mean_return"]).all()
    with pytest.raises(ValueError, match="outside"):
        episode_stats(res, n_contexts=2)
