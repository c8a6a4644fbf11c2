"""PPO's running normalisation, C ABI on the host: every refusal of carl_ppo_input_stats, carl_brax_ppo_input_stats,
carl_ppo_return_stats and carl_ppo_return_merge by its message (all are validated before anything is enqueued, so they run
without a GPU), the slab counts, the struct binding, carl_amd.PPO's new arguments and the ``steps`` / ``input_partial``
contract of ``ppo_input_stats`` as far as it is checked before a launch.  CPU-only."""
import ctypes as C
import inspect
import subprocess

import numpy as np
import pytest
import torch

import brax_policy_abi_util as U
import brax_policy_cases as BP
import policy_cases as PC
from carl_amd import PPO, _lib
from carl_amd.brax_engine import _BRAX_FAMILY
from carl_amd.policy import InputStats, MLPPolicy
from policy_cases import HEADER, c_policy

PTR = 0x10000  # a 16-byte-aligned "device pointer" that is never dereferenced: every call here is refused first
ANT = BP.build_model("ant")[0]
INPUT, BRAX_INPUT = b"carl_ppo_input_stats: ", b"carl_brax_ppo_input_stats: "
WALK, MERGE = b"carl_ppo_return_stats: ", b"carl_ppo_return_merge: "


def test_struct_layout_matches_c(tmp_path):
    cls, name = _lib.PpoReturnStats, "carl_ppo_return_stats_t"
    fs = [f[0] for f in cls._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             f'printf("%zu\\n", sizeof({name}));']
    lines += [f'printf("%zu\\n", offsetof({name}, {f}));' for f in fs]
    lines += ["return 0;}"]
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fs]
    assert _lib.load().carl_abi_version() == _lib.CARL_ABI_VERSION == 9  # additive


def test_slab_counts():
    lib = _lib.load()
    f = lib.carl_ppo_input_stats_slabs
    assert [f(0, 4), f(-1, 4), f(4, 0), f(4, -3)] == [0, 0, 0, 0]
    assert [f(1, 1), f(256, 1), f(257, 1), f(300, 9), f(65536, 1), f(65536, 128), f(2 ** 30, 1)] == [1, 1, 2, 11, 256, 256, 256]
    g = lib.carl_ppo_return_stats_slabs
    assert [g(-5), g(0), g(1), g(256), g(257), g(65536)] == [0, 0, 1, 1, 2, 256]


# ---------------------------------------------------------------- carl_ppo_input_stats
def classic_batch(**kw):
    """a valid carl_ppo_batch_t for c_policy() (CartPole: 2 context inputs + 4 observations; 1000 lanes x 4 steps)"""
    b = _lib.PpoBatch()
    b.family, b.n_lanes, b.n_steps, b.row_pitch, b.obs_dim = _lib.CARTPOLE, 1000, 4, 1008, 4
    b.n_contexts, b.ctx_stride, b.n_samples = 4, 4, 4000
    for f in ("obs0", "obs", "context_id", "ctx_table"):
        setattr(b, f, PTR)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def stats(partial=PTR, capacity=256):
    return _lib.PolicyStats(partial, capacity)


def input_stats(b=None, pol=None, st=None, fn="carl_ppo_input_stats", null=()):
    b, pol, st = b or classic_batch(), pol or c_policy(), st or stats()
    args = [None if k in null else C.byref(v) for k, v in (("ppo", b), ("policy", pol), ("stats", st))]
    return getattr(_lib.load(), fn)(*args, None)


INPUT_REFUSALS = [
    (dict(null=("ppo",)), b"ppo / policy is NULL"),
    (dict(null=("policy",)), b"ppo / policy is NULL"),
    (dict(b=classic_batch(family=_lib.CARL_N_FAMILIES)), b"family 5 is a Brax family -- its sums are carl_brax_ppo_input_stats"),
    (dict(b=classic_batch(obs_dim=3)), b"obs_dim 3, the family's is 4"),
    (dict(pol=c_policy(n_out=5)), b"the policy's shape is outside the limits"),
    (dict(pol=c_policy(n_in=33)), b"the policy's shape is outside the limits"),
    (dict(pol=c_policy(width=(65, 64))), b"the policy's shape is outside the limits"),
    (dict(pol=c_policy(params=None)), b"params is NULL"),
    (dict(pol=c_policy(n_ctx=-1)), b"n_ctx -1 outside [0, n_in = 6]"),
    (dict(pol=c_policy(n_ctx=7)), b"n_ctx 7 outside [0, n_in = 6]"),
    (dict(pol=c_policy(ctx_rows=(0, 8))), b"ctx_rows[1] = 8 is not a context-table row"),
    (dict(pol=c_policy(ctx_rows=(-1, 3))), b"ctx_rows[0] = -1 is not a context-table row"),
    (dict(pol=c_policy(n_in=7)), b"n_in 7 != n_ctx 2 + obs_dim 4"),
    (dict(b=classic_batch(idx=PTR)), b"idx must be NULL (the sums run over every sample of the buffer)"),
    (dict(b=classic_batch(n_steps=0)), b"n_steps 0 < 1 or n_lanes 1000 < 0"),
    (dict(b=classic_batch(n_lanes=-1, row_pitch=0)), b"n_steps 4 < 1 or n_lanes -1 < 0"),
    (dict(b=classic_batch(row_pitch=999)), b"row_pitch 999 < n_lanes 1000"),
    (dict(b=classic_batch(n_steps=2 ** 22, row_pitch=1024)), b"4194304 steps x 1024 lanes per row: flat indices do not fit 2^31 - 1"),
    (dict(b=classic_batch(n_contexts=0)), b"n_contexts 0 / ctx_stride 4 invalid"),
    (dict(b=classic_batch(ctx_stride=3)), b"n_contexts 4 / ctx_stride 3 invalid"),
    (dict(b=classic_batch(obs0=None)), b"obs0, obs, context_id and ctx_table are required"),
    (dict(b=classic_batch(obs=None)), b"obs0, obs, context_id and ctx_table are required"),
    (dict(b=classic_batch(context_id=None)), b"obs0, obs, context_id and ctx_table are required"),
    (dict(b=classic_batch(ctx_table=None)), b"obs0, obs, context_id and ctx_table are required"),
    (dict(null=("stats",)), b"stats / stats->partial is NULL"),
    (dict(st=stats(partial=None)), b"stats / stats->partial is NULL"),
    (dict(st=stats(partial=PTR + 8)), b"stats->partial is not on a 16-byte boundary"),
    (dict(st=stats(capacity=15)), b"stats->partial_capacity 15 < 16 slabs (carl_ppo_input_stats_slabs)"),
]


@pytest.mark.parametrize("kw,msg", INPUT_REFUSALS, ids=[str(i) for i in range(len(INPUT_REFUSALS))])
def test_input_stats_refusals(kw, msg):
    U.refused(INPUT, input_stats(**kw), msg)


def test_input_stats_of_an_unknown_family_and_without_lanes():
    assert input_stats(b=classic_batch(family=-1)) == _lib.ERR_INVALID_ARGUMENT
    assert b"unknown family -1" in _lib.load().carl_last_error()
    assert input_stats(b=classic_batch(n_lanes=0, row_pitch=0), st=stats(capacity=0)) == 0  # nothing is enqueued


# ---------------------------------------------------------------- carl_brax_ppo_input_stats
def brax_batch(**kw):
    """a valid carl_ppo_batch_t for U.policy(ANT): 2 context inputs + 27 observations, dense rows"""
    return classic_batch(**{**dict(family=_BRAX_FAMILY, row_pitch=0, obs_dim=ANT.obs_dim), **kw})


BRAX_INPUT_REFUSALS = [
    (dict(null=("ppo",)), b"ppo / policy is NULL"),
    (dict(b=brax_batch(family=_lib.CARTPOLE)), b"family 0 is a classic-control family -- its sums are carl_ppo_input_stats"),
    (dict(b=brax_batch(family=_lib.CARL_N_FAMILIES - 1)), b"family 4 is a classic-control family -- its sums are "
                                                           b"carl_ppo_input_stats"),
    (dict(b=brax_batch(row_pitch=1008)), b"row_pitch 1008: Brax families take dense rows (0 or n_lanes = 1000)"),
    (dict(pol=U.policy(ANT, n_out=25)), b"the policy's shape is outside the limits"),
    (dict(pol=U.policy(ANT, params=None)), b"params is NULL"),
    (dict(pol=U.policy(ANT, n_ctx=30)), b"n_ctx 30 outside [0, n_in = 29]"),
    (dict(b=brax_batch(obs_dim=26)), b"n_in 29 != n_ctx 2 + obs_dim 26"),
    (dict(b=brax_batch(obs_dim=0), pol=U.policy(ANT, n_in=2)), b"n_in 2 != n_ctx 2 + obs_dim 0"),
    (dict(b=brax_batch(idx=PTR)), b"idx must be NULL (the sums run over every sample of the buffer)"),
    (dict(b=brax_batch(n_steps=0)), b"n_steps 0 < 1 or n_lanes 1000 < 0"),
    (dict(b=brax_batch(obs=None)), b"obs0, obs, context_id and ctx_table are required"),
    (dict(st=stats(partial=PTR + 4)), b"stats->partial is not on a 16-byte boundary"),
    (dict(st=stats(capacity=0)), b"stats->partial_capacity 0 < 16 slabs (carl_ppo_input_stats_slabs)"),
]


@pytest.mark.parametrize("kw,msg", BRAX_INPUT_REFUSALS, ids=[str(i) for i in range(len(BRAX_INPUT_REFUSALS))])
def test_brax_input_stats_refusals(kw, msg):
    kw = dict(kw)
    kw.setdefault("b", brax_batch())
    kw.setdefault("pol", U.policy(ANT))
    U.refused(BRAX_INPUT, input_stats(fn="carl_brax_ppo_input_stats", **kw), msg)


def test_brax_input_stats_takes_a_wide_head_and_a_far_context_row():
    """what the classic entry point refuses of a shape (8 outputs) and of a row (beyond a classic table) passes here; with
    no lane nothing is enqueued"""
    p = U.policy(ANT)
    p.ctx_rows[1] = 40
    assert input_stats(b=brax_batch(n_lanes=0), pol=p, st=stats(capacity=0), fn="carl_brax_ppo_input_stats") == 0


# ---------------------------------------------------------------- carl_ppo_return_stats / carl_ppo_return_merge
def walk_args(**kw):
    rs = _lib.PpoReturnStats()
    rs.n_lanes, rs.n_steps, rs.row_pitch, rs.gamma = 1000, 4, 1008, 0.99
    rs.reward = rs.terminated = rs.truncated = rs.ret = rs.partial = PTR
    rs.partial_capacity = 4
    for k, v in kw.items():
        setattr(rs, k, v)
    return rs


WALK_REFUSALS = [
    (dict(n_steps=0), b"n_steps 0 < 1 or n_lanes 1000 < 0"),
    (dict(n_lanes=-2, row_pitch=0), b"n_steps 4 < 1 or n_lanes -2 < 0"),
    (dict(row_pitch=512), b"row_pitch 512 < n_lanes 1000"),
    (dict(gamma=-0.5), b"gamma -0.5 is not finite and >= 0"),
    (dict(gamma=float("nan")), b"gamma nan is not finite and >= 0"),
    (dict(reward=None), b"reward, terminated, truncated and ret are required"),
    (dict(terminated=None), b"reward, terminated, truncated and ret are required"),
    (dict(truncated=None), b"reward, terminated, truncated and ret are required"),
    (dict(ret=None), b"reward, terminated, truncated and ret are required"),
    (dict(partial=None), b"partial is NULL or not on a 16-byte boundary"),
    (dict(partial=PTR + 8), b"partial is NULL or not on a 16-byte boundary"),
    (dict(partial_capacity=3), b"partial_capacity 3 < 4 slabs (carl_ppo_return_stats_slabs)"),
]


@pytest.mark.parametrize("kw,msg", WALK_REFUSALS, ids=[str(i) for i in range(len(WALK_REFUSALS))])
def test_return_stats_refusals(kw, msg):
    U.refused(WALK, _lib.load().carl_ppo_return_stats(C.byref(walk_args(**kw)), None), msg)


def test_return_stats_null_struct_and_no_lanes():
    lib = _lib.load()
    U.refused(WALK, lib.carl_ppo_return_stats(None, None), b"the argument struct is NULL")
    assert lib.carl_ppo_return_stats(C.byref(walk_args(n_lanes=0, row_pitch=0, partial_capacity=0)), None) == 0
    assert lib.carl_ppo_return_stats(C.byref(walk_args(ret_rows=None, n_lanes=0, row_pitch=0)), None) == 0


def merge(partial=PTR, n_slabs=4, n_b=4000, running="ok", eps=1e-8, scale=PTR):
    run = _lib.PolicyRunningStats(PTR, PTR, PTR) if running == "ok" else running
    return _lib.load().carl_ppo_return_merge(partial, n_slabs, n_b, None if run is None else C.byref(run), eps, scale, None)


MERGE_REFUSALS = [
    (dict(partial=None), b"partial is NULL or not on a 16-byte boundary"),
    (dict(partial=PTR + 8), b"partial is NULL or not on a 16-byte boundary"),
    (dict(n_slabs=-1), b"n_slabs -1 < 0"),
    (dict(n_b=-1), b"n_b -1 < 0"),
    (dict(running=None), b"running and its three arrays are required"),
    (dict(running=_lib.PolicyRunningStats(None, PTR, PTR)), b"running and its three arrays are required"),
    (dict(running=_lib.PolicyRunningStats(PTR, None, PTR)), b"running and its three arrays are required"),
    (dict(running=_lib.PolicyRunningStats(PTR, PTR, None)), b"running and its three arrays are required"),
    (dict(eps=-1e-8), b"eps -1e-08 is not finite and >= 0"),
    (dict(eps=float("inf")), b"eps inf is not finite and >= 0"),
    (dict(scale=None), b"scale is NULL"),
]


@pytest.mark.parametrize("kw,msg", MERGE_REFUSALS, ids=[str(i) for i in range(len(MERGE_REFUSALS))])
def test_return_merge_refusals(kw, msg):
    U.refused(MERGE, merge(**kw), msg)


def test_return_merge_of_nothing_enqueues_nothing():
    assert merge(n_b=0) == 0


# ---------------------------------------------------------------- carl_amd.PPO and the engine methods, before a launch
def host_networks():
    eng = PC.fake_engine(_lib.CARTPOLE)
    eng.b = _lib.Batch()
    eng.b.flags = _lib.FLAG_AUTORESET
    eng.device, eng.lib = torch.device("cpu"), _lib.load()
    rng = np.random.default_rng(0)
    actor = MLPPolicy.for_env(eng, PC.rand_layers(rng, [eng.F + 4, 8, 2]))
    critic = MLPPolicy.for_env(eng, PC.rand_layers(rng, [eng.F + 4, 8, 1]), head="value")
    return eng, actor, critic


def test_ppo_takes_the_normalisation_arguments_off_by_default():
    p = inspect.signature(PPO.__init__).parameters
    assert [p[k].default for k in ("normalize_inputs", "normalize_reward", "clip_reward", "norm_eps")] == [False, False, 10.0, 1e-8]
    eng, actor, critic = host_networks()
    for kw, msg in ((dict(clip_reward=0.0), "clip_reward"), (dict(clip_reward=float("nan")), "clip_reward"),
                    (dict(norm_eps=-1.0), "norm_eps"), (dict(norm_eps=float("inf")), "norm_eps")):
        with pytest.raises(ValueError, match=msg):
            PPO(eng, actor, critic, n_steps=4, normalize_inputs=True, normalize_reward=True, **kw)
    with pytest.raises(ValueError, match="norm_eps 0 with normalize_reward"):  # constant returns would give scale = inf
        PPO(eng, actor, critic, n_steps=4, normalize_reward=True, norm_eps=0.0)


def test_input_stats_result_contract_is_checked_before_the_launch():
    eng, actor, critic = host_networks()
    N, T, D = eng.n, 3, eng.D
    obs0, obs = torch.zeros(N, D), torch.zeros(T, N, D)
    cid = torch.zeros((T, N), dtype=torch.int32)
    with pytest.raises(ValueError, match="context_id"):
        eng.ppo_input_stats(actor, {"obs": obs}, obs0, cid.long())
    with pytest.raises(ValueError, match="'obs'"):
        eng.ppo_input_stats(actor, {"obs": obs[:, :, :3]}, obs0, cid)
    with pytest.raises(ValueError, match="obs0"):
        eng.ppo_input_stats(actor, {"obs": obs}, obs0[:-1], cid)
    slabs = _lib.load().carl_ppo_input_stats_slabs(N, T)
    with pytest.raises(ValueError, match=f"input_partial.*>= {slabs}, 2, 32"):
        eng.ppo_input_stats(actor, {"obs": obs}, obs0, cid, out={"input_partial": torch.zeros(slabs - 1, 2, 32, dtype=torch.float64)})
    with pytest.raises(ValueError, match="steps.*filled with T"):
        eng.ppo_input_stats(actor, {"obs": obs}, obs0, cid, out={"steps": torch.zeros(N, dtype=torch.int64)})
    # what InputStats.update reads of a result
    with pytest.raises(ValueError, match="input_partial"):
        InputStats(actor, "cpu").update({"steps": torch.zeros(N, dtype=torch.int32)}, policy=actor)
