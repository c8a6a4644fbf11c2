"""A population of PPO learners, C ABI on the host: every refusal of carl_ppo_grad_sets, carl_ppo_adv_stats_sets and
carl_adam_step_sets by its message (all are validated before anything is enqueued, so they run without a GPU), the workspace
size, the struct binding against a C program compiled with the header, carl_amd.PopulationPPO's and the engine methods'
argument checks as far as they come before a launch.  CPU-only."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import brax_policy_abi_util as U
import policy_cases as PC
from carl_amd import PopulationPPO, _lib
from carl_amd.policy import MLPPolicy
from policy_cases import HEADER

PTR = 0x10000  # a "device pointer" that is never dereferenced: every call here is refused first
GRAD, ADV, ADAM = b"carl_ppo_grad_sets: ", b"carl_ppo_adv_stats_sets: ", b"carl_adam_step_sets: "
INF, NAN = float("inf"), float("nan")
P, L, T = 3, 256, 5


def test_struct_layout_and_hyper_columns_match_c(tmp_path):
    cls, name = _lib.PpoSets, "carl_ppo_sets_t"
    fs = [f[0] for f in cls._fields_]
    macros = ["CARL_PPO_HYPER", "CARL_PPO_HYPER_LR", "CARL_PPO_HYPER_CLIP_RANGE", "CARL_PPO_HYPER_VF_COEF",
              "CARL_PPO_HYPER_ENT_COEF", "CARL_PPO_HYPER_MAX_GRAD_NORM", "CARL_ABI_VERSION"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             f'printf("%zu\\n", sizeof({name}));']
    lines += [f'printf("%zu\\n", offsetof({name}, {f}));' for f in fs]
    lines += [f'printf("%d\\n", {m});' for m in macros] + ["return 0;}"]
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fs] + [
        _lib.PPO_HYPER, _lib.PPO_HYPER_LR, _lib.PPO_HYPER_CLIP_RANGE, _lib.PPO_HYPER_VF_COEF, _lib.PPO_HYPER_ENT_COEF,
        _lib.PPO_HYPER_MAX_GRAD_NORM, 9]
    assert _lib.PPO_HYPER_NAMES == ("lr", "clip_range", "vf_coef", "ent_coef", "max_grad_norm")
    assert _lib.load().carl_abi_version() == _lib.CARL_ABI_VERSION == 9  # additive


# ---------------------------------------------------------------- carl_ppo_grad_sets
def actor(**kw):
    return PC.c_policy(**{"n_sets": P, "lanes_per_set": L, **kw})


def critic(**kw):
    return PC.c_policy(**{"n_out": 1, "head": _lib.POLICY_HEAD_BOX, "n_sets": P, "lanes_per_set": L, **kw})


def batch(**kw):
    b = _lib.PpoBatch()
    b.family, b.n_lanes, b.n_steps, b.row_pitch, b.obs_dim = _lib.CARTPOLE, P * L, T, 0, 4
    b.n_contexts, b.ctx_stride, b.action_dtype, b.n_samples = 4, 4, _lib.ACTION_I32, 512
    b.clip_range, b.vf_coef, b.ent_coef = NAN, -1.0, INF  # (not read: the members' come from hyper)
    for f in ("obs0", "obs", "context_id", "ctx_table", "action", "log_prob", "advantage", "ret"):
        setattr(b, f, PTR)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def sets(**kw):
    s = _lib.PpoSets(PTR, PTR, PTR, 512, 2)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def out(**kw):
    need = _lib.load().carl_ppo_sets_workspace_floats(C.byref(actor()), C.byref(critic()), 512)
    o = _lib.PpoOut(PTR, PTR, PTR, PTR, None, None, PTR, need)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_workspace_floats():
    lib = _lib.load()
    f, one = lib.carl_ppo_sets_workspace_floats, lib.carl_ppo_workspace_floats
    a1, c1 = PC.c_policy(), PC.c_policy(n_out=1, head=_lib.POLICY_HEAD_BOX)
    for n in (1, 256, 257, 300, 512, 1280, 65536, 65537, 10 ** 6):
        assert f(C.byref(actor()), C.byref(critic()), n) == P * one(C.byref(a1), C.byref(c1), n)
        assert f(C.byref(actor(n_sets=1)), C.byref(critic(n_sets=1)), n) == one(C.byref(a1), C.byref(c1), n)
    # 256 workgroups of two 64-wide networks: 2 x 6 540 floats per workgroup, about 13 MB per member
    assert f(C.byref(actor(n_sets=16)), C.byref(critic(n_sets=16)), 10 ** 6) == 16 * 256 * 2 * 6540
    assert 13.0e6 < 256 * 2 * 6540 * 4 < 13.5e6
    assert f(None, C.byref(critic()), 512) == -1 and f(C.byref(actor()), None, 512) == -1
    assert f(C.byref(actor()), C.byref(critic()), 0) == -1 and f(C.byref(actor()), C.byref(critic()), -4) == -1
    assert f(C.byref(actor(n_sets=0)), C.byref(critic()), 512) == -1
    assert f(C.byref(actor(n_hidden=3)), C.byref(critic()), 512) == -1 and f(C.byref(actor()), C.byref(critic(n_hidden=-1)), 512) == -1


GRAD_REFUSALS = [
    # what carl_ppo_grad refuses, by ppo_host_checks.hpp's messages
    (dict(b=dict(family=_lib.CARL_N_FAMILIES)), b"family 5 is a Brax family -- the PPO update covers the classic-control families only"),
    (dict(b=dict(n_lanes=0)), b"n_lanes 0 / n_steps 5 < 1"),
    (dict(b=dict(n_steps=0)), b"n_lanes 768 / n_steps 0 < 1"),
    (dict(b=dict(row_pitch=700)), b"row_pitch 700 < n_lanes 768"),
    (dict(b=dict(obs_dim=3)), b"obs_dim 3, the family's is 4"),
    (dict(a=dict(n_hidden=3)), None),
    (dict(a=dict(n_in=7)), b"n_in 7 != n_ctx 2 + obs_dim 4"),
    (dict(a=dict(n_out=3)), b"head width 3, the family needs 2 (n_actions)"),
    (dict(a=dict(head=_lib.POLICY_HEAD_BOX)), b"head kind 1 does not match the family's action space"),
    (dict(a=dict(params=None)), b"params is NULL"),
    (dict(c=dict(n_out=2)), b"critic: head width 2, the family needs 1 (a value network has 1)"),
    (dict(c=dict(n_ctx=1, n_in=5)), b"critic: n_ctx 1, the actor has 2 (the critic reads the actor's inputs)"),
    (dict(c=dict(params=None)), b"critic: params is NULL"),
    (dict(b=dict(action_dtype=_lib.ACTION_F32)), b"the action column is int32 (CARL_ACTION_I32) for this family"),
    (dict(b=dict(n_contexts=0)), b"n_contexts 0 / ctx_stride 4 invalid"),
    (dict(b=dict(n_samples=0), s=dict(idx_set_stride=0)), b"n_samples 0 < 1"),
    (dict(b=dict(n_samples=3841), s=dict(idx_set_stride=4000)), b"n_samples 3841 > n_steps 5 x n_lanes 768"),
    (dict(b=dict(obs=None)), b"a required pointer of ppo is NULL (all but idx and adv_norm)"),
    (dict(o=dict(stats=None)), b"out->grad_actor, out->grad_critic and out->stats are required"),
    (dict(o=dict(workspace=None)), b"out->workspace is NULL or not on a 16-byte boundary"),
    (dict(o=dict(workspace=PTR + 4)), b"out->workspace is NULL or not on a 16-byte boundary"),
    (dict(o=dict(workspace_floats=100)), None),
    # what only a population can get wrong
    (dict(a=dict(n_sets=0)), b"n_sets 0 < 1"),
    (dict(a=dict(n_sets=-2)), b"n_sets -2 < 1"),
    (dict(a=dict(n_sets=65536), b=dict(n_lanes=65536 * 256)), b"n_sets 65536 > 65535 (the second grid dimension)"),
    (dict(a=dict(lanes_per_set=0)), b"lanes_per_set 0 is not a positive multiple of 256 (carl_policy_lane_quantum)"),
    (dict(a=dict(lanes_per_set=300)), b"lanes_per_set 300 is not a positive multiple of 256 (carl_policy_lane_quantum)"),
    (dict(a=dict(n_sets=2), c=dict(n_sets=2)), b"2 sets x 256 lanes are not the buffer's 768 lanes (member s owns lanes "
                                                b"[s * lanes_per_set, (s + 1) * lanes_per_set))"),
    (dict(a=dict(n_sets=1, lanes_per_set=1024), c=dict(n_sets=1, lanes_per_set=1024)),
     b"1 sets x 1024 lanes are not the buffer's 768 lanes (member s owns lanes [s * lanes_per_set, (s + 1) * lanes_per_set))"),
    (dict(c=dict(n_sets=1)), b"critic: 1 sets x 256 lanes, the actor has 3 x 256"),
    (dict(c=dict(lanes_per_set=512)), b"critic: 3 sets x 512 lanes, the actor has 3 x 256"),
    (dict(s=dict(hyper=None)), b"sets->hyper is NULL"),
    (dict(s=dict(idx=None)), b"sets->idx is NULL (every member's minibatch is a row of indices)"),
    (dict(s=dict(idx_set_stride=511)), b"idx_set_stride 511 < n_samples 512"),
    (dict(s=dict(adv_norm_set_stride=1)), b"adv_norm_set_stride 1 < 2"),
    (dict(b=dict(n_samples=1281), s=dict(idx_set_stride=1281)),
     b"n_samples 1281 > n_steps 5 x lanes_per_set 256 (a member's minibatch is drawn from its own lanes)"),
    (dict(o=dict(new_log_prob=PTR)), b"out->new_log_prob / out->new_value are not offered for a population (NULL)"),
    (dict(o=dict(new_value=PTR)), b"out->new_log_prob / out->new_value are not offered for a population (NULL)"),
]


@pytest.mark.parametrize("kw,msg", GRAD_REFUSALS, ids=[str(i) for i in range(len(GRAD_REFUSALS))])
def test_grad_sets_refusals(kw, msg):
    lib = _lib.load()
    code = lib.carl_ppo_grad_sets(C.byref(batch(**kw.get("b", {}))), C.byref(actor(**kw.get("a", {}))),
                                  C.byref(critic(**kw.get("c", {}))), None, C.byref(sets(**kw.get("s", {}))),
                                  C.byref(out(**kw.get("o", {}))), None)
    if msg is None:  # (a message with computed numbers: the prefix and the code)
        assert code == _lib.ERR_INVALID_ARGUMENT and lib.carl_last_error().startswith(GRAD)
    else:
        U.refused(GRAD, code, msg)


def test_grad_sets_box_family_and_null_structs():
    lib = _lib.load()
    a, c, s, o = actor(n_out=1, head=_lib.POLICY_HEAD_BOX, n_in=5, n_ctx=2), critic(n_in=5, n_ctx=2), sets(), out()
    b = batch(family=_lib.PENDULUM, obs_dim=3, action_dtype=_lib.ACTION_F32)
    U.refused(GRAD, lib.carl_ppo_grad_sets(C.byref(b), C.byref(a), C.byref(c), None, C.byref(s), C.byref(o), None),
              b"a Box family needs log_std and out->grad_log_std ([n_sets] on the device)")
    o2 = out(grad_log_std=None)
    U.refused(GRAD, lib.carl_ppo_grad_sets(C.byref(b), C.byref(a), C.byref(c), PTR, C.byref(s), C.byref(o2), None),
              b"a Box family needs log_std and out->grad_log_std ([n_sets] on the device)")
    b, a, c = batch(), actor(), critic()
    for args in ((None, C.byref(a), C.byref(c), None, C.byref(s), C.byref(o)), (C.byref(b), None, C.byref(c), None, C.byref(s), C.byref(o)),
                 (C.byref(b), C.byref(a), None, None, C.byref(s), C.byref(o)), (C.byref(b), C.byref(a), C.byref(c), None, None, C.byref(o)),
                 (C.byref(b), C.byref(a), C.byref(c), None, C.byref(s), None)):
        U.refused(GRAD, lib.carl_ppo_grad_sets(*args, None), b"ppo / policy / critic / sets / out is NULL")


# ---------------------------------------------------------------- carl_ppo_adv_stats_sets
def adv_args(**kw):
    a = _lib.PpoAdvStats(PTR, PTR, PTR, 4096, 1000, 300, 1e-8)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ADV_REFUSALS = [
    (dict(advantage=None), {}, b"advantage, idx and adv_norm are required"),
    (dict(idx=None), {}, b"advantage, idx and adv_norm are required"),
    (dict(adv_norm=None), {}, b"advantage, idx and adv_norm are required"),
    (dict(n_total=0), {}, b"n_total 0 < 1 or batch_size 300 < 1"),
    (dict(batch_size=0), {}, b"n_total 1000 < 1 or batch_size 0 < 1"),
    (dict(storage_floats=0), {}, b"storage_floats 0 < 1"),
    (dict(eps=-1e-8), {}, b"eps -1e-08 is not finite and >= 0"),
    (dict(eps=NAN), {}, b"eps nan is not finite and >= 0"),
    ({}, dict(n_sets=0), b"n_sets 0 < 1"),
    ({}, dict(n_sets=-1), b"n_sets -1 < 1"),
    ({}, dict(n_sets=65536), b"n_sets 65536 > 65535 (the second grid dimension)"),
    ({}, dict(stride=999), b"idx_set_stride 999 < n_total 1000"),
    ({}, dict(stride=0), b"idx_set_stride 0 < n_total 1000"),
]


@pytest.mark.parametrize("kw,call,msg", ADV_REFUSALS, ids=[str(i) for i in range(len(ADV_REFUSALS))])
def test_adv_stats_sets_refusals(kw, call, msg):
    code = _lib.load().carl_ppo_adv_stats_sets(C.byref(adv_args(**kw)), call.get("n_sets", P), call.get("stride", 1000), None)
    U.refused(ADV, code, msg)


def test_adv_stats_sets_null_struct():
    U.refused(ADV, _lib.load().carl_ppo_adv_stats_sets(None, P, 1000, None), b"the argument struct is NULL")


# ---------------------------------------------------------------- carl_adam_step_sets
def adam_args(n=(100, 50, 1), null=(), **kw):
    a = _lib.Adam()
    a.n_tensors = len(n)
    for i, k in enumerate(n):
        a.n[i] = k
        for f in ("param", "grad", "m", "v"):
            getattr(a, f)[i] = None if (f, i) in null else PTR
    a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm = NAN, 0.9, 0.999, 1e-5, -1.0  # (lr, max_grad_norm: not read)
    a.step, a.beta_pow, a.norm_out = PTR, PTR, None
    for k, v in kw.items():
        setattr(a, k, v)
    return a


MOST = 1 << 18
ADAM_REFUSALS = [
    (dict(n_tensors=0), {}, b"n_tensors 0 outside [1, 4]"),
    (dict(n_tensors=5), {}, b"n_tensors 5 outside [1, 4]"),
    (dict(n=(100, -1)), {}, b"n[1] = -1 < 0"),
    (dict(n=(MOST, 1)), {}, b"more than 262144 elements in all (carl_adam_step_max_floats)"),  # per member
    (dict(null=(("param", 0),)), {}, b"param, grad, m and v of tensor 0 are required"),
    (dict(null=(("v", 2),)), {}, b"param, grad, m and v of tensor 2 are required"),
    (dict(step=None), {}, b"step and beta_pow are required"),
    (dict(beta_pow=None), {}, b"step and beta_pow are required"),
    (dict(eps=0.0), {}, b"eps 0 is not finite and > 0"),
    (dict(eps=INF), {}, b"eps inf is not finite and > 0"),
    (dict(beta1=1.0), {}, b"beta1 1 / beta2 0.999 outside [0, 1)"),
    (dict(beta2=NAN), {}, b"beta1 0.9 / beta2 nan outside [0, 1)"),
    ({}, dict(n_sets=0), b"n_sets 0 < 1"),
    ({}, dict(n_sets=-3), b"n_sets -3 < 1"),
    ({}, dict(n_sets=65536), b"n_sets 65536 > 65535 (the second grid dimension)"),
    ({}, dict(hyper=None), b"hyper is NULL (lr and max_grad_norm are read from the device)"),
]


@pytest.mark.parametrize("kw,call,msg", ADAM_REFUSALS, ids=[str(i) for i in range(len(ADAM_REFUSALS))])
def test_adam_step_sets_refusals(kw, call, msg):
    code = _lib.load().carl_adam_step_sets(C.byref(adam_args(**kw)), call.get("n_sets", P), call.get("hyper", PTR), None)
    U.refused(ADAM, code, msg)


def test_adam_step_sets_null_struct_and_nothing_to_do():
    lib = _lib.load()
    U.refused(ADAM, lib.carl_adam_step_sets(None, P, PTR, None), b"the argument struct is NULL")
    assert lib.carl_adam_step_sets(C.byref(adam_args(n=(0, 0))), P, PTR, None) == 0  # nothing is enqueued


# ---------------------------------------------------------------- carl_amd.PopulationPPO and the engine methods, before a launch
def host_population(family=_lib.CARTPOLE, n=P * L):
    eng = PC.fake_engine(family)
    eng.n = n
    eng.b = _lib.Batch()
    eng.b.flags = _lib.FLAG_AUTORESET
    eng.device, eng.lib = torch.device("cpu"), _lib.load()
    rng = np.random.default_rng(0)
    n_out = 2 if family == _lib.CARTPOLE else 1
    actors = [MLPPolicy.for_env(eng, PC.rand_layers(rng, [eng.F + eng.D, 8, n_out])) for _ in range(P)]
    critics = [MLPPolicy.for_env(eng, PC.rand_layers(rng, [eng.F + eng.D, 8, 1]), head="value") for _ in range(P)]
    return eng, actors, critics


def test_population_ppo_checks_its_arguments():
    eng, actors, critics = host_population()
    ok = dict(lanes_per_set=L, n_steps=T)
    rng = np.random.default_rng(1)
    wide = MLPPolicy.for_env(eng, PC.rand_layers(rng, [eng.F + eng.D, 16, 2]))
    bad = [
        ((eng, actors[:2], critics), ok, "one actor and one critic per member"),
        ((eng, [], []), ok, "one actor and one critic per member"),
        ((eng, [actors[0], actors[1], wide], critics), ok, "must have one shape"),
        ((eng, actors, [critics[0], critics[1], actors[2]]), ok, "must have one shape"),
        ((eng, [MLPPolicy.stack(actors, L)] * P, critics), ok, "one-set host-built"),
        ((eng, actors, critics), dict(ok, lanes_per_set=300), "not a positive multiple of 256"),
        ((eng, actors, critics), dict(ok, lanes_per_set=512), "1536"),
        ((object(), actors, critics), ok, "not a classic-control CARLEnv or VecEngine"),
        ((eng, actors, critics), dict(ok, batch_size=T * L + 1), "batch_size"),
        ((eng, actors, critics), dict(ok, batch_size=0), "batch_size"),
        ((eng, actors, critics), dict(ok, lr=[1e-3, 1e-3]), "lr has 2 values"),
        ((eng, actors, critics), dict(ok, lr=-1e-3), "lr -0.001: finite and >= 0"),
        ((eng, actors, critics), dict(ok, lr=[1e-3, NAN, 1e-3]), "lr nan: finite and >= 0"),
        ((eng, actors, critics), dict(ok, clip_range=INF), "clip_range inf: finite and >= 0"),
        ((eng, actors, critics), dict(ok, vf_coef=[0.5, 0.5, -0.5]), "vf_coef -0.5: finite and >= 0"),
        ((eng, actors, critics), dict(ok, ent_coef=NAN), "ent_coef nan: finite and >= 0"),
        ((eng, actors, critics), dict(ok, max_grad_norm=-1.0), "max_grad_norm -1.0: >= 0"),
        ((eng, actors, critics), dict(ok, max_grad_norm=[0.5, NAN, None]), "max_grad_norm nan: >= 0"),
    ]
    for args, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            PopulationPPO(*args, **kw)
    for name in ("normalize_inputs", "normalize_reward"):  # they are not parameters
        with pytest.raises(TypeError, match=name):
            PopulationPPO(eng, actors, critics, **ok, **{name: True})
    eng.b.flags = 0
    with pytest.raises(ValueError, match="auto_reset=True"):
        PopulationPPO(eng, actors, critics, **ok)
    eng5, actors5, _ = host_population(_lib.PENDULUM)
    with pytest.raises(ValueError, match="family"):
        PopulationPPO(eng, actors5, critics, **ok)


def test_population_ppo_refuses_brax_policies_and_engines():
    import brax_policy_cases as BPC
    from carl_amd.brax_engine import BraxVecEngine

    eng, actors, critics = host_population()
    brax_eng = BPC.fake_engine("ant") if hasattr(BPC, "fake_engine") else object.__new__(BraxVecEngine)
    with pytest.raises(ValueError, match="Brax engines, MixedVecEngine pairs and the gymnasium drop-in are out of scope"):
        PopulationPPO(brax_eng, actors, critics, lanes_per_set=L, n_steps=T)
    for method in ("ppo_grad_sets", "ppo_sets_workspace"):
        with pytest.raises(NotImplementedError, match="classic-control families only"):
            getattr(object.__new__(BraxVecEngine), method)()


def test_engine_methods_check_their_tensors_before_the_launch():
    eng, actors, critics = host_population()
    f32, i32, f64 = torch.float32, torch.int32, torch.float64
    adv, idx = torch.zeros(4, 10), torch.zeros((P, 12), dtype=i32)
    for a, i, kw, msg in ((adv.double(), idx, {}, "'advantage'"), (adv.t(), idx, {}, "'advantage'"),
                          (adv, idx.long(), {}, "'idx'"), (adv, idx[0], {}, "'idx'"), (adv, idx[:, ::2], {}, "'idx'"),
                          (adv, idx[:, :0], {}, "'idx'"), (adv, idx, dict(batch_size=0), "batch_size 0 < 1"),
                          (adv, idx, dict(out=torch.zeros(3, 2)), r"'out'.*\[3, 3, 2\]"),
                          (adv, idx, dict(out=torch.zeros(P, 3, 2, dtype=f64)), "'out'")):
        with pytest.raises(ValueError, match=msg):
            eng.ppo_adv_stats_sets(a, i, **{"batch_size": 5, **kw})
    p, g = [torch.zeros(P, 3), torch.zeros(P, 4)], [torch.zeros(P, 3), torch.zeros(P, 4)]
    st = eng.adam_state(p, n_sets=P)
    assert [tuple(t.shape) for t in st["m"] + st["v"]] == [(P, 3), (P, 4)] * 2 and st["step"].dtype == torch.int64
    assert st["step"].tolist() == [0] * P and st["beta_pow"].tolist() == [[1.0, 1.0]] * P and st["beta_pow"].dtype == f64
    one = eng.adam_state(p)  # the present behaviour is the default
    assert tuple(one["step"].shape) == (1,) and tuple(one["beta_pow"].shape) == (2,)
    with pytest.raises(ValueError, match="n_sets 2"):
        eng.adam_state(p, n_sets=2)
    hyper = torch.zeros(P, _lib.PPO_HYPER, dtype=f64)
    bad = [
        (([], [], st, hyper), {}, "0 tensors"),
        ((p * 3, g * 3, st, hyper), {}, "6 tensors"),
        ((p, g[:1], st, hyper), {}, "need 2 gradients"),
        ((p, [g[0], torch.zeros(P, 5)], st, hyper), {}, r"grads\[1\].*\[3, 4\]"),
        ((p, [g[0].double(), g[1]], st, hyper), {}, r"grads\[0\]"),
        (([p[0], torch.zeros(2, 6)], g, st, hyper), {}, r"params\[1\]"),
        ((p, g, {**st, "step": torch.zeros(1, dtype=torch.int64)}, hyper), {}, r"state\['step'\]"),
        ((p, g, {**st, "beta_pow": torch.ones(2, dtype=f64)}, hyper), {}, r"state\['beta_pow'\]"),
        ((p, g, st, hyper), dict(norm_out=torch.zeros(2, dtype=f64)), "'norm_out'"),
        ((p, g, st, hyper.float()), {}, "'hyper'"),
        ((p, g, st, hyper[:2]), {}, "'hyper'"),
        ((p, g, st, torch.zeros(P, 4, dtype=f64)), {}, "'hyper'"),
    ]
    for args, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            eng.adam_step_sets(*args, **kw)
    # ppo_grad_sets: the set layout against the engine, before anything else
    stacked_a, stacked_c = MLPPolicy.stack(actors, L), MLPPolicy.stack(critics, L, head="value")
    with pytest.raises(ValueError, match="same weight sets and lanes_per_set"):
        eng.ppo_grad_sets(actors[0], critics[0], {}, None, None, idx=None, hyper=hyper)
    with pytest.raises(ValueError, match="same weight sets and lanes_per_set"):
        eng.ppo_grad_sets(stacked_a, MLPPolicy.stack(critics[:2], L, head="value"), {}, None, None, idx=None, hyper=hyper)
    eng.n = 1024
    with pytest.raises(ValueError, match="3 sets x 256 lanes are not this engine's 1024 lanes"):
        eng.ppo_grad_sets(stacked_a, stacked_c, {}, None, None, idx=None, hyper=hyper)
