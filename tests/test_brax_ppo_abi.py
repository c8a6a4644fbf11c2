"""The PPO update of the Brax families, C ABI on the host: every refusal of carl_brax_policy_context_trace and
carl_brax_ppo_grad by its message, in the header's order (all are validated before anything is enqueued, so they run
without a GPU), the workspace / tile / workgroups functions, the struct bindings, and the ValueErrors of carl_amd.PPO and of
the engine methods that are raised before a launch.  CPU-only."""
import ctypes as C

import numpy as np
import pytest
import torch

import brax_policy_abi_util as U
import brax_policy_cases as BP
import brax_ppo_ref as BR
from carl_amd import PPO, _lib
from carl_amd.brax_engine import BraxVecEngine
from carl_amd.brax_policy import BraxMLPPolicy

PTR = 0x10000  # a 16-byte-aligned "device pointer" that is never dereferenced: every call here is refused first
ANT = BP.build_model("ant")[0]
HUMANOID = BP.build_model("humanoid")[0]
TRACE, GRAD = b"carl_brax_policy_context_trace: ", b"carl_brax_ppo_grad: "


def test_the_bindings_take_the_structs_of_the_classic_entry_points():
    lib = _lib.load()
    assert lib.carl_brax_ppo_grad.argtypes[0]._type_ is _lib.PpoBatch and lib.carl_brax_ppo_grad.argtypes[5]._type_ is _lib.PpoOut
    assert lib.carl_brax_ppo_grad.argtypes[1]._type_ is _lib.BraxSys
    assert len(lib.carl_brax_policy_context_trace.argtypes) == 8  # no row pitch: dense rows
    assert lib.carl_abi_version() == _lib.CARL_ABI_VERSION  # additive


# ---------------------------------------------------------------- carl_brax_policy_context_trace
def classic_batch(family):
    b = U.batch()
    b.family = family
    return b


def trace(b, ctx0=PTR, ep0=PTR, te=PTR, tr=PTR, T=12, out=PTR):
    return _lib.load().carl_brax_policy_context_trace(None if b is None else C.byref(b), ctx0, ep0, te, tr, T, out, None)


TRACE_REFUSALS = [
    (dict(b=None), b"batch is NULL"),
    (dict(b=classic_batch(_lib.CARTPOLE)), b"family 0 is a classic-control family -- its trace is carl_policy_context_trace"),
    (dict(b=classic_batch(_lib.CARL_N_FAMILIES - 1)), b"family 4 is a classic-control family -- its trace is "
                                                        b"carl_policy_context_trace"),
    (dict(b=U.batch(n=-1)), b"n_lanes -1 / n_steps 12 < 0"),
    (dict(b=U.batch(), T=-2), b"n_lanes 1000 / n_steps -2 < 0"),
    (dict(b=U.batch(n_contexts=0)), b"n_contexts 0 < 1"),
    (dict(b=U.batch(selector=9)), b"unknown selector 9"),
    (dict(b=U.batch(), ctx0=None), b"a required pointer is NULL"),
    (dict(b=U.batch(), ep0=None), b"a required pointer is NULL"),
    (dict(b=U.batch(), te=None), b"a required pointer is NULL"),
    (dict(b=U.batch(), tr=None), b"a required pointer is NULL"),
    (dict(b=U.batch(), out=None), b"a required pointer is NULL"),
]


@pytest.mark.parametrize("kw,msg", TRACE_REFUSALS, ids=[str(i) for i in range(len(TRACE_REFUSALS))])
def test_context_trace_refusals(kw, msg):
    U.refused(TRACE, trace(**kw), msg)


def test_context_trace_without_work_enqueues_nothing():
    assert trace(U.batch(n=0)) == 0 and trace(U.batch(), T=0) == 0


# ---------------------------------------------------------------- carl_brax_ppo_grad
def critic(s=ANT, **kw):
    return U.policy(s, **{**dict(n_out=1), **kw})


def ppo_batch(s=ANT, **kw):
    """a valid carl_ppo_batch_t for U.policy(s) (1000 envs x 4 steps, dense rows, every sample)"""
    b = _lib.PpoBatch()
    b.family, b.n_lanes, b.n_steps, b.row_pitch, b.obs_dim = -1, 1000, 4, 0, s.obs_dim
    b.n_contexts, b.ctx_stride, b.action_dtype, b.n_samples = 4, 4, _lib.ACTION_F32, 4000
    b.clip_range, b.vf_coef, b.ent_coef = 0.2, 0.5, 0.0
    for f in ("obs0", "obs", "context_id", "ctx_table", "action", "log_prob", "advantage", "ret"):
        setattr(b, f, PTR)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def ppo_out(pol=None, crit=None, M=4000, **kw):
    o = _lib.PpoOut()
    o.grad_actor = o.grad_critic = o.grad_log_std = o.stats = o.workspace = PTR
    o.workspace_floats = _lib.load().carl_brax_ppo_workspace_floats(C.byref(pol or U.policy(ANT)), C.byref(crit or critic()), M)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def grad(b=None, s=ANT, pol=None, crit=None, log_std=PTR, out=None):
    b, pol, crit = b or ppo_batch(s), pol or U.policy(s), crit or critic(s)
    out = out or ppo_out(M=max(b.n_samples, 1))
    return _lib.load().carl_brax_ppo_grad(C.byref(b), C.byref(s), C.byref(pol), C.byref(crit), log_std, C.byref(out), None)


def rows(a, b_):
    p = U.policy(ANT)
    p.ctx_rows[0], p.ctx_rows[1] = a, b_
    return p


def crit_rows(a, b_):
    p = critic()
    p.ctx_rows[0], p.ctx_rows[1] = a, b_
    return p


def width(w0, w1, maker=U.policy):
    p = maker(ANT)
    p.width[0], p.width[1] = w0, w1
    return p


GRAD_REFUSALS = [
    (dict(b=ppo_batch(family=_lib.PENDULUM)), b"family %d is a classic-control family -- its update is carl_ppo_grad" % _lib.PENDULUM),
    (dict(b=ppo_batch(n_lanes=0)), b"n_lanes 0 / n_steps 4 < 1"),
    (dict(b=ppo_batch(n_steps=0)), b"n_lanes 1000 / n_steps 0 < 1"),
    (dict(b=ppo_batch(row_pitch=1008)), b"row_pitch 1008: Brax families take dense rows (0 or n_lanes = 1000)"),
    (dict(b=ppo_batch(obs_dim=26)), b"obs_dim 26, the model's is 27"),
    (dict(s=HUMANOID, b=ppo_batch(HUMANOID), pol=U.policy(HUMANOID), crit=critic(HUMANOID)),
     b"17 actuators: the sampled closed loop and its update hold at most 8"),
    (dict(pol=U.policy(ANT, n_hidden=3)), b"n_hidden 3 outside [0, 2]"),
    (dict(pol=width(65, 64)), b"hidden width[0] = 65 outside [1, 64]"),
    (dict(pol=U.policy(ANT, n_ctx=33)), b"n_ctx 33 outside [0, 32]"),
    (dict(pol=U.policy(ANT, n_ctx=6, n_in=33)), b"6 context inputs + 27 observations are more than CARL_POLICY_MAX_IN = 32 "
                                                b"policy inputs (Humanoid-size observations are out of scope)"),
    (dict(pol=rows(0, -1)), b"ctx_rows[1] = -1 is not a context-table row"),
    (dict(pol=U.policy(ANT, n_in=28)), b"n_in 28 != n_ctx 2 + obs_dim 27"),
    (dict(pol=U.policy(ANT, n_out=7)), b"head width 7, the model needs 8 (one output per actuator)"),
    (dict(pol=U.policy(ANT, head=_lib.POLICY_HEAD_ARGMAX)), b"head kind 0: the Brax families take Box actions "
                                                            b"(CARL_POLICY_HEAD_BOX)"),
    (dict(pol=U.policy(ANT, activation=7)), b"unknown activation 7"),
    (dict(pol=U.policy(ANT, n_sets=2)), b"n_sets 2, a gradient step has one weight set (several are evolution strategies' "
                                        b"territory)"),
    (dict(pol=U.policy(ANT, params=None)), b"params is NULL"),
    (dict(crit=critic(n_out=2)), b"critic: head width 2, the model needs 1 (a value network has 1)"),
    (dict(crit=critic(n_sets=3)), b"critic: n_sets 3, a gradient step has one weight set (several are evolution strategies' "
                                  b"territory)"),
    (dict(crit=width(64, 0, critic)), b"critic: hidden width[1] = 0 outside [1, 64]"),
    (dict(crit=critic(n_in=28, n_ctx=1)), b"critic: n_ctx 1, the actor has 2 (the critic reads the actor's inputs)"),
    (dict(crit=crit_rows(0, 2)), b"critic: ctx_rows[1] = 2, the actor's is 1"),
    (dict(crit=critic(params=None)), b"critic: params is NULL"),
    (dict(b=ppo_batch(action_dtype=_lib.ACTION_I32)), b"the action column is float32 (CARL_ACTION_F32) for the Brax families"),
    (dict(b=ppo_batch(n_contexts=0)), b"n_contexts 0 / ctx_stride 4 invalid"),
    (dict(b=ppo_batch(ctx_stride=3)), b"n_contexts 4 / ctx_stride 3 invalid"),
    (dict(b=ppo_batch(n_lanes=1 << 20, n_steps=1 << 11, n_samples=1, idx=PTR)), b"2048 steps x 1048576 lanes per row: flat "
                                                                                b"indices do not fit 2^31 - 1"),
    (dict(b=ppo_batch(n_samples=0, idx=PTR)), b"n_samples 0 < 1"),
    (dict(b=ppo_batch(n_samples=4001, idx=PTR)), b"n_samples 4001 > n_steps 4 x n_lanes 1000"),
    (dict(b=ppo_batch(n_samples=3999)), b"idx is NULL (every sample) but n_samples 3999 != n_steps 4 x n_lanes 1000"),
    (dict(b=ppo_batch(clip_range=-0.1)), b"clip_range -0.1 is not finite and >= 0"),
    (dict(b=ppo_batch(clip_range=float("nan"))), b"clip_range nan is not finite and >= 0"),
    (dict(b=ppo_batch(vf_coef=float("inf"))), b"vf_coef inf is not finite and >= 0"),
    (dict(b=ppo_batch(ent_coef=-1.0)), b"ent_coef -1 is not finite and >= 0"),
    (dict(b=ppo_batch(obs0=None)), b"a required pointer of ppo is NULL (all but idx and adv_norm)"),
    (dict(b=ppo_batch(context_id=None)), b"a required pointer of ppo is NULL (all but idx and adv_norm)"),
    (dict(out=ppo_out(stats=None)), b"out->grad_actor, out->grad_critic and out->stats are required"),
    (dict(out=ppo_out(grad_critic=None)), b"out->grad_actor, out->grad_critic and out->stats are required"),
    (dict(log_std=None), b"log_std and out->grad_log_std are required ([n_act] on the device)"),
    (dict(out=ppo_out(grad_log_std=None)), b"log_std and out->grad_log_std are required ([n_act] on the device)"),
    (dict(out=ppo_out(workspace=None)), b"out->workspace is NULL or not on a 16-byte boundary"),
    (dict(out=ppo_out(workspace=PTR + 4)), b"out->workspace is NULL or not on a 16-byte boundary"),
]


@pytest.mark.parametrize("kw,msg", GRAD_REFUSALS, ids=[str(i) for i in range(len(GRAD_REFUSALS))])
def test_brax_ppo_grad_refusals(kw, msg):
    U.refused(GRAD, grad(**kw), msg)


def test_brax_ppo_grad_refuses_null_structs_and_a_small_workspace():
    lib = _lib.load()
    b, pol, crit, out = ppo_batch(), U.policy(ANT), critic(), ppo_out()
    full = (C.byref(b), C.byref(ANT), C.byref(pol), C.byref(crit), PTR, C.byref(out))
    for hole in (0, 1, 2, 3, 5):
        args = tuple(None if i == hole else a for i, a in enumerate(full))
        U.refused(GRAD, lib.carl_brax_ppo_grad(*args, None), b"ppo / sys / policy / critic / out is NULL")
    need = out.workspace_floats
    U.refused(GRAD, grad(out=ppo_out(workspace_floats=need - 1)),
              b"workspace of %d floats, %d needed (carl_brax_ppo_workspace_floats)" % (need - 1, need))


def test_size_functions():
    lib = _lib.load()
    TS = lib.carl_brax_ppo_tile()
    assert TS == BR.TILE == lib.carl_ppo_tile()
    assert [lib.carl_brax_ppo_grad_workgroups(m) for m in (-1, 0, 1, TS, TS + 1, 2 * TS + 3)] == [0, 0, 1, 1, 2, 3]
    cap = BR.WORKGROUPS_CAP
    assert lib.carl_brax_ppo_grad_workgroups(cap * TS) == cap == lib.carl_brax_ppo_grad_workgroups(cap * TS + 1)
    pol, crit = U.policy(ANT), critic()
    ws = lambda p, c, m: lib.carl_brax_ppo_workspace_floats(C.byref(p), C.byref(c), m)  # noqa: E731
    full, one = ws(pol, crit, 65536 * 128), ws(pol, crit, 1)
    assert 0 < full * 4 < 32 << 20 and full == cap * one and ws(pol, crit, 2 * TS + 3) == 3 * one
    # a slab holds every parameter of both networks
    assert one >= lib.carl_brax_policy_set_floats(C.byref(pol)) + lib.carl_brax_policy_set_floats(C.byref(crit)) - 2 * (2 * 29 + 4)
    lin = ws(U.policy(ANT, n_hidden=0), critic(n_hidden=0), 1)
    assert 0 < lin < one
    assert ws(U.policy(ANT, n_hidden=3), crit, 1) == -1 and ws(pol, crit, 0) == -1
    assert ws(U.policy(ANT, n_out=9), crit, 1) == -1 and ws(pol, U.policy(ANT), 1) == -1  # 9 outputs; a critic with 8
    assert lib.carl_brax_ppo_workspace_floats(None, C.byref(crit), 1) == -1


# ---------------------------------------------------------------- Python: refusals before any launch
def nets(rng=None, rows=()):
    rng = rng or np.random.default_rng(0)
    actor = U.ant_policy(rng, rows=rows)
    crit = BraxMLPPolicy(U.info(27, 8), list(rows), BP.make_layers(rng, 27 + len(rows), (8,), 1), "relu", head="value")
    return actor, crit


def fake_engine(mode="redraw", auto_reset=True, model="ant"):
    eng = U.fake_brax_engine(auto_reset)
    eng.autoreset_mode, eng.family, eng.info = mode, -1, U.info(27, 8)
    if model != "ant":
        eng.sys = BP.build_model(model)[0]
        eng.D = eng.sys.obs_dim
    return eng


def test_ppo_refusals_without_a_gpu():
    from carl_amd.mixed import MixedVecEngine

    actor, crit = nets()
    with pytest.raises(ValueError, match="autoreset_mode='first_state'"):
        PPO(fake_engine("first_state"), actor, crit)
    with pytest.raises(ValueError, match="auto_reset=True"):
        PPO(fake_engine(auto_reset=False), actor, crit)
    with pytest.raises(ValueError, match="17 actuators"):
        PPO(fake_engine(model="humanoid"), actor, crit)
    with pytest.raises(ValueError, match="MixedVecEngine pairs and the gymnasium drop-in are out of scope"):
        PPO(object.__new__(MixedVecEngine), actor, crit)
    with pytest.raises(ValueError, match="gymnasium drop-in"):
        PPO(object(), actor, crit)  # (what the drop-in hands over is no CARLBraxEnv either)
    with pytest.raises(ValueError, match="head='value'"):
        PPO(fake_engine(), actor, actor)
    with pytest.raises(ValueError, match="one-set host-built"):
        PPO(fake_engine(), BraxMLPPolicy.stack([actor, actor], 256), crit)


def test_engine_method_refusals_without_a_gpu():
    eng = fake_engine()
    eng.lib = _lib.load()
    actor, crit = nets()
    T, N = 3, eng.n
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)  # noqa: E731
    buf = {"action": z(T, N, 8), "log_prob": z(T, N), "advantage": z(T, N), "return": z(T, N), "obs": z(T, N, 27)}
    cid, obs0 = z(T, N, dt=torch.int32), z(N, 27)
    with pytest.raises(TypeError, match="BraxMLPPolicy"):
        eng.ppo_grad(object(), crit, buf, obs0, cid)
    with pytest.raises(ValueError, match=r"'action': needs a contiguous float32 \[T, 1024, 8\]"):
        eng.ppo_grad(actor, crit, {**buf, "action": z(T, N)}, obs0, cid)
    with pytest.raises(ValueError, match=r"'action': needs a contiguous float32 \[T, 1024, 8\]"):
        eng.ppo_grad(actor, crit, {**buf, "action": z(T, N, 8, dt=torch.float64)}, obs0, cid)
    with pytest.raises(ValueError, match="'log_prob'"):
        eng.ppo_grad(actor, crit, {**buf, "log_prob": z(T, N + 16)[:, :N]}, obs0, cid)  # padded rows
    with pytest.raises(ValueError, match="'context_id'"):
        eng.ppo_grad(actor, crit, buf, obs0, cid.long())
    with pytest.raises(ValueError, match="'obs0'"):
        eng.ppo_grad(actor, crit, buf, z(N, 26), cid)
    with pytest.raises(ValueError, match="'idx'"):
        eng.ppo_grad(actor, crit, buf, obs0, cid, idx=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="output 'grad_log_std'"):
        eng.ppo_grad(actor, crit, buf, obs0, cid, out={"grad_log_std": z(1)})  # one value per actuator
    with pytest.raises(ValueError, match="ppo_workspace: invalid shapes"):
        eng.ppo_workspace(actor, crit, 0)
    flags = z(T, N, dt=torch.uint8)
    with pytest.raises(ValueError, match="'ctx_idx0'"):
        eng.context_trace(z(N), z(N, dt=torch.int32), flags, flags)
    with pytest.raises(ValueError, match="'truncated'"):
        eng.context_trace(z(N, dt=torch.int32), z(N, dt=torch.int32), flags, flags.float())
    with pytest.raises(ValueError, match="flag rows of 1000 lanes"):
        eng.context_trace(z(N, dt=torch.int32), z(N, dt=torch.int32), flags[:, :1000], flags[:, :1000])
    assert isinstance(eng, BraxVecEngine)
