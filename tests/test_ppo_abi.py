"""The PPO update, C ABI on the host: the carl_ppo_batch_t / carl_ppo_out_t layouts against the header, every refusal of
carl_policy_context_trace and carl_ppo_grad by its message (validated before anything is enqueued, so they run without a
GPU), and the size functions.  CPU-only."""
import ctypes as C
import subprocess

import pytest

import ppo_ref as R
from carl_amd import _lib
from policy_cases import HEADER, c_batch, c_policy

PTR = 0x10000  # a 16-byte-aligned "device pointer" that is never dereferenced: every call here is refused first


@pytest.mark.parametrize("cls,name", [(_lib.PpoBatch, "carl_ppo_batch_t"), (_lib.PpoOut, "carl_ppo_out_t")])
def test_struct_layout_matches_c(tmp_path, cls, name):
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


# ---------------------------------------------------------------- carl_policy_context_trace
def trace(b, ctx0=PTR, ep0=PTR, te=PTR, tr=PTR, T=12, pitch=0, out=PTR):
    return _lib.load().carl_policy_context_trace(None if b is None else C.byref(b), ctx0, ep0, te, tr, T, pitch, out, None)


TRACE_REFUSALS = [
    (dict(b=None), b"batch is NULL"),
    (dict(b=c_batch(family=_lib.CARL_N_FAMILIES)), b"family 5 is a Brax family -- the PPO update covers the classic-control "
                                                    b"families only"),
    (dict(b=c_batch(family=-1)), b"unknown family -1"),
    (dict(b=c_batch(n=-1)), b"n_lanes -1 / n_steps 12 < 0"),
    (dict(b=c_batch(), T=-2), b"n_lanes 1000 / n_steps -2 < 0"),
    (dict(b=c_batch(n_contexts=0)), b"n_contexts 0 < 1"),
    (dict(b=c_batch(selector=9)), b"unknown selector 9"),
    (dict(b=c_batch(), pitch=999), b"row_pitch 999 < n_lanes 1000"),
    (dict(b=c_batch(), ctx0=None), b"a required pointer is NULL"),
    (dict(b=c_batch(), ep0=None), b"a required pointer is NULL"),
    (dict(b=c_batch(), te=None), b"a required pointer is NULL"),
    (dict(b=c_batch(), tr=None), b"a required pointer is NULL"),
    (dict(b=c_batch(), out=None), b"a required pointer is NULL"),
]


@pytest.mark.parametrize("kw,msg", TRACE_REFUSALS, ids=[str(i) for i in range(len(TRACE_REFUSALS))])
def test_context_trace_refusals(kw, msg):
    assert trace(**kw) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().carl_last_error() == b"carl_policy_context_trace: " + msg


def test_context_trace_without_work_enqueues_nothing():
    assert trace(c_batch(n=0)) == 0 and trace(c_batch(), T=0) == 0


# ---------------------------------------------------------------- carl_ppo_grad
def critic(**kw):
    return c_policy(**{**dict(n_out=1, head=_lib.POLICY_HEAD_BOX), **kw})


def ppo_batch(**kw):
    """a valid carl_ppo_batch_t for c_policy() (CartPole, 1000 lanes x 4 steps in rows of 1008, every sample)"""
    b = _lib.PpoBatch()
    b.family, b.n_lanes, b.n_steps, b.row_pitch, b.obs_dim = _lib.CARTPOLE, 1000, 4, 1008, 4
    b.n_contexts, b.ctx_stride, b.action_dtype, b.n_samples = 4, 4, _lib.ACTION_I32, 4000
    b.clip_range, b.vf_coef, b.ent_coef = 0.2, 0.5, 0.0
    for f in ("obs0", "obs", "context_id", "ctx_table", "action", "log_prob", "advantage", "ret"):
        setattr(b, f, PTR)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def ppo_out(pol=None, crit=None, M=4000, **kw):
    o = _lib.PpoOut()
    o.grad_actor = o.grad_critic = o.grad_log_std = o.stats = o.workspace = PTR
    o.workspace_floats = _lib.load().carl_ppo_workspace_floats(C.byref(pol or c_policy()), C.byref(crit or critic()), M)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def grad(b=None, pol=None, crit=None, log_std=PTR, out=None):
    b, pol, crit = b or ppo_batch(), pol or c_policy(), crit or critic()
    out = out or ppo_out(pol, crit, max(b.n_samples, 1))
    return _lib.load().carl_ppo_grad(C.byref(b), C.byref(pol), C.byref(crit), log_std, C.byref(out), None)


def pendulum(**kw):
    return ppo_batch(**{**dict(family=_lib.PENDULUM, obs_dim=3, action_dtype=_lib.ACTION_F32), **kw})


def pendulum_nets():
    kw = dict(n_in=5)
    return c_policy(n_out=1, head=_lib.POLICY_HEAD_BOX, **kw), critic(**kw)


GRAD_REFUSALS = [
    (dict(b=ppo_batch(family=_lib.CARL_N_FAMILIES)), b"carl_ppo_grad: family 5 is a Brax family -- the PPO update covers the "
                                                      b"classic-control families only"),
    (dict(b=ppo_batch(n_lanes=0)), b"carl_ppo_grad: n_lanes 0 / n_steps 4 < 1"),
    (dict(b=ppo_batch(n_steps=0)), b"carl_ppo_grad: n_lanes 1000 / n_steps 0 < 1"),
    (dict(b=ppo_batch(row_pitch=999)), b"carl_ppo_grad: row_pitch 999 < n_lanes 1000"),
    (dict(b=ppo_batch(obs_dim=3)), b"carl_ppo_grad: obs_dim 3, the family's is 4"),
    (dict(pol=c_policy(n_hidden=3)), b"carl_ppo_grad: n_hidden 3 outside [0, 2]"),
    (dict(pol=c_policy(width=(65, 64))), b"carl_ppo_grad: hidden width[0] = 65 outside [1, 64]"),
    (dict(pol=c_policy(ctx_rows=(0, 8))), b"carl_ppo_grad: ctx_rows[1] = 8 is not a context-table row (F = 8)"),
    (dict(pol=c_policy(n_in=7)), b"carl_ppo_grad: n_in 7 != n_ctx 2 + obs_dim 4"),
    (dict(pol=c_policy(n_out=3)), b"carl_ppo_grad: head width 3, the family needs 2 (n_actions)"),
    (dict(pol=c_policy(activation=7)), b"carl_ppo_grad: unknown activation 7"),
    (dict(pol=c_policy(n_sets=2)), b"carl_ppo_grad: n_sets 2, a gradient step has one weight set (several are evolution "
                                   b"strategies' territory)"),
    (dict(pol=c_policy(params=None)), b"carl_ppo_grad: params is NULL"),
    (dict(pol=c_policy(head=_lib.POLICY_HEAD_BOX)), b"carl_ppo_grad: head kind 1 does not match the family's action space"),
    (dict(crit=critic(n_out=2)), b"carl_ppo_grad: critic: head width 2, the family needs 1 (a value network has 1)"),
    (dict(crit=critic(n_sets=3)), b"carl_ppo_grad: critic: n_sets 3, a gradient step has one weight set (several are "
                                  b"evolution strategies' territory)"),
    (dict(crit=critic(width=(64, 0))), b"carl_ppo_grad: critic: hidden width[1] = 0 outside [1, 64]"),
    (dict(crit=critic(n_in=5, n_ctx=1)), b"carl_ppo_grad: critic: n_ctx 1, the actor has 2 (the critic reads the actor's "
                                         b"inputs)"),
    (dict(crit=critic(ctx_rows=(0, 2))), b"carl_ppo_grad: critic: ctx_rows[1] = 2, the actor's is 3"),
    (dict(crit=critic(params=None)), b"carl_ppo_grad: critic: params is NULL"),
    (dict(b=ppo_batch(action_dtype=_lib.ACTION_F32)), b"carl_ppo_grad: the action column is int32 (CARL_ACTION_I32) for this "
                                                       b"family"),
    (dict(b=pendulum(action_dtype=_lib.ACTION_I32), pend=True), b"carl_ppo_grad: the action column is float32 "
                                                                 b"(CARL_ACTION_F32) for this family"),
    (dict(b=ppo_batch(n_contexts=0)), b"carl_ppo_grad: n_contexts 0 / ctx_stride 4 invalid"),
    (dict(b=ppo_batch(ctx_stride=3)), b"carl_ppo_grad: n_contexts 4 / ctx_stride 3 invalid"),
    (dict(b=ppo_batch(n_samples=0, idx=PTR)), b"carl_ppo_grad: n_samples 0 < 1"),
    (dict(b=ppo_batch(n_samples=4001, idx=PTR)), b"carl_ppo_grad: n_samples 4001 > n_steps 4 x n_lanes 1000"),
    (dict(b=ppo_batch(n_samples=3999)), b"carl_ppo_grad: idx is NULL (every sample) but n_samples 3999 != n_steps 4 x n_lanes "
                                        b"1000"),
    (dict(b=ppo_batch(clip_range=-0.1)), b"carl_ppo_grad: clip_range -0.1 is not finite and >= 0"),
    (dict(b=ppo_batch(clip_range=float("nan"))), b"carl_ppo_grad: clip_range nan is not finite and >= 0"),
    (dict(b=ppo_batch(vf_coef=float("inf"))), b"carl_ppo_grad: vf_coef inf is not finite and >= 0"),
    (dict(b=ppo_batch(ent_coef=-1.0)), b"carl_ppo_grad: ent_coef -1 is not finite and >= 0"),
    (dict(b=ppo_batch(obs0=None)), b"carl_ppo_grad: a required pointer of ppo is NULL (all but idx and adv_norm)"),
    (dict(b=ppo_batch(context_id=None)), b"carl_ppo_grad: a required pointer of ppo is NULL (all but idx and adv_norm)"),
    (dict(out=ppo_out(stats=None)), b"carl_ppo_grad: out->grad_actor, out->grad_critic and out->stats are required"),
    (dict(out=ppo_out(grad_critic=None)), b"carl_ppo_grad: out->grad_actor, out->grad_critic and out->stats are required"),
    (dict(b=pendulum(), pend=True, log_std=None), b"carl_ppo_grad: a Box family needs log_std and out->grad_log_std ([1] on "
                                                  b"the device)"),
    (dict(out=ppo_out(workspace=None)), b"carl_ppo_grad: out->workspace is NULL or not on a 16-byte boundary"),
    (dict(out=ppo_out(workspace=PTR + 4)), b"carl_ppo_grad: out->workspace is NULL or not on a 16-byte boundary"),
]


@pytest.mark.parametrize("kw,msg", GRAD_REFUSALS, ids=[str(i) for i in range(len(GRAD_REFUSALS))])
def test_ppo_grad_refusals(kw, msg):
    kw = dict(kw)
    if kw.pop("pend", False):
        kw["pol"], kw["crit"] = pendulum_nets()
    assert grad(**kw) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().carl_last_error() == msg


def test_ppo_grad_refuses_null_structs_and_a_small_workspace():
    lib = _lib.load()
    b, pol, crit, out = ppo_batch(), c_policy(), critic(), ppo_out()
    for args in ((None, C.byref(pol), C.byref(crit), PTR, C.byref(out)), (C.byref(b), None, C.byref(crit), PTR, C.byref(out)),
                 (C.byref(b), C.byref(pol), None, PTR, C.byref(out)), (C.byref(b), C.byref(pol), C.byref(crit), PTR, None)):
        assert lib.carl_ppo_grad(*args, None) == _lib.ERR_INVALID_ARGUMENT
        assert lib.carl_last_error() == b"carl_ppo_grad: ppo / policy / critic / out is NULL"
    need = out.workspace_floats
    assert grad(out=ppo_out(workspace_floats=need - 1)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == (b"carl_ppo_grad: workspace of %d floats, %d needed (carl_ppo_workspace_floats)"
                                     % (need - 1, need))
    # a Box family without out->grad_log_std
    pol, crit = pendulum_nets()
    assert grad(b=pendulum(), pol=pol, crit=crit, out=ppo_out(pol, crit, grad_log_std=None)) == _lib.ERR_INVALID_ARGUMENT
    assert b"a Box family needs log_std and out->grad_log_std" in lib.carl_last_error()


def test_size_functions():
    lib = _lib.load()
    TS = lib.carl_ppo_tile()
    assert TS == R.TILE
    assert [lib.carl_ppo_grad_workgroups(m) for m in (-1, 0, 1, TS, TS + 1, 2 * TS + 3)] == [0, 0, 1, 1, 2, 3]
    cap = R.WORKGROUPS_CAP
    assert lib.carl_ppo_grad_workgroups(cap * TS) == cap == lib.carl_ppo_grad_workgroups(cap * TS + 1)
    assert lib.carl_ppo_grad_workgroups(65536 * 128) == cap  # full size: the partials stay in the low tens of MB
    pol, crit = c_policy(), critic()
    full = lib.carl_ppo_workspace_floats(C.byref(pol), C.byref(crit), 65536 * 128)
    assert 0 < full * 4 < 32 << 20
    one = lib.carl_ppo_workspace_floats(C.byref(pol), C.byref(crit), 1)
    assert full == cap * one and lib.carl_ppo_workspace_floats(C.byref(pol), C.byref(crit), 2 * TS + 3) == 3 * one
    # a slab holds every parameter of both networks
    assert one >= lib.carl_policy_set_floats(C.byref(pol)) + lib.carl_policy_set_floats(C.byref(crit)) - 2 * (2 * 6 + 4)
    # a smaller shape needs less
    lin = lib.carl_ppo_workspace_floats(C.byref(c_policy(n_hidden=0)), C.byref(critic(n_hidden=0)), 1)
    assert 0 < lin < one
    assert lib.carl_ppo_workspace_floats(C.byref(c_policy(n_hidden=3)), C.byref(crit), 1) == -1
    assert lib.carl_ppo_workspace_floats(C.byref(pol), C.byref(crit), 0) == -1
    assert lib.carl_ppo_workspace_floats(None, C.byref(crit), 1) == -1
