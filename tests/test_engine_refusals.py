"""What the engines' Python front end refuses, and in which words, before anything is enqueued: every tensor argument of
the device entry points (``gae``, ``context_trace``, the PPO update and its statistics, the Adam step, the population
twins, the closed-loop launches) spoiled in every way its check can fail, and every keyword rule -- on fake engines whose
device is the CPU and whose library raises ``Launched`` where a call would have been enqueued.  The outcomes (exception
type and full message) are literals in engine_refusal_messages.py, recorded on the code as it stood before the layout
predicates of carl_amd/_tensors.py existed; the predicates' own edge cases are at the end of this file.

Left out, because the check sits behind a launch that needs a device:
- ``rollout_policy(..., gae=)``: the ``"advantage"`` / ``"return"`` buffers in ``out`` (``gae`` checks them after the
  closed-loop launch; ``gae``'s own cases cover the check);
- ``EvolutionStrategy.step``: what ``fitness_shaping`` returns (behind the evaluation launch);
- ``PopulationPPO.copy_members``: ``src`` (the constructor allocates on the device; test_gpu_population_ppo.py covers it).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import brax_policy_abi_util as U
import brax_policy_cases as BP
import engine_refusal_messages as M
import policy_cases as PC
from carl_amd import _lib, _tensors
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import InputStats, MLPPolicy

f32, f64, i32, i64, u8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
CPU = torch.device("cpu")


class Launched(Exception):
    """every check passed: the call reached the library function named here"""


class HostLib:
    """The library with its host-only helpers (sizes, counts, tables, the last error) and no launches"""
    _HOST = ("_rows", "_slabs", "_workgroups", "_floats", "_pitch", "_quantum", "_info", "_error")

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.endswith(self._HOST):
            return getattr(self._lib, name)

        def launch(*args):
            raise Launched(name)

        return launch


@pytest.fixture(autouse=True)
def no_launches(monkeypatch):
    """Nothing in this file reaches a launch, on a machine with a GPU either: every handle to the library is a
    ``HostLib``, and the device guard around a call is a no-op (the fake engines' device is the CPU)."""
    host = HostLib(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: host)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())


def _finish(eng, auto_reset):
    eng.b.flags = _lib.FLAG_AUTORESET if auto_reset else 0
    eng.b.n_contexts = eng.b.ctx_stride = 4
    eng.device, eng.lib, eng._b_ref, eng._stream = CPU, _lib.load(), C.byref(eng.b), lambda: 0
    eng.ctx_table = torch.zeros(8, 4)
    return eng


def classic(family=_lib.CARTPOLE, n=24, auto_reset=True):
    eng = PC.fake_engine(family)
    eng.n, eng.b = n, _lib.Batch()
    return _finish(eng, auto_reset)


def brax(n=8, auto_reset=True):
    eng = U.fake_brax_engine(auto_reset, n=n)
    eng.family, eng.info, eng._sys_ref, eng._tuned = -1, U.info(27, 8), C.byref(eng.sys), {}
    eng.sys_dev, eng.obs = torch.zeros(16, dtype=u8), torch.zeros(n, 27)
    return _finish(eng, auto_reset)


def classic_nets(eng, n_sets=None):
    rng, box = np.random.default_rng(0), not eng.info.action_is_discrete
    n_in = len(eng.ctx_obs_rows) + eng.D
    make = lambda: (MLPPolicy.for_env(eng, PC.rand_layers(rng, [n_in, 8, 1 if box else 2])),  # noqa: E731
                    MLPPolicy.for_env(eng, PC.rand_layers(rng, [n_in, 8, 1]), head="value"))
    if n_sets is None:
        return make()
    pairs = [make() for _ in range(n_sets)]
    return (MLPPolicy.stack([a for a, _ in pairs], eng.n // n_sets), MLPPolicy.stack([c for _, c in pairs], eng.n // n_sets))


def brax_nets():
    rng = np.random.default_rng(0)
    return U.ant_policy(rng), BraxMLPPolicy(U.info(27, 8), [], BP.make_layers(rng, 27, (8,), 1), "relu", head="value")


def z(*shape, dt=f32):
    return torch.zeros(shape, dtype=dt)


def rows(T, N, P, *tail, dt=f32):
    """[T, N] + tail rows of pitch P lanes"""
    return torch.zeros((T, P) + tail, dtype=dt)[:, :N]


# ---------------------------------------------------------------- the ways a tensor argument can be wrong
def spoils(t):
    """{name: a tensor that differs from the valid ``t`` in one respect}; the names say which"""
    s, out = tuple(t.shape), {}
    cast = lambda dt: torch.empty_strided(s, t.stride(), dtype=dt).zero_()  # noqa: E731
    out["dtype"] = cast(f64 if t.dtype != f64 else f32)
    if t.dtype == u8:
        out["bool"] = cast(torch.bool)
    out["device"] = torch.empty_strided(s, t.stride(), dtype=t.dtype, device="meta")
    out["rank"] = t[None]
    out["last_dim"] = torch.zeros(s[:-1] + (s[-1] + 1,), dtype=t.dtype)
    out["last_strided"] = torch.zeros(s[:-1] + (2 * s[-1],), dtype=t.dtype)[..., ::2]
    if s[0] > 1:
        out["fewer_rows"] = t[:-1]
    if t.dim() >= 2:
        per_lane = int(np.prod(s[2:], dtype=np.int64))
        pitch = t.stride(0) // per_lane if s[0] > 1 else s[1]
        make = lambda T, N, P: torch.zeros((T, P) + s[2:], dtype=t.dtype)[:, :N]  # noqa: E731
        out["more_rows"] = make(s[0] + 1, s[1], pitch)
        out["lanes"] = make(s[0], s[1] + 1, max(pitch, s[1] + 1))
        out["lane_strided"] = torch.zeros((s[0], 2 * pitch) + s[2:], dtype=t.dtype)[:, : 2 * s[1]: 2]
        out["pitch"] = make(s[0], s[1], s[1] + 16 if pitch == s[1] else s[1])
        out["pitch_zero"] = t[:1].expand(s)
    return out


def put(args, path, value):
    """``args`` with the entry at ``path`` replaced (``value`` is ``put`` itself: removed); containers on the way copied"""
    k, rest = path[0], path[1:]
    new = dict(args) if isinstance(args, dict) else list(args)
    if rest:
        new[k] = put(args[k], rest, value)
    elif value is put:
        del new[k]
    else:
        new[k] = value
    return new


def get(args, path):
    for k in path:
        args = args[k]
    return args


def outcome(fn, kw):
    try:
        fn(**kw)
    except Launched as e:
        return ("Launched", str(e))
    except Exception as e:  # noqa: BLE001 (the type is part of what is recorded)
        return (type(e).__name__, str(e))
    return ("returned", "")


def observe(spec, path):
    """{outcome: "the spoils that end in it, sorted"} of one argument of one spec"""
    fn, kw = SPECS[spec][0]()
    seen = {}
    variants = dict(spoils(get(kw, path)))
    if len(path) > 1 and isinstance(path[-1], str):
        variants["missing"] = put
    for name, bad in variants.items():
        seen.setdefault(outcome(fn, put(kw, path, bad)), []).append(name)
    return {k: " ".join(sorted(v)) for k, v in seen.items()}


# ---------------------------------------------------------------- the calls: name -> (() -> (method, valid keywords), paths)
T, P_ = 3, 32  # steps; lanes per padded row of the classic engine's 24


def _gae():
    e = classic()
    r = lambda dt=f32: rows(T, e.n, P_, dt=dt)  # noqa: E731
    return e.gae, dict(reward=r(), value=r(), terminated=r(u8), truncated=r(u8), last_value=z(e.n), gamma=0.99, lam=0.95,
                       boot_value=r(), out={"advantage": r(), "return": r()})


def _context_trace(make_eng, P):
    def make():
        e = make_eng()
        flags = lambda dt=u8: rows(T, e.n, P(e), dt=dt)  # noqa: E731
        return e.context_trace, dict(ctx_idx0=z(e.n, dt=i32), episode0=z(e.n, dt=i32), terminated=flags(), truncated=flags(),
                                     out=flags(i32))
    return make


def _ppo_grad(make_eng, nets, P, tail=(), adt=i32, n_ls=0):
    def make():
        e = make_eng()
        actor, critic = nets(e)
        N, p = e.n, P(e)
        buf = {"obs": rows(T, N, p, e.D), "action": rows(T, N, p, *tail, dt=adt), "log_prob": rows(T, N, p),
               "advantage": rows(T, N, p), "return": rows(T, N, p)}
        out = {"grad_actor": z(actor.set_floats), "grad_critic": z(critic.set_floats), "stats": z(6), "new_log_prob": z(5),
               "new_value": z(5)}
        if n_ls:
            out["grad_log_std"] = z(n_ls)
        return e.ppo_grad, dict(policy=actor, value_net=critic, buf=buf, obs0=z(N, e.D), context_id=rows(T, N, p, dt=i32),
                                idx=z(5, dt=i32), adv_norm=z(2), forward=True, out=out, workspace=z(64))
    return make


_PPO_GRAD_PATHS = [("buf", k) for k in ("obs", "action", "log_prob", "advantage", "return")] + [
    ("obs0",), ("context_id",), ("idx",), ("adv_norm",)] + [
    ("out", k) for k in ("grad_actor", "grad_critic", "stats", "new_log_prob", "new_value")]


def _ppo_grad_sets():
    e = classic(n=512)
    actor, critic = classic_nets(e, 2)
    N, p = e.n, 512
    buf = {"obs": rows(T, N, p, e.D), "action": rows(T, N, p, dt=i32), "log_prob": rows(T, N, p),
           "advantage": rows(T, N, p), "return": rows(T, N, p)}
    out = {"grad_actor": z(2, actor.set_floats), "grad_critic": z(2, critic.set_floats), "stats": z(2, 6)}
    return e.ppo_grad_sets, dict(policy=actor, value_net=critic, buf=buf, obs0=z(N, e.D), context_id=rows(T, N, p, dt=i32),
                                 idx=z(2, 5, dt=i32), hyper=z(2, _lib.PPO_HYPER, dt=f64), adv_norm=z(2, 2), out=out,
                                 workspace=z(64))


def _ppo_input_stats(make_eng, nets, P):
    def make():
        e = make_eng()
        N, p = e.n, P(e)
        slabs = int(e.lib.carl_ppo_input_stats_slabs(N, T))
        return e.ppo_input_stats, dict(policy=nets(e)[0], buf={"obs": rows(T, N, p, e.D)}, obs0=z(N, e.D),
                                       context_id=rows(T, N, p, dt=i32),
                                       out={"input_partial": z(slabs, 2, _lib.POLICY_MAX_IN, dt=f64), "steps": z(N, dt=i32)})
    return make


def _ppo_return_stats():
    e = classic()
    slabs = int(e.lib.carl_ppo_return_stats_slabs(e.n))
    r = lambda dt=f32: rows(T, e.n, P_, dt=dt)  # noqa: E731
    return e.ppo_return_stats, dict(reward=r(), terminated=r(u8), truncated=r(u8), ret=z(e.n), gamma=0.99, ret_rows=True,
                                    out={"return_partial": z(slabs, 2, dt=f64), "ret_rows": r()})


def _ppo_return_merge():
    return classic().ppo_return_merge, dict(partial=z(3, 2, dt=f64), n_b=72, scale=z(1),
                                            running={"count": z(1, dt=i64), "mean": z(1, dt=f64), "m2": z(1, dt=f64)})


def _adv_stats(sets, flat=False):
    def make():
        e = classic()
        adv = z(T * P_) if flat else rows(T, e.n, P_)
        if sets:
            return e.ppo_adv_stats_sets, dict(advantage=adv, idx=z(2, 12, dt=i32), batch_size=5, out=z(2, 3, 2))
        return e.ppo_adv_stats, dict(advantage=adv, idx=z(12, dt=i32), batch_size=5, out=z(3, 2))
    return make


def _adam(sets):
    def make():
        e = classic()
        lead = (2,) if sets else ()
        p = [z(*lead, 3), z(*lead, 2, 2)]
        g = [z(*lead, 3), z(*lead, 4)]
        st = e.adam_state(p, n_sets=2 if sets else None)
        kw = dict(params=p, grads=g, state=st, norm_out=z(*lead, 2, dt=f64))
        if sets:
            return e.adam_step_sets, dict(kw, hyper=z(2, _lib.PPO_HYPER, dt=f64))
        return e.adam_step, dict(kw, lr=3e-4)
    return make


_ADAM_PATHS = [("params", 0), ("params", 1), ("grads", 1), ("state", "m", 0), ("state", "v", 1), ("state", "step"),
               ("state", "beta_pow"), ("norm_out",)]


def _rollout_classic(family=_lib.CARTPOLE):
    def make():
        e = classic(family)
        actor, critic = classic_nets(e)
        out = e.alloc_rollout(T, final_obs=True)
        adt = i32 if e.info.action_is_discrete else f32
        out.update(action=rows(T, e.n, P_, dt=adt), log_prob=rows(T, e.n, P_), value=rows(T, e.n, P_),
                   boot_value=rows(T, e.n, P_), last_value=z(e.n))
        return e.rollout_policy, dict(policy=actor, n_steps=T, out=out, final_obs=True, deterministic=False, value_net=critic)
    return make


def _rollout_brax():
    e = brax()
    actor, critic = brax_nets()
    out = e.alloc_rollout(T, action=True)
    out.update(log_prob=z(T, e.n), value=z(T, e.n), boot_value=z(T, e.n), last_value=z(e.n))
    return e.rollout_policy, dict(policy=actor, n_steps=T, out=out, deterministic=False, value_net=critic)


def _summary(make_eng, nets):
    def make():
        e = make_eng()
        return e.rollout_policy, dict(policy=nets(e)[0], n_steps=T, mode="summary", out=e.alloc_policy_summary())
    return make


def _episodes(make_eng, nets, method, slabs):
    def make():
        e = make_eng()
        out = e.alloc_policy_episodes(2)
        out["input_partial"] = z(slabs(e, nets(e)[0]), 2, _lib.POLICY_MAX_IN, dt=f64)
        return getattr(e, method), dict(policy=nets(e)[0], n_episodes=2, max_steps=T, out=out, input_stats=True)
    return make


def _brax_slabs(e, pol):
    return int(e.lib.carl_brax_policy_stats_slabs(C.byref(e.b), C.byref(e.sys), C.byref(pol.struct(e.n, 0x10)), T))


def _input_stats_block():
    actor = classic_nets(classic())[0]
    st = InputStats(actor, "cpu")
    return st.update, dict(result={"input_partial": z(1, 2, _lib.POLICY_MAX_IN, dt=f64), "steps": z(24, dt=i32)},
                           policy_or_block=z(2, actor.set_floats), policy=actor, stream=0)


_EPISODE_PATHS = [("out", k) for k in ("episodes", "steps", "return", "length", "context_id", "terminated", "input_partial")]
_dense = lambda e: e.n  # noqa: E731
_padded = lambda e: P_  # noqa: E731
_bnets = lambda e: brax_nets()  # noqa: E731

SPECS = {
    "gae": (_gae, [("reward",), ("value",), ("terminated",), ("truncated",), ("last_value",), ("boot_value",),
                   ("out", "advantage"), ("out", "return")]),
    "context_trace": (_context_trace(classic, _padded),
                      [("ctx_idx0",), ("episode0",), ("terminated",), ("truncated",), ("out",)]),
    "context_trace/brax": (_context_trace(brax, _dense),
                           [("ctx_idx0",), ("episode0",), ("terminated",), ("truncated",), ("out",)]),
    "ppo_grad": (_ppo_grad(classic, classic_nets, _padded), _PPO_GRAD_PATHS),
    "ppo_grad/pendulum": (_ppo_grad(lambda: classic(_lib.PENDULUM), classic_nets, _padded, adt=f32, n_ls=1),
                          [("buf", "action"), ("out", "grad_log_std")]),
    "ppo_grad/brax": (_ppo_grad(brax, _bnets, _dense, tail=(8,), adt=f32, n_ls=8),
                      _PPO_GRAD_PATHS + [("out", "grad_log_std")]),
    "ppo_grad_sets": (_ppo_grad_sets, [("buf", "obs"), ("buf", "action"), ("obs0",), ("context_id",), ("idx",), ("hyper",),
                                       ("adv_norm",), ("out", "grad_actor"), ("out", "grad_critic"), ("out", "stats")]),
    "ppo_input_stats": (_ppo_input_stats(classic, classic_nets, _padded),
                        [("buf", "obs"), ("obs0",), ("context_id",), ("out", "input_partial"), ("out", "steps")]),
    "ppo_input_stats/brax": (_ppo_input_stats(brax, _bnets, _dense),
                             [("buf", "obs"), ("obs0",), ("context_id",), ("out", "input_partial"), ("out", "steps")]),
    "ppo_return_stats": (_ppo_return_stats, [("reward",), ("terminated",), ("truncated",), ("ret",),
                                             ("out", "return_partial"), ("out", "ret_rows")]),
    "ppo_return_merge": (_ppo_return_merge, [("partial",), ("running", "count"), ("running", "mean"), ("running", "m2"),
                                             ("scale",)]),
    "ppo_adv_stats": (_adv_stats(False), [("advantage",), ("idx",), ("out",)]),
    "ppo_adv_stats/flat": (_adv_stats(False, flat=True), [("advantage",)]),
    "ppo_adv_stats_sets": (_adv_stats(True), [("advantage",), ("idx",), ("out",)]),
    "ppo_adv_stats_sets/flat": (_adv_stats(True, flat=True), [("advantage",)]),
    "adam_step": (_adam(False), _ADAM_PATHS),
    "adam_step_sets": (_adam(True), _ADAM_PATHS + [("hyper",)]),
    "rollout_policy": (_rollout_classic(), [("out", k) for k in (
        "obs", "reward", "terminated", "truncated", "final_obs", "action", "log_prob", "value", "boot_value", "last_value")]),
    "rollout_policy/pendulum": (_rollout_classic(_lib.PENDULUM), [("out", "action")]),
    "rollout_policy/brax": (_rollout_brax, [("out", k) for k in (
        "obs", "reward", "terminated", "truncated", "action", "log_prob", "value", "boot_value", "last_value")]),
    "rollout_policy/summary": (_summary(classic, classic_nets), [("out", k) for k in ("episodes", "return_sum", "length_sum")]),
    "rollout_policy/brax/summary": (_summary(brax, _bnets), [("out", k) for k in ("episodes", "return_sum", "length_sum")]),
    "evaluate_policy": (_episodes(classic, classic_nets, "evaluate_policy",
                                  lambda e, pol: int(e.lib.carl_policy_stats_workgroups(e.n))), _EPISODE_PATHS),
    "evaluate_episodes": (_episodes(brax, _bnets, "evaluate_episodes", _brax_slabs), _EPISODE_PATHS),
    "InputStats.update": (_input_stats_block, [("policy_or_block",)]),
}
ARGUMENTS = [(spec, path) for spec, (_, paths) in SPECS.items() for path in paths]


@pytest.mark.parametrize("spec", list(SPECS))
def test_valid_arguments_reach_the_launch(spec):
    fn, kw = SPECS[spec][0]()
    assert outcome(fn, kw) == M.LAUNCHES[spec]


@pytest.mark.parametrize("spec,path", ARGUMENTS, ids=[f"{s}:{'.'.join(map(str, p))}" for s, p in ARGUMENTS])
def test_tensor_argument(spec, path):
    assert observe(spec, path) == M.TENSORS[spec][".".join(map(str, path))]


# ---------------------------------------------------------------- keyword rules and whatever else is no tensor layout
def _rp(eng_kind, auto_reset=True, **kw):
    """``rollout_policy`` of a fresh engine; ``value_net=True``: its matching critic"""
    e = classic(auto_reset=auto_reset) if eng_kind == "classic" else brax(auto_reset=auto_reset)
    actor, critic = classic_nets(e) if eng_kind == "classic" else brax_nets()
    if kw.get("value_net") is True:
        kw["value_net"] = critic
    if kw.get("policy") == "critic":
        kw["policy"] = critic
    kw.setdefault("policy", actor)
    return e.rollout_policy, dict(n_steps=T, **kw)


def _ev(eng_kind, auto_reset=True, n=None, **kw):
    e = classic(auto_reset=auto_reset) if eng_kind == "classic" else brax(auto_reset=auto_reset)
    actor = (classic_nets(e) if eng_kind == "classic" else brax_nets())[0]
    if n:
        e.n = n
    return (e.evaluate_policy if eng_kind == "classic" else e.evaluate_episodes), dict(policy=actor, **kw)


def _critic_with(**attrs):
    """``rollout_policy`` of a classic engine with a critic that differs from the actor's in ``attrs``"""
    e = classic()
    actor, critic = classic_nets(e)
    for k, v in attrs.items():
        setattr(critic, k, v)
    return e.rollout_policy, dict(policy=actor, n_steps=T, deterministic=False, value_net=critic)


def _shifted_critic(eng_kind):
    e = classic() if eng_kind == "classic" else brax()
    actor, critic = classic_nets(e) if eng_kind == "classic" else brax_nets()
    critic.params = critic.params.copy()
    critic.params[:, critic.weight_floats] += 1.0
    return e.rollout_policy, dict(policy=actor, n_steps=T, deterministic=False, value_net=critic)


def _sets_call(method, **kw):
    fn, base = SPECS[method][0]()
    return fn, dict(base, **kw)


def _population_mismatch():
    e = classic(n=512)
    actor, _ = classic_nets(e, 2)
    _, critic = classic_nets(e, 1)
    fn, base = _ppo_grad_sets()
    return e.ppo_grad_sets, dict(base, policy=actor, value_net=critic)


def _population_lanes():
    e = classic(n=768)
    fn, base = _ppo_grad_sets()
    return e.ppo_grad_sets, base


RULES = {}
for kind in ("classic", "brax"):
    sampled = dict(deterministic=False)
    RULES.update({
        f"rollout_policy/{kind}: gae without value_net": lambda k=kind: _rp(k, gae=(0.99, 0.95)),
        f"rollout_policy/{kind}: value_net in summary mode": lambda k=kind: _rp(k, value_net=True, mode="summary", **sampled),
        f"rollout_policy/{kind}: bootstrap_truncated without auto_reset":
            lambda k=kind: _rp(k, auto_reset=False, value_net=True, **sampled),
        f"rollout_policy/{kind}: no bootstrap without auto_reset launches":
            lambda k=kind: _rp(k, auto_reset=False, value_net=True, bootstrap_truncated=False, **sampled),
        f"rollout_policy/{kind}: deterministic valued": lambda k=kind: _rp(k, value_net=True),
        f"rollout_policy/{kind}: log_prob deterministic": lambda k=kind: _rp(k, log_prob=True),
        f"rollout_policy/{kind}: log_prob in summary mode": lambda k=kind: _rp(k, log_prob=True, mode="summary", **sampled),
        f"rollout_policy/{kind}: summary without auto_reset": lambda k=kind: _rp(k, auto_reset=False, mode="summary"),
        f"rollout_policy/{kind}: unknown mode": lambda k=kind: _rp(k, mode="episodes"),
        f"rollout_policy/{kind}: sampled with log_prob launches": lambda k=kind: _rp(k, log_prob=True, **sampled),
        f"rollout_policy/{kind}: summary launches": lambda k=kind: _rp(k, mode="summary"),
        f"rollout_policy/{kind}: valued with gae launches": lambda k=kind: _rp(k, value_net=True, gae=(0.99, 0.95), **sampled),
        f"rollout_policy/{kind}: gae of three values": lambda k=kind: _rp(k, value_net=True, gae=(0.9, 0.9, 0.9), **sampled),
        f"rollout_policy/{kind}: the actor as value_net": lambda k=kind: _rp(k, value_net=_rp(k)[1]["policy"], **sampled),
        f"rollout_policy/{kind}: a critic as policy": lambda k=kind: _rp(k, policy="critic", value_net=True, **sampled),
        f"rollout_policy/{kind}: value_net of another transform": lambda k=kind: _shifted_critic(k),
        f"rollout_policy/{kind}: out without action": lambda k=kind: _rp(k, out={}),
        f"evaluate/{kind}: without auto_reset": lambda k=kind: _ev(k, auto_reset=False, n_episodes=1, max_steps=4),
        f"evaluate/{kind}: no episodes": lambda k=kind: _ev(k, n_episodes=0, max_steps=4),
        f"evaluate/{kind}: negative steps": lambda k=kind: _ev(k, n_episodes=1, max_steps=-1),
        f"evaluate/{kind}: 2^31 records": lambda k=kind: _ev(k, n=1 << 20, n_episodes=1 << 11, max_steps=4),
        f"evaluate/{kind}: launches": lambda k=kind: _ev(k, n_episodes=2, max_steps=4),
        f"evaluate/{kind}: out without a key": lambda k=kind: _ev(k, n_episodes=2, max_steps=4, out={}),
        f"alloc_policy_episodes/{kind}: no episodes":
            lambda k=kind: ((classic() if k == "classic" else brax()).alloc_policy_episodes, dict(n_episodes=0)),
    })
RULES.update({
    "rollout_policy/classic: final_obs in summary mode": lambda: _rp("classic", final_obs=True, mode="summary"),
    "rollout_policy/classic: summary out without a key": lambda: _rp("classic", mode="summary", out={}),
    "rollout_policy/brax: summary out without a key": lambda: _rp("brax", mode="summary", out={}),
    "rollout_policy/classic: a Brax policy": lambda: _rp("classic", policy=brax_nets()[0]),
    "rollout_policy/brax: a classic policy": lambda: _rp("brax", policy=classic_nets(classic())[0]),
    "rollout_policy/brax: a classic critic": lambda: _rp("brax", value_net=classic_nets(classic())[1], deterministic=False),
    "rollout_policy/classic: value_net of another family": lambda: _critic_with(family=_lib.ACROBOT),
    "rollout_policy/classic: value_net of other context rows": lambda: _critic_with(ctx_rows=[0]),
    "rollout_policy/classic: value_net of another set layout": lambda: _critic_with(lanes_per_set=256),
    "adam_state: no sets": lambda: (classic().adam_state, dict(params=[z(2, 3)], n_sets=0)),
    "adam_state: a parameter without the sets axis": lambda: (classic().adam_state, dict(params=[z(2, 3), z(3)], n_sets=2)),
    "adam_step: no tensors": lambda: _sets_call("adam_step", params=[], grads=[]),
    "adam_step: five tensors": lambda: _sets_call("adam_step", params=[z(1)] * 5, grads=[z(1)] * 5),
    "adam_step: fewer gradients": lambda: _sets_call("adam_step", grads=[z(3)]),
    "adam_step_sets: no tensors": lambda: _sets_call("adam_step_sets", params=[], grads=[]),
    "adam_step_sets: five tensors": lambda: _sets_call("adam_step_sets", params=[z(2, 1)] * 5, grads=[z(2, 1)] * 5),
    "adam_step_sets: fewer gradients": lambda: _sets_call("adam_step_sets", grads=[z(2, 3)]),
    "adam_step_sets: params[0] a scalar": lambda: _sets_call("adam_step_sets", params=[z(), z(2, 2, 2)]),
    "adam_step_sets: params[1] of other sets": lambda: _sets_call("adam_step_sets", params=[z(2, 3), z(4, 1)]),
    "adam_step_sets: hyper no tensor": lambda: _sets_call("adam_step_sets", hyper=None),
    "ppo_adv_stats: batch_size 0": lambda: _sets_call("ppo_adv_stats", batch_size=0),
    "ppo_adv_stats_sets: batch_size 0": lambda: _sets_call("ppo_adv_stats_sets", batch_size=0),
    "ppo_adv_stats: a three-dimensional advantage": lambda: _sets_call("ppo_adv_stats", advantage=z(2, 3, 4)),
    "ppo_adv_stats_sets: an empty advantage": lambda: _sets_call("ppo_adv_stats_sets", advantage=z(0)),
    "ppo_grad: idx None and no adv_norm launch": lambda: _sets_call("ppo_grad", idx=None, adv_norm=None, forward=False, out=None),
    "ppo_grad_sets: more samples than a member has": lambda: _sets_call("ppo_grad_sets", idx=z(2, T * 256 + 1, dt=i32)),
    "ppo_grad_sets: idx no tensor": lambda: _sets_call("ppo_grad_sets", idx=None),
    "ppo_grad_sets: no adv_norm launches": lambda: _sets_call("ppo_grad_sets", adv_norm=None, out=None),
    "ppo_grad_sets: actor and critic of other sets": _population_mismatch,
    "ppo_grad_sets: sets that do not tile the lanes": _population_lanes,
    "ppo_grad: a buffer of other lanes": lambda: (lambda fn, kw: (classic(n=16).ppo_grad, kw))(*SPECS["ppo_grad"][0]()),
    "ppo_grad/brax: a classic policy": lambda: _sets_call("ppo_grad/brax", policy=classic_nets(classic())[0]),
    "ppo_input_stats: one step launches": lambda: (lambda e: (e.ppo_input_stats, dict(
        policy=classic_nets(e)[0], buf={"obs": z(5, e.n, e.D)[::5]}, obs0=z(e.n, e.D), context_id=z(5, e.n, dt=i32)[::5])))(classic()),
    "ppo_input_stats: a one-dimensional context_id": lambda: _sets_call("ppo_input_stats", context_id=z(24, dt=i32)),
    "ppo_input_stats: no steps": lambda: _sets_call("ppo_input_stats", context_id=z(0, 24, dt=i32)),
    "ppo_input_stats: more slabs than needed launch": lambda: (lambda fn, kw: (fn, put(kw, ("out", "input_partial"), torch.cat(
        [kw["out"]["input_partial"]] * 2))))(*SPECS["ppo_input_stats"][0]()),
    "ppo_return_stats: without ret_rows launches": lambda: _sets_call("ppo_return_stats", ret_rows=False, out=None),
    "ppo_return_merge: scale allocated launches": lambda: _sets_call("ppo_return_merge", scale=None),
    "ppo_workspace: no samples": lambda: (lambda e: (e.ppo_workspace, dict(zip(("policy", "value_net"), classic_nets(e)),
                                                                            n_samples=0)))(classic()),
    "gae: buffers allocated launch": lambda: _sets_call("gae", out=None, boot_value=None),
    "context_trace: out allocated launches": lambda: _sets_call("context_trace", out=None),
    "context_trace/brax: padded rows": lambda: (lambda e: (e.context_trace, dict(
        ctx_idx0=z(e.n, dt=i32), episode0=z(e.n, dt=i32), terminated=rows(T, e.n, 16, dt=u8),
        truncated=rows(T, e.n, 16, dt=u8))))(brax()),
    "InputStats.update: block no tensor": lambda: _sets_call("InputStats.update", policy_or_block=3.0),
    "InputStats.update: n_write beyond the block": lambda: _sets_call("InputStats.update", n_write=3),
})


@pytest.mark.parametrize("rule", list(RULES))
def test_rule(rule):
    assert outcome(*RULES[rule]()) == M.RULES[rule]


def test_allocators_and_the_shared_tables():
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.engine import LaneEngine, VecEngine

    for e in (classic(), brax()):
        s = e.alloc_policy_summary()
        assert {k: (t.dtype, tuple(t.shape)) for k, t in s.items()} == {
            "episodes": (i32, (e.n,)), "return_sum": (f32, (e.n,)), "length_sum": (i32, (e.n,))}
        assert all(int(t.abs().sum()) == 0 for t in s.values())
        ep = e.alloc_policy_episodes(3)
        assert {k: (t.dtype, tuple(t.shape)) for k, t in ep.items()} == {
            "episodes": (i32, (e.n,)), "steps": (i32, (e.n,)), "return": (f32, (3, e.n)), "length": (i32, (3, e.n)),
            "context_id": (i32, (3, e.n)), "terminated": (u8, (3, e.n))}
    assert BraxVecEngine._EPISODE_KEYS is VecEngine._EPISODE_KEYS
    e = classic()
    st = e.adam_state([z(3), z(2, 2)])
    assert [tuple(t.shape) for t in st["m"] + st["v"]] == [(3,), (2, 2)] * 2 and sorted(st) == ["beta_pow", "m", "step", "v"]
    assert (st["step"].dtype, st["step"].tolist(), st["beta_pow"].dtype, st["beta_pow"].tolist()) == (i64, [0], f64, [1.0, 1.0])
    st = e.adam_state([z(2, 3), z(2, 2, 2)], n_sets=2)
    assert [tuple(t.shape) for t in st["m"] + st["v"]] == [(2, 3), (2, 2, 2)] * 2
    assert (st["step"].dtype, st["step"].tolist(), st["beta_pow"].dtype, st["beta_pow"].tolist()) == (
        i64, [0, 0], f64, [[1.0, 1.0]] * 2)
    assert "gae" in LaneEngine.__dict__ and "gae" not in VecEngine.__dict__ and "gae" not in BraxVecEngine.__dict__


# ---------------------------------------------------------------- the layout predicates themselves, at and past their edges
def test_is_exact():
    ok = _tensors.is_exact
    t = z(3, 4)
    assert ok(t, CPU, f32, (3, 4)) and ok(t, CPU, f32, 12) and ok(t, CPU, f32, (None, 4)) and ok(t[None], CPU, f32, 12)
    assert ok(z(0, 4), CPU, f32, (None, 4)) and ok(z(1)[::2], CPU, f32, 1)  # no rows; one element is contiguous
    assert ok(z(3, 8)[:, ::2], CPU, f32, (3, 4), contiguous=False)
    for bad in (t.double(), z(3, 8)[:, ::2], z(4, 3).t(), z(3, 5), z(12), t[None], torch.empty(3, 4, device="meta"), None,
                t.numpy()):
        assert not ok(bad, CPU, f32, (3, 4)), bad
    assert not ok(z(3, 5), CPU, f32, (None, 4)) and not ok(z(4), CPU, f32, (None, 4)) and not ok(z(13), CPU, f32, 12)
    assert not ok(z(24)[::2], CPU, f32, 12) and not ok(t.double(), CPU, f32, 12, contiguous=False)


def test_is_rows():
    ok = _tensors.is_rows
    assert ok(rows(3, 5, 8), CPU, (f32,), 3, 5, 8) and ok(rows(3, 5, 5), CPU, (f32,), 3, 5, 5)  # P > N, P == N
    assert ok(rows(3, 5, 8, dt=torch.bool), CPU, (u8, torch.bool), 3, 5, 8)
    assert ok(rows(4, 5, 8), CPU, (f32,), 3, 5, 8, at_least=True) and not ok(rows(4, 5, 8), CPU, (f32,), 3, 5, 8)
    assert not ok(rows(2, 5, 8), CPU, (f32,), 3, 5, 8, at_least=True)
    assert ok(z(7, 9)[::7, :5], CPU, (f32,), 1, 5, 8)  # T == 1: any stride(0)
    assert not ok(z(7, 9)[::3, :5], CPU, (f32,), 3, 5, 8)  # T > 1: stride(0) is the pitch
    assert ok(z(3, 8, 4)[:, :1, 0], CPU, (f32,), 3, 1, 32)  # N == 1: any stride(1)
    assert not ok(z(3, 16)[:, :4:2], CPU, (f32,), 3, 2, 16)  # N > 1: unit stride
    assert ok(rows(3, 5, 8, 4), CPU, (f32,), 3, 5, 8, (4,)) and ok(rows(4, 5, 8, 4), CPU, (f32,), 3, 5, 8, (4,), at_least=True)
    assert ok(torch.empty_strided((3, 5, 1), (5, 1, 99)), CPU, (f32,), 3, 5, 5, (1,))  # a tail of size 1: any stride there
    assert not ok(z(3, 5, 4)[:, :, :1], CPU, (f32,), 3, 5, 20, (1,))  # (but its lanes lie one element apart)
    for bad in (rows(3, 5, 8, 4).double(), rows(3, 5, 9, 4), rows(3, 5, 8, 8)[..., ::2], rows(3, 5, 8, 5), rows(3, 5, 8),
                torch.empty_strided((3, 5, 4), (32, 4, 1), device="meta"), None):
        assert not ok(bad, CPU, (f32,), 3, 5, 8, (4,)), bad
    for bad in (rows(3, 5, 8).double(), rows(3, 5, 9), rows(3, 6, 8), rows(3, 5, 8)[None], z(5), None,
                torch.empty_strided((3, 5), (8, 1), device="meta")):
        assert not ok(bad, CPU, (f32,), 3, 5, 8), bad


def test_row_layout():
    assert _tensors.row_layout(rows(3, 5, 8)) == (3, 5, 8) and _tensors.row_layout(z(3, 5)) == (3, 5, 5)
    assert _tensors.row_layout(z(7, 9)[::7, :5]) == (1, 5, 5)  # one row leaves the pitch open: N
    assert _tensors.row_layout(z(1, 5).expand(3, 5)) == (3, 5, 0)  # (the caller refuses P < N)
    for bad in (z(5), z(3, 5, 2)):
        with pytest.raises(ValueError, match="unpack"):
            _tensors.row_layout(bad)


if __name__ == "__main__":  # python tests/test_engine_refusals.py > tests/engine_refusal_messages.py: record what the code does now
    import pprint

    host = HostLib(_lib.load())
    _lib.load = lambda: host
    torch.cuda.device = lambda d: contextlib.nullcontext()
    tensors = {}
    for spec_, path_ in ARGUMENTS:
        tensors.setdefault(spec_, {})[".".join(map(str, path_))] = observe(spec_, path_)
    print('"""The outcomes test_engine_refusals.py expects, as literals: (exception type, full message) -- ("Launched", the '
          'library\nfunction) where every check passed.  TENSORS maps each spoiled argument\'s outcomes to the spoils that end '
          'in them.\nWritten by ``python tests/test_engine_refusals.py``; review the diff of a regeneration like any other."""\n')
    for name_, value_ in (("LAUNCHES", {s: outcome(*SPECS[s][0]()) for s in SPECS}), ("TENSORS", tensors),
                          ("RULES", {k: outcome(*f()) for k, f in RULES.items()})):
        print(f"{name_} = " + pprint.pformat(value_, width=150, sort_dicts=False) + "\n")
