"""Host side of the closed-loop rollout's critic and of GAE (no GPU): the value head of MLPPolicy, every refusal of
rollout_policy(value_net=..., gae=...) and of the two C entry points, the header <-> ctypes layouts, and the fp32 GAE
restatement (value_cases.gae_ref, the reference of test_gpu_gae.py) against a float64 SB3-formula loop."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import value_cases as VC
from carl_amd import _lib
from carl_amd.policy import MLPPolicy
from policy_cases import (HEADER, SAMPLING_LOG_PROB_REQUIRED, SAMPLING_LOG_PROB_UNALIGNED, SAMPLING_LOG_STD, c_batch, c_io,
                          c_policy, check_first_of_two, fake_engine, rand_layers)


def fake(family=_lib.CARTPOLE, auto_reset=True):
    eng = fake_engine(family)
    eng.b = _lib.Batch()
    eng.b.flags = _lib.FLAG_AUTORESET if auto_reset else 0
    return eng


def pair(eng, rng, a_widths=(8,), c_widths=(5,), **ckw):
    n_in = eng.F + eng.D
    n_out = int(eng.info.n_actions) if eng.info.action_is_discrete else 1
    actor = MLPPolicy.for_env(eng, rand_layers(rng, [n_in, *a_widths, n_out]), "tanh")
    critic = MLPPolicy.for_env(eng, rand_layers(rng, [n_in, *c_widths, 1]), "relu", head="value", **ckw)
    return actor, critic


def test_value_network_packs_one_output_for_every_family():
    rng = np.random.default_rng(0)
    for fam in (_lib.CARTPOLE, _lib.PENDULUM, _lib.ACROBOT, _lib.MOUNTAINCAR, _lib.MOUNTAINCAR_CONT):
        eng = fake(fam)
        _, c = pair(eng, rng, c_widths=(7, 3))
        assert c.head == "value" and c.n_out == 1 and c.widths == [7, 3]
        s = c.struct(1000, 0x1000)
        assert (s.n_out, s.n_hidden, s.width[0], s.width[1], s.head) == (1, 2, 7, 3, _lib.POLICY_HEAD_BOX)
        assert c.params.shape == (1, _lib.load().carl_policy_set_floats(C.byref(s)))
        W, b = c.layers[-1]
        off = sum(w.size + v.size for w, v in c.layers[:-1])
        np.testing.assert_array_equal(c.params[0, off: off + W.size + 1], np.concatenate([W.reshape(-1), b]))
        np.testing.assert_array_equal(c.transform_section()[0], np.concatenate([c.shift, c.scale, [c.clip]]))
    eng = fake(_lib.CARTPOLE)
    n_in = eng.F + eng.D
    with pytest.raises(ValueError, match="head width 2"):
        MLPPolicy.for_env(eng, rand_layers(rng, [n_in, 2]), head="value")
    with pytest.raises(ValueError, match="head width 1"):
        MLPPolicy.for_env(eng, rand_layers(rng, [n_in, 1]))  # the default is still a policy head
    with pytest.raises(ValueError, match="head 'critic'"):
        MLPPolicy.for_env(eng, rand_layers(rng, [n_in, 1]), head="critic")
    with pytest.raises(ValueError, match="log_std"):
        MLPPolicy.for_env(fake(_lib.PENDULUM), rand_layers(rng, [10, 1]), head="value", log_std=0.0)


def test_value_head_through_from_sequential_and_stack():
    import torch

    eng = fake(_lib.ACROBOT)
    n_in = eng.F + eng.D
    seq = torch.nn.Sequential(torch.nn.Linear(n_in, 6), torch.nn.Tanh(), torch.nn.Linear(6, 1))
    c = MLPPolicy.from_sequential(eng, seq, head="value")
    assert c.head == "value" and c.n_out == 1 and c.activation == "tanh"
    with pytest.raises(ValueError, match="head width 1"):
        MLPPolicy.from_sequential(eng, seq)
    st = MLPPolicy.stack([c, MLPPolicy.from_sequential(eng, seq, head="value")], 256, head="value")
    assert st.head == "value" and st.n_sets == 2 and st.transform_section().shape == (2, 2 * n_in + 1)
    with pytest.raises(ValueError, match="head='policy'"):
        MLPPolicy.stack([c], 256, head="policy")
    a = MLPPolicy.for_env(eng, rand_layers(np.random.default_rng(1), [n_in, 6, 3]))
    with pytest.raises(ValueError, match="same family"):
        MLPPolicy.stack([a, c], 256)


def test_rollout_policy_refuses_before_any_launch():
    rng = np.random.default_rng(2)
    eng = fake()
    a, c = pair(eng, rng)
    with pytest.raises(ValueError, match="gae=.*needs value_net"):
        eng.rollout_policy(a, 4, gae=(0.99, 0.95))
    with pytest.raises(ValueError, match="transitions mode only"):
        eng.rollout_policy(a, 4, mode="summary", value_net=c)
    with pytest.raises(ValueError, match="head='value'"):
        eng.rollout_policy(a, 4, value_net=a)
    other = fake(_lib.MOUNTAINCAR)
    with pytest.raises(ValueError, match="family"):
        eng.rollout_policy(a, 4, value_net=pair(other, rng)[1])
    n_in = eng.F + eng.D
    fewer = MLPPolicy.for_env(eng, rand_layers(rng, [n_in - 1, 1]), head="value", context_features=list(range(eng.F - 1)))
    with pytest.raises(ValueError, match="context rows"):
        eng.rollout_policy(a, 4, value_net=fewer)
    with pytest.raises(ValueError, match="one set layout"):
        eng.rollout_policy(a, 4, value_net=MLPPolicy.stack([c, c], 512))
    with pytest.raises(ValueError, match="bit for bit"):
        eng.rollout_policy(a, 4, value_net=pair(eng, rng, input_clip=5.0)[1])
    with pytest.raises(ValueError, match="bit for bit"):  # -0 is not +0
        eng.rollout_policy(a, 4, value_net=pair(eng, rng, input_shift=-np.zeros(n_in, np.float32))[1])
    off = fake(auto_reset=False)
    with pytest.raises(ValueError, match="bootstrap_truncated=True needs auto_reset"):
        off.rollout_policy(a, 4, value_net=c)


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    b, p = c_batch(), c_policy()
    b.flags = 0
    io = _lib.StepIO()
    for f in ("action", "obs", "reward", "terminated", "truncated"):
        setattr(io, f, 0x3000)
    io.action_dtype, io.row_pitch = _lib.ACTION_I32, 1008

    def crit(**kw):
        c = c_policy(n_out=1, head=_lib.POLICY_HEAD_BOX, width=(16, 8), activation=_lib.POLICY_RELU)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def call(c=None, out=None, io_=io, smp=None):
        c = crit() if c is None else c
        out = _lib.PolicyValue(0x4000, 0x5000, None) if out is None else out
        return lib.carl_rollout_policy_valued(C.byref(b), C.byref(p), C.byref(c), smp, None if io_ is None else C.byref(io_),
                                              4, None, C.byref(out), None), lib.carl_last_error()

    for kw, msg in [(dict(io_=None), b"transitions mode only"), (dict(c=crit(n_out=2)), b"a value network has 1"),
                    (dict(c=crit(n_in=5)), b"the actor has 6 / 2"), (dict(c=crit(n_hidden=3)), b"critic: n_hidden 3"),
                    (dict(c=crit(lanes_per_set=2048)), b"the actor has 1 x 1024"), (dict(c=crit(params=None)), b"critic: params"),
                    (dict(c=crit(activation=7)), b"critic: unknown activation"),
                    (dict(out=_lib.PolicyValue(0x4000, None, None)), b"out->last_value are required"),
                    (dict(smp=C.byref(_lib.PolicySampling(1, None, None))), b"sampling->log_prob is NULL")]:
        code, err = call(**kw)
        assert code == -1 and msg in err, (kw, err)
    c2 = crit()
    c2.ctx_rows[1] = 2
    code, err = call(c=c2)
    assert code == -1 and b"ctx_rows[1] = 2, the actor's is 3" in err
    for out, msg in [(_lib.PolicyValue(0x4004, 0x5000, None), b"16-byte"), (_lib.PolicyValue(0x4000, 0x5000, 0x6000), b"CARL_FLAG_AUTORESET")]:
        code, err = call(out=out)
        assert code == -2 and msg in err, err  # CARL_ERR_UNSUPPORTED

    g = _lib.Gae()
    assert lib.carl_gae(None, None) == -1
    g.n_lanes, g.n_steps = 4, -1
    assert lib.carl_gae(C.byref(g), None) == -1 and b"n_steps -1" in lib.carl_last_error()
    g.n_steps, g.row_pitch = 3, 2
    assert lib.carl_gae(C.byref(g), None) == -1 and b"row_pitch 2 < n_lanes 4" in lib.carl_last_error()
    g.row_pitch = 0
    assert lib.carl_gae(C.byref(g), None) == -1 and b"required pointer" in lib.carl_last_error()
    g.n_lanes = 0
    for f in ("reward", "value", "last_value", "terminated", "truncated", "advantage", "ret"):
        setattr(g, f, 0x1000)
    assert lib.carl_gae(C.byref(g), None) == 0  # nothing to do: nothing enqueued


def test_valued_entry_point_words_the_shared_checks_as_before_and_in_their_order():
    """the whole message of the checks the critic shares with the actor and of the sampling checks, and which of two
    spoilt arguments answers"""
    lib = _lib.load()
    who = b"carl_rollout_policy_valued: "
    S = _lib.PolicySampling

    def crit(n_in=6, **kw):
        c = c_policy(n_in=n_in, n_out=1, head=_lib.POLICY_HEAD_BOX, width=(16, 8), activation=_lib.POLICY_RELU)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def call(b, p, c, smp=None, io="default", out="default"):
        io = c_io() if io == "default" else io
        out = _lib.PolicyValue(0x4000, 0x5000, None) if out == "default" else out
        return lib.carl_rollout_policy_valued(C.byref(b), C.byref(p), None if c is None else C.byref(c),
                                              None if smp is None else C.byref(smp), None if io is None else C.byref(io),
                                              4, None, None if out is None else C.byref(out), None)

    b, p = c_batch(), c_policy()
    wide = crit()
    wide.width[0] = 65
    for c, msg in [(crit(n_hidden=3), b"critic: n_hidden 3 outside [0, 2]"),
                   (wide, b"critic: hidden width[0] = 65 outside [1, 64]"),
                   (crit(activation=7), b"critic: unknown activation 7"),
                   (crit(params=None), b"critic: params is NULL"),
                   # two at once: the critic's checks in their order
                   (crit(n_hidden=3, n_out=2), b"critic: n_hidden 3 outside [0, 2]"),
                   (crit(n_out=2, n_in=5), b"critic: head width 2, a value network has 1"),
                   (crit(n_in=5, activation=7), b"critic: n_in 5 / n_ctx 2, the actor has 6 / 2 (the critic reads the "
                                                b"actor's inputs)"),
                   (crit(activation=7, lanes_per_set=2048), b"critic: unknown activation 7"),
                   (crit(activation=7, params=None), b"critic: unknown activation 7"),
                   (crit(lanes_per_set=2048, params=None), b"critic: 1 sets x 2048 lanes, the actor has 1 x 1024"),
                   (None, b"critic is NULL")]:
        assert call(b, p, c, out=None) == _lib.ERR_INVALID_ARGUMENT  # (the critic before the value outputs)
        assert lib.carl_last_error() == who + msg
    # io NULL answers before a bad critic, a NULL batch / policy before that, the actor's own checks after it
    assert call(b, p, crit(n_hidden=3), io=None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == who + b"io is NULL -- transitions mode only (a summary has no use for values)"
    assert lib.carl_rollout_policy_valued(None, C.byref(p), None, None, None, 4, None, None, None) == -1
    assert lib.carl_last_error() == who + b"batch / policy is NULL"
    # the sampling checks: after the actor's, before the critic's; log_std, then the required column, then its alignment
    bp = c_batch(family=_lib.PENDULUM)
    pp, cp, io_f = c_policy(n_in=5, n_out=1, head=_lib.POLICY_HEAD_BOX), crit(n_in=5), c_io(action_dtype=_lib.ACTION_F32)
    for smp, code, msg in [(S(1, None, 0x4004), -1, SAMPLING_LOG_STD), (S(1, None, None), -1, SAMPLING_LOG_STD),
                           (S(1, 0x6000, None), -1, SAMPLING_LOG_PROB_REQUIRED),
                           (S(1, 0x6000, 0x4004), _lib.ERR_UNSUPPORTED, SAMPLING_LOG_PROB_UNALIGNED)]:
        assert call(bp, pp, crit(n_in=5, n_hidden=3), smp, io_f) == code
        assert lib.carl_last_error() == who + msg
    assert call(b, p, None, S(1, None, None)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == who + SAMPLING_LOG_PROB_REQUIRED
    assert call(bp, pp, cp, S(1, None, None), c_io(action_dtype=_lib.ACTION_F32, row_pitch=999)) == -1
    assert lib.carl_last_error() == who + b"io.row_pitch 999 < n_lanes 1000"
    for smp in (None, S(1, None, 0x4004)):
        check_first_of_two(who[:-2], lambda b, p: call(b, p, crit(n_hidden=3), smp, out=None))


def test_rollout_policy_refuses_bad_columns_in_their_order():
    """the dtype and row refusals of the per-step columns, whole, and which of two bad columns answers: the launch's
    own buffers (action first), then log_prob, then every critic column's dtype before any critic column's rows"""
    import torch

    rng = np.random.default_rng(3)
    eng = fake()
    eng.device = torch.device("cpu")
    a, c = pair(eng, rng)
    T, n, P = 4, eng.n, 1008

    def col(dtype=torch.float32, rows=T, pitch=P):
        return torch.empty((rows, pitch), dtype=dtype)[:, :n]

    def out(**kw):
        o = {"obs": torch.empty((T, P, eng.D))[:, :n], "reward": col(), "terminated": col(torch.uint8),
             "truncated": col(torch.uint8), "action": col(torch.int32)}
        o.update(kw)
        return o

    def rows(k, t):
        return (f"rollout_policy output '{k}': shape {tuple(t.shape)} / strides {tuple(t.stride())} do not form "
                f"[>= {T}, {n}] rows of one common pitch ({P} lanes)")

    short, dense, f64 = col(rows=T - 1), col(pitch=n), col(torch.float64)
    cases = [
        (dict(deterministic=False, log_prob=True), out(action=col(torch.int64), log_prob=f64),
         "rollout_policy 'action' buffer must be torch.int32 for this family"),
        (dict(deterministic=False, log_prob=True), out(action=col(torch.int32, pitch=n), log_prob=f64),
         rows("action", col(torch.int32, pitch=n))),
        (dict(deterministic=False, log_prob=True), out(log_prob=f64), "rollout_policy 'log_prob' buffer must be torch.float32"),
        (dict(deterministic=False, log_prob=True), out(log_prob=short), rows("log_prob", short)),
        (dict(deterministic=False, log_prob=True), out(log_prob=dense), rows("log_prob", dense)),
        (dict(deterministic=False, value_net=c), out(log_prob=f64, value=f64),
         "rollout_policy 'log_prob' buffer must be torch.float32"),
        (dict(value_net=c), out(log_prob=f64, value=f64), "rollout_policy 'value' buffer must be torch.float32"),
        (dict(value_net=c), out(value=short, boot_value=f64), "rollout_policy 'boot_value' buffer must be torch.float32"),
        (dict(value_net=c), out(value=short, boot_value=dense), rows("value", short)),
        (dict(value_net=c), out(value=col(), boot_value=dense), rows("boot_value", dense)),
        (dict(value_net=c, bootstrap_truncated=False), out(value=dense, boot_value=f64), rows("value", dense)),
        (dict(value_net=c), out(value=col(), boot_value=col(), last_value=torch.empty(n, dtype=torch.float64)),
         f"rollout_policy 'last_value' must be a contiguous float32 [{n}] tensor on cpu"),
    ]
    for kw, o, msg in cases:
        with pytest.raises(ValueError) as e:
            eng.rollout_policy(a, T, out=o, **kw)
        assert str(e.value) == msg, (kw, str(e.value))


def test_new_struct_layouts_match_the_header(tmp_path):
    structs = {"carl_policy_value_t": _lib.PolicyValue, "carl_gae_t": _lib.Gae}
    c_name = {"lam": "lambda"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    want = []
    for name, cls in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        want.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({name}, {c_name.get(f, f)}));')
            want.append(getattr(cls, f).offset)
    lines.append("return 0;}")
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == want


@pytest.mark.parametrize("boot", [False, True])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_fp32_gae_rule_is_sb3s_within_the_recurrence_bound(gamma, lam, boot):
    rng = np.random.default_rng(int(gamma * 100) + boot)
    d = VC.random_gae_inputs(rng, 64, 200)
    bv = d.pop("boot_value") if boot else d.pop("boot_value") * 0
    adv, ret = VC.gae_ref(**d, gamma=gamma, lam=lam, boot_value=bv if boot else None)
    a64, r64, ea, er = VC.gae_sb3_f64(**d, gamma=gamma, lam=lam, boot_value=bv if boot else None)
    assert (d["terminated"] & d["truncated"]).any() and (d["truncated"] & ~d["terminated"]).any()
    assert np.all(np.abs(adv - a64) <= ea), np.max(np.abs(adv - a64) / ea)
    assert np.all(np.abs(ret - r64) <= er), np.max(np.abs(ret - r64) / er)
    assert np.max(np.abs(adv - a64) / ea) > 1e-3  # the bound is of the error's order, not a blank cheque


def test_gae_rule_selects_do_not_leak_masked_values():
    rng = np.random.default_rng(9)
    d = VC.random_gae_inputs(rng, 6, 8)
    d["terminated"][:] = 0
    d["truncated"][:] = 0
    d["terminated"][2, 3] = 1
    d["truncated"][4, 5] = 1
    base = VC.gae_ref(**d, gamma=0.99, lam=0.95)
    poisoned = dict(d, boot_value=d["boot_value"].copy())
    poisoned["boot_value"][2, 3] = np.nan  # terminated: no bootstrap
    poisoned["boot_value"][0, 0] = np.inf  # not done
    out = VC.gae_ref(**poisoned, gamma=0.99, lam=0.95)
    for x, y in zip(base, out):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
