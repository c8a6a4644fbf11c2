"""The closed-loop rollout with a critic (carl_rollout_policy_valued) on the GPU: every kernel instance -- step type x
padded width H of {0, 32, 64} x sampled / deterministic -- against the same launch without a critic (nothing the critic
does not own changes a bit) and against oracle.policy_forward of the critic's packed block on teacher-forced inputs
(value, last_value, boot_value), plus weight sets, canaries and the engine options."""
import numpy as np
import pytest
import torch

import value_cases as VC
from carl_amd import _lib
from policy_cases import STEP_TYPES, make_engine, make_policy, stacked_policy
from policy_checks import SAMPLED_SEED, assert_same_state, engine_state, teacher

pytestmark = pytest.mark.gpu

N, T = 263, 19  # two workgroups, a ragged last one, a partial wave, pitch 272; 19 = 2 * 8 + 3 = 4 * 4 + 3
BOX = (_lib.PENDULUM, _lib.MOUNTAINCAR_CONT)
VALUE_FILL = 0x4B1D4B1D  # a float32 bit pattern (1.03e7) no value of these tests takes


def same_bits(a, b):
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


def engine_for(step_type, n=N, **kw):
    family, opts = STEP_TYPES[step_type]
    opts = dict(opts, **kw)
    opts.setdefault("max_episode_steps", 12 if family == _lib.CARTPOLE else 5)
    eng = make_engine(family, n, seed=n + 7, n_contexts=max(1, min(64, n)), **opts)
    if family == _lib.CARTPOLE:
        # Six pushes to the right before the launch: every pole leans, fast.  A launch then starts mid-episode, lanes the
        # policy cannot save terminate within a few steps, the episodes after their reset run into the limit of 12 steps,
        # and some terminate on the very step that truncates them -- whatever the policy.  (From a fresh reset a policy
        # that happens to balance ends every episode by truncation: the linear deterministic one did.)
        for _ in range(6):
            eng.step(torch.ones(n, dtype=torch.int32, device=eng.device))
    return eng


def networks(eng, a_widths, c_widths, a_act, c_act, seed):
    rng = np.random.default_rng(seed)
    actor = make_policy(eng, a_widths, a_act, rng, "all", clip=3.0, log_std=-0.5 if eng.family in BOX else None)
    return actor, VC.make_critic(eng, actor, c_widths, c_act, rng)


def check_valued_launch(eng, actor, critic, T, sampled, sets=None, final_obs=True, boot=True, expect_both=False, out=None):
    """checks 1-4 of one valued launch from a snapshot; returns (its output, the teacher-forced inputs [T, n, n_in])"""
    kw = dict(deterministic=False, sample_seed=SAMPLED_SEED, log_prob=True) if sampled else {}
    snap = eng.snapshot()
    ref = eng.rollout_policy(actor, T, final_obs=final_obs, **kw)
    ref_state = engine_state(eng)
    eng.restore(snap)
    out = eng.rollout_policy(actor, T, final_obs=final_obs, out=out, value_net=critic, bootstrap_truncated=boot, **kw)
    # 1. the critic changes nothing it does not own
    for k in ref:
        assert same_bits(out[k][:T], ref[k]), k
    assert_same_state(ref_state, engine_state(eng))
    ctx_after = eng.ctx_idx.cpu().numpy().astype(np.int64)
    # 2. value on the teacher-forced inputs
    x = teacher(eng, actor, snap, out["action"][:T])[0]
    lane_sets = None if sets is None else np.tile(sets, T)
    VC.check_values(critic, x, out["value"][:T].cpu().numpy(), lane_sets)
    # 3. last_value: the engine's context and observation after the launch
    tab = eng.ctx_table.cpu().numpy()
    x_last = np.concatenate([tab[actor.ctx_rows][:, ctx_after].T, out["obs"][T - 1].cpu().numpy()], axis=1)
    VC.check_values(critic, x_last, out["last_value"].cpu().numpy(), sets)
    te, tr = (out[k][:T].cpu().numpy().astype(bool) for k in ("terminated", "truncated"))
    if expect_both:
        assert (tr & ~te).any(), "the case must contain a truncation-only step"
        assert te.any(), "the case must contain a termination"
        assert (tr & te).any(), "the case must contain a step that is both terminated and truncated"
    if not boot:
        assert "boot_value" not in out
        return out, x
    # 4. boot_value: the critic of [context values before the step, terminal observation] on truncation-only steps
    cut = tr & ~te
    bv = out["boot_value"][:T].cpu().numpy()
    assert np.all(bv[~cut].view(np.int32) == 0), "boot_value must be +0.0f wherever the step was not truncated only"
    if final_obs:
        x_boot = np.concatenate([x[:, :, : len(actor.ctx_rows)], out["final_obs"][:T].cpu().numpy()], axis=2)
        VC.check_values(critic, x_boot, bv, lane_sets, where=cut)
    return out, x


def hidden_of(H):
    return {0: (), 32: (31,), 64: (33, 64)}[H]


@pytest.mark.parametrize("sampled", [False, True], ids=["deterministic", "sampled"])
@pytest.mark.parametrize("H", [0, 32, 64])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_every_instance(step_type, H, sampled):
    eng = engine_for(step_type)  # round-robin selector: a reset moves the lane, so boot_value needs the OLD context
    act = ["relu", "tanh", "identity"][(H // 32 + sampled) % 3]
    actor, critic = networks(eng, hidden_of(H), hidden_of(H), act, act, seed=H + 3 * sampled)
    snap = eng.snapshot()
    out, _ = check_valued_launch(eng, actor, critic, T, sampled, expect_both=eng.family == _lib.CARTPOLE)
    tr = out["truncated"][:T].cpu().numpy().astype(bool) & ~out["terminated"][:T].cpu().numpy().astype(bool)
    assert tr.any(), "no truncation-only step: boot_value was not exercised"
    ctx = eng.ctx_idx.cpu().numpy()
    eng.restore(snap)
    assert (eng.ctx_idx.cpu().numpy() != ctx).any(), "no lane moved context"
    # the same boot_value bits whether or not final_obs was requested
    kw = dict(deterministic=False, sample_seed=SAMPLED_SEED) if sampled else {}
    again = eng.rollout_policy(actor, T, value_net=critic, **kw)
    assert "final_obs" not in again
    for k in ("boot_value", "value", "last_value", "action"):
        assert same_bits(again[k], out[k]), k


@pytest.mark.parametrize("t", [1, 43])
def test_other_horizons(t):
    eng = engine_for("cartpole")
    actor, critic = networks(eng, (33,), (16, 8), "relu", "relu", seed=t)
    check_valued_launch(eng, actor, critic, t, sampled=True, expect_both=t == 43)


@pytest.mark.parametrize("a_widths,c_widths,a_act,c_act", [
    ((), (40, 9), "identity", "tanh"),      # a linear actor in an H = 64 instance
    ((64, 64), (), "tanh", "identity"),     # a linear critic in an H = 64 instance
    ((33,), (7,), "relu", "relu"),          # a narrower critic
    ((5, 6), (64,), "relu", "tanh"),        # a wider critic, another activation
])
@pytest.mark.parametrize("step_type", ["pendulum", "acrobot"])
def test_critic_shapes_apart_from_the_actors(step_type, a_widths, c_widths, a_act, c_act):
    eng = engine_for(step_type)
    actor, critic = networks(eng, a_widths, c_widths, a_act, c_act, seed=len(c_widths))
    check_valued_launch(eng, actor, critic, T, sampled=True)
    check_valued_launch(eng, actor, critic, T, sampled=False)


def test_two_stacked_critics_follow_their_own_sets():
    eng = engine_for("cartpole", n=512)
    actor = stacked_policy(eng, 2, 256, np.random.default_rng(11))
    crits = [VC.make_critic(eng, actor, (20,), "relu", np.random.default_rng(s)) for s in (1, 2)]
    critic = type(actor).stack(crits, 256, head="value")
    critic.params = critic.params.copy()
    critic.transform_section()[:] = actor.transform_section()  # (each set's section is its actor set's)
    sets = np.arange(512) // 256
    out, x = check_valued_launch(eng, actor, critic, T, sampled=False, sets=sets, expect_both=True)
    with pytest.raises(AssertionError):  # ... and not the other set
        VC.check_values(critic, x, out["value"][:T].cpu().numpy(), np.tile(1 - sets, T))


@pytest.mark.parametrize("n", [263, 256])
@pytest.mark.parametrize("sampled", [False, True])
def test_canaries_round_the_new_columns(n, sampled):
    eng = engine_for("mountaincar", n=n)
    actor, critic = networks(eng, (33,), (12,), "relu", "relu", seed=n)
    P0 = eng._row_pitch()
    P = P0 + 32 if n % 16 == 0 else P0
    rows = T + 3
    adt = torch.int32 if eng.info.action_is_discrete else torch.float32
    full = {"obs": torch.zeros((rows, P, eng.D), device=eng.device), "reward": torch.zeros((rows, P), device=eng.device),
            "terminated": torch.zeros((rows, P), dtype=torch.uint8, device=eng.device),
            "truncated": torch.zeros((rows, P), dtype=torch.uint8, device=eng.device),
            "action": torch.zeros((rows, P), dtype=adt, device=eng.device)}
    for k in ("value", "boot_value") + (("log_prob",) if sampled else ()):
        full[k] = torch.full((rows, P), VALUE_FILL, dtype=torch.int32, device=eng.device).view(torch.float32)
    lv_full = torch.full((n + 24,), VALUE_FILL, dtype=torch.int32, device=eng.device).view(torch.float32)
    view = {k: v[:, :n] for k, v in full.items()}
    view["last_value"] = lv_full[8: 8 + n]
    check_valued_launch(eng, actor, critic, T, sampled, final_obs=False, out=view)
    for k in ("value", "boot_value"):
        c = full[k].view(torch.int32) == VALUE_FILL
        assert bool(c[T:].all()), f"{k}: a row >= T was written"
        assert bool(c[:, P0:].all()), f"{k}: a column >= carl_rollout_pitch(n) was written"
        assert not bool(c[:T, :P0].any()), f"{k}: an entry of [T][pitch] is missing"
    c = lv_full.view(torch.int32) == VALUE_FILL
    assert bool(c[:8].all()) and bool(c[8 + n:].all()) and not bool(c[8: 8 + n].any())


def test_no_auto_reset_without_bootstrapping():
    eng = engine_for("cartpole", auto_reset=False)
    actor, critic = networks(eng, (33,), (12,), "relu", "relu", seed=5)
    with pytest.raises(ValueError, match="auto_reset"):
        eng.rollout_policy(actor, T, value_net=critic)
    out, _ = check_valued_launch(eng, actor, critic, T, sampled=True, final_obs=False, boot=False)
    assert out["terminated"].any()
    assert "boot_value" not in out


def test_lane_offset():
    eng = engine_for("mountaincar", lane_offset=1000)
    actor, critic = networks(eng, (33,), (12,), "relu", "tanh", seed=6)
    check_valued_launch(eng, actor, critic, T, sampled=True)


def test_gae_from_the_same_call_is_gae_of_its_columns():
    eng = engine_for("cartpole")
    actor, critic = networks(eng, (33,), (12,), "relu", "relu", seed=8)
    out = eng.rollout_policy(actor, T, deterministic=False, sample_seed=3, value_net=critic, gae=(0.99, 0.95))
    res = eng.gae(out["reward"], out["value"], out["terminated"], out["truncated"], out["last_value"], 0.99, 0.95,
                  boot_value=out["boot_value"])
    te, tr = (out[k].cpu().numpy().astype(bool) for k in ("terminated", "truncated"))
    assert (tr & ~te).any() and te.any()
    for k in ("advantage", "return"):
        assert same_bits(out[k], res[k]), k
    adv, ret = VC.gae_ref(*(out[k].cpu().numpy() for k in ("reward", "value", "terminated", "truncated", "last_value")),
                          0.99, 0.95, boot_value=out["boot_value"].cpu().numpy())
    np.testing.assert_array_equal(out["advantage"].cpu().numpy().view(np.int32), adv.view(np.int32))
    np.testing.assert_array_equal(out["return"].cpu().numpy().view(np.int32), ret.view(np.int32))
