"""Every Brax kernel instance against the float64 oracle (oracle/brax_spring.c through oracle/brax.py), per lane.

carl_brax.hip's `kBraxKernels` holds 29 (class, width) entries: 40 `brax_kernel<MODE, MULTI, K, TASK, PLANAR, F32>`
functions, 11 reset + 29 step.  This file pins WHICH kernel runs and checks its physics on contexts that vary gravity and
friction only, every mass at its default, under the static selector: no env changes context inside a launch.  What
`load_ctx` does with the other columns -- elasticity, angular damping, joint stiffness, the link masses and their
stability clamp -- and with a context that changes on an in-launch reset is checked per instance by
tests/test_gpu_brax_context_matrix.py.  tests/brax_kernel_cases.py names one representative model per class (and
tests/test_brax_kernel_table.py holds that table against the library), beside a back-half Halfcheetah on the planar
kernels (joint anchors off their parent's z axis, which Hopper's are not) and the float32 shapes bench.py times; here
every (case, width) is pinned through
`carl_brax_sys_t::lanes_per_env` and run with n = 815 envs (a ragged last wavefront at every width), the static
selector over random gravity / friction contexts and a TimeLimit of 4 (auto-reset inside the window):

1. reset observations within 5e-6 of the oracle's (the reset kernel of the case's class at that width);
2. nine env steps, each re-synced from the engine's state (tests/brax_parity_util.py: step_both), random actions over
   the model's action bounds; truncation exact;
3. (per class) a 6-step rollout bit-identical at every width the class lists -- what lets `BraxVecEngine.autotune`
   pick a width by time alone;
4. the rollout equals repeated `step` bit for bit at that width, branch record and counters included;
5. (planar, multi, float32 lean) the large-batch fragment schedule equals per-call steps bit for bit.

Models that stand on the ground start half their envs 5 mm deep in it (`_touch_down`), and at least a tenth of their
lane-steps must deliver a contact impulse: the contact path is checked, not only the joints.

Bars of check 2.  Float64 pose algebra (the product path): north_star's 1e-5 as a maximum over the agreeing
lane-steps, at most 1e-3 of them excluded for a contact or termination decision that flipped inside the rounding
interval -- the bar of tests/test_gpu_brax.py.  Float32 pose algebra (CARL_FLAG_BRAX_FP32, opt-in): not a 1e-5 path.
profiles/r06_brax_fp32_deviation.txt measured its one-step deviation from the oracle over 81 920 lane-steps per family
(2 048 envs x 40 steps, eight families): agreeing maxima 1.4e-5 (inverted pendulum) to 6.6e-5 (HumanoidStandup), p99
2.4e-6 to 2.9e-5, contact exclusions up to 1.4e-3 (Walker2d).  The float32 bar is about three times the worst of each:
max <= 2e-4, p99 <= 1e-4, excluded <= 5e-3 of the lane-steps.  A wrong float32-only term that moves a single lane-step
by more than rounding amplified by the constraint springs fails the maximum; one that moves every lane a little fails
the p99.
"""
import numpy as np
import pytest
import torch

from brax_kernel_cases import CASES, EXTRA_CASES, FP32, GENERIC, GROUND_CONTACT, build, touch_down
from brax_parity_util import Parity, assert_parity, rel_err, step_both
from oracle import brax as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, STEPS, TIME_LIMIT = 815, 9, 4
F32_MAX, F32_P99, F32_EXCLUDED = 2e-4, 1e-4, 5e-3
COUNTERS = ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done", "ctx_obs", "last_return",
            "last_length")
ALL = CASES + EXTRA_CASES
BY_LABEL = {c.label: c for c in ALL}


def _rows(rng, n, default, names):
    rows = np.tile(default, (n, 1))
    rows[:, names.index("gravity")] = rng.uniform(-15, -5, n)
    rows[:, names.index("friction")] = rng.uniform(0.3, 1.5, n)
    return rows.astype(np.float32).astype(np.float64)


def _pinned(case, width):
    """-> (sys, names, default context, action bounds) of a case pinned to `width` lanes per env"""
    s, names, default = build(case.model)
    s.lanes_per_env = width
    return s, names, default, (float(min(s.act_lo[: s.n_act])), float(max(s.act_hi[: s.n_act])))


def _engine(case, s, names, rows, n, device, **kw):
    from carl_amd.brax_engine import BraxVecEngine

    return BraxVecEngine(s, len(names), rows, n, device, pose_float32=bool(case.flags & FP32),
                         generic_substep=bool(case.flags & GENERIC), **kw)


def _touch_down(eng):
    """the envs of a model that stands on the ground, half of them lowered 5 mm into it (brax_kernel_cases.touch_down)"""
    eng.set_state64(touch_down(eng.sys, eng.state64().cpu().numpy()))


def _assert_f32_parity(par: Parity, label):
    assert_parity(par, label, tol=F32_MAX, max_excluded=F32_EXCLUDED)
    p99 = float(np.percentile(np.concatenate(par.err), 99))
    assert p99 <= F32_P99, (label, p99)


@pytest.mark.parametrize("case,width", [(c, w) for c in ALL for w in c.widths], ids=str)
def test_every_kernel_instance_matches_oracle_and_its_rollout_equals_steps(device, case, width):
    seed = 1000 + 100 * ALL.index(case) + width
    rng = np.random.default_rng(seed)
    s, names, default, (lo, hi) = _pinned(case, width)
    rows = _rows(rng, N, default, names)
    kw = dict(selector=O.SEL_STATIC, seed=seed, ctx_idx0=np.arange(N))
    eng = _engine(case, s, names, rows, N, device, max_episode_steps=TIME_LIMIT, branch_record=True, **kw)
    assert width in eng.lane_widths()  # (so the hint is taken as it is: the launch runs this width's kernel)
    ora = B.Engine(s, rows, N, max_steps=TIME_LIMIT, **kw)
    obs = eng.reset().cpu().numpy()
    assert rel_err(obs, ora.reset()).max() < 5e-6
    if case.model in GROUND_CONTACT:
        _touch_down(eng)

    acts = rng.uniform(lo, hi, (STEPS, N, s.n_act)).astype(np.float32)
    par, steps, hits = Parity(), [], 0
    for t in range(STEPS):
        o, rew, term, trunc, out = step_both(eng, ora, acts[t], par, t)
        steps.append((o.clone(), rew.clone(), term.clone(), trunc.clone(), eng.final_obs.clone(), eng.branch_sig.clone()))
        hits += int((eng.branch_sig[:, 0] != 0).sum())
        done = (term.cpu().numpy() | trunc.cpu().numpy()) != 0
        if par.flag_mismatch == 0:
            # the observation returned on a done step is the reset observation of the next episode
            assert rel_err(o.cpu().numpy()[done], out.obs[done]).max(initial=0.0) < 5e-6
            np.testing.assert_array_equal(eng.elapsed.cpu().numpy(), ora.elapsed)
    assert int(eng.episodes_done.sum()) >= N  # TimeLimit 4 inside 9 steps: every env auto-reset at least once
    print(f"{case.label}/{width}: ground contact in {hits / (N * STEPS):.3f} of the lane-steps")
    if case.model in GROUND_CONTACT:
        assert hits >= 0.1 * N * STEPS, hits  # the contact path is exercised, not only the joints
    if case.flags & FP32:
        _assert_f32_parity(par, f"{case.label}/{width}")
    else:
        assert_parity(par, f"{case.label}/{width}")

    # the same env steps fused: one rollout launch from the same reset
    roll = _engine(case, s, names, rows, N, device, max_episode_steps=TIME_LIMIT, **kw)
    roll.reset()
    if case.model in GROUND_CONTACT:
        _touch_down(roll)
    out = roll.rollout(torch.as_tensor(acts, device=device), roll.alloc_rollout(STEPS, final_obs=True, branch_record=True))
    for t, (o, rew, term, trunc, fin, sig) in enumerate(steps):
        assert torch.equal(out["obs"][t], o) and torch.equal(out["reward"][t], rew), t
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), t
        d = (term | trunc).bool()
        assert torch.equal(out["final_obs"][t][d], fin[d]), t
        assert torch.equal(out["branch_sig"][t], sig), t
    for name in COUNTERS:
        assert torch.equal(getattr(roll, name), getattr(eng, name)), name


@pytest.mark.parametrize("case", ALL, ids=str)
def test_every_width_of_a_class_gives_bit_identical_transitions(device, case):
    """`BraxVecEngine.autotune` picks the width by time alone (and `CARLBraxEnv` autotunes by default, float32 included):
    a 6-step rollout, auto-reset inside, must come out the same bit for bit at every width the class lists."""
    T = 6
    rng = np.random.default_rng(77)
    ref = None
    for width in case.widths:
        s, names, default, (lo, hi) = _pinned(case, width)
        if ref is None:
            rows = _rows(rng, N, default, names)
            acts = torch.as_tensor(rng.uniform(lo, hi, (T, N, s.n_act)).astype(np.float32), device=device)
        eng = _engine(case, s, names, rows, N, device, max_episode_steps=TIME_LIMIT, selector=O.SEL_STATIC, seed=77,
                      ctx_idx0=np.arange(N))
        eng.reset()
        if case.model in GROUND_CONTACT:
            _touch_down(eng)
        out = eng.rollout(acts, eng.alloc_rollout(T, final_obs=True))
        cur = {k: out[k] for k in ("obs", "reward", "terminated", "truncated", "final_obs")}
        cur.update({k: getattr(eng, k) for k in COUNTERS})
        if ref is None:
            ref = (width, cur)
            assert int(eng.episodes_done.sum()) >= N
        else:
            for k, v in cur.items():
                assert torch.equal(v, ref[1][k]), (case.label, k, ref[0], width)


@pytest.mark.parametrize("label,width", [("planar", 16), ("multi", 16), ("ant_f32", 9)])
def test_large_batch_fragment_schedule_equals_repeated_step(device, label, width):
    """More env groups than the chip holds wavefronts (at most 256 CUs x 4 SIMDs x 3 = 3 072): the rollout cuts each
    workgroup's (group, step) work into fragments handed over between wavefronts at step boundaries (brax_kernels.hip.h:
    run()).  Bit for bit the per-call steps, counters included -- for the planar, multi-hinge and float32 lean kernels
    (tests/test_gpu_brax.py covers the float64 lean one)."""
    case = BY_LABEL[label]
    n, T = 30000, 7
    assert -(-n // (64 // width)) > 3072
    s, names, default, (lo, hi) = _pinned(case, width)
    rng = np.random.default_rng(12)
    rows = _rows(rng, 64, default, names)
    acts = torch.as_tensor(rng.uniform(lo, hi, (T, n, s.n_act)).astype(np.float32), device=device)
    kw = dict(selector=O.SEL_ROUND_ROBIN, seed=5, max_episode_steps=5)
    e1, e2 = (_engine(case, s, names, rows, n, device, **kw) for _ in range(2))
    for e in (e1, e2):
        e.reset()
        if case.model in GROUND_CONTACT:
            _touch_down(e)
    out = e1.rollout(acts, e1.alloc_rollout(T, final_obs=True))
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew), t
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), t
        d = (term | trunc).bool()
        assert torch.equal(out["final_obs"][t][d], e2.final_obs[d]), t
    for name in COUNTERS:
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    assert int(e1.episodes_done.min()) >= 1  # TimeLimit 5 < T: every env finished an episode inside the launch
