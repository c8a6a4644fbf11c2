"""Per-env context application of every Brax kernel instance against the float64 oracle, with contexts that move.

`load_ctx` (carl_amd/csrc/brax_kernels.hip.h) turns an env's context row into its gravity, friction, elasticity, angular
damping factor exp(ang_damping dt), joint-stiffness scale and per-link masses -- the masses through the stability clamp
`mass_ratio_floor`, or `mass_ratio_floor_multi` when two or more links are light.  It runs at launch start and again
inside the step loop when an env auto-resets onto another context, its loops stride by the lane-group width, and it is
compiled into every (class, width, F32) instance.  tests/test_gpu_brax_kernel_matrix.py runs those instances on gravity /
friction rows with the static selector; here every (case, width) of tests/brax_kernel_cases.py (`CTX_CASES`: the kernel
table's cases and two models with the `joint_stiffness` column) runs on `context_matrix_rows`: every physics column the
model declares varied, every `mass_<link>` column through the clamp's four regimes (nominal-or-heavier, light above its
floor, under the single floor alone, under the combined floor with another), 37 rows under the round-robin selector at
stride 3 and a TimeLimit of 4, so that every env changes context -- masses included -- at each of its resets inside the
9-step window.  n = 815 envs (a ragged last wavefront at every width); models that stand on the ground start half their
envs 5 mm deep in it.

1. per-call parity: reset observations within 5e-6 (`obs_extended` models read the masses there), nine re-synced steps
   (tests/brax_parity_util.py: step_both); `ctx_idx`, `elapsed`, `episodes_done` equal the oracle's exactly on every
   step; `ctx_obs` holds the sampled row, not the clamped one;
2. the fused rollout from the same reset equals those steps bit for bit, branch record and counters included -- what
   exercises the `load_ctx` inside the step loop;
3. (per case) a 6-step rollout on these rows is bit-identical at every width the class lists;
4. the large-batch fragment schedule on these rows equals per-call steps bit for bit.

Bars of check 1 (`brax_kernel_cases.ctx_bars`).  Float64 pose algebra: 1e-5 as a maximum over the agreeing lane-steps,
at most 1e-3 excluded.  Float32: the kernel matrix's max 2e-4 / p99 1e-4 / excluded 5e-3 were measured on nominal masses;
on these rows they are multiplied by max(1, R), R the amplification of a float32 start-state rounding by the light
masses measured on the oracle alone (`F32_LIGHT_MASS_AMPLIFICATION`: at most 1.44 at the maximum, 1.37 at p99).
tests/test_brax_kernel_table.py holds these inputs on the host: regime coverage, stability, the share of edge-prone
lane-steps, R, and that each of five injected context faults moves the oracle far past the bar.
"""
import numpy as np
import pytest
import torch

from brax_kernel_cases import CTX_CASES, CTX_N, CTX_N_CTX, CTX_STEPS, CTX_STRIDE, CTX_TIME_LIMIT, FP32, GENERIC, \
    context_matrix_rows, ctx_bars, ctx_inputs, lane_widths, touch_down
from brax_parity_util import Parity, assert_parity, rel_err, step_both
from oracle import oracle as O

pytestmark = pytest.mark.gpu

COUNTERS = ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done", "ctx_obs", "last_return",
            "last_length")
BY_LABEL = {c.label: c for c in CTX_CASES}


def _engine(inp, s, device, n=None, rows=None, **kw):
    from carl_amd.brax_engine import BraxVecEngine

    case = inp.case
    kw = {**inp.selector, "max_episode_steps": inp.time_limit, **kw}
    return BraxVecEngine(s, len(inp.names), inp.rows if rows is None else rows, inp.n if n is None else n, device,
                         pose_float32=bool(case.flags & FP32), generic_substep=bool(case.flags & GENERIC), **kw)


def _start(inp, eng):
    """reset, and the touched-down start of a model that stands on the ground; -> the reset observation"""
    obs = eng.reset()
    if inp.touch:
        eng.set_state64(touch_down(eng.sys, eng.state64().cpu().numpy()))
    return obs


def _assert_bars(par: Parity, case, label):
    tol, p99_bar, excluded = ctx_bars(case)
    assert_parity(par, label, tol=tol, max_excluded=excluded)
    if p99_bar is not None:
        p99 = float(np.percentile(np.concatenate(par.err), 99))
        print(f"{label}: p99 {p99:.2e} (bar {p99_bar:.2e})")
        assert p99 <= p99_bar, (label, p99)


@pytest.mark.parametrize("case,width", [(c, w) for c in CTX_CASES for w in c.widths], ids=str)
def test_moving_contexts_match_the_oracle_and_the_rollout_equals_the_steps(device, case, width):
    assert (CTX_N, CTX_STEPS, CTX_TIME_LIMIT, CTX_N_CTX, CTX_STRIDE) == (815, 9, 4, 37, 3)
    inp = ctx_inputs(case)
    s, N, label = inp.pinned(width), inp.n, f"{case.label}/{width}"
    eng = _engine(inp, s, device, branch_record=True)
    assert width in eng.lane_widths()  # (so the hint is taken as it is: the launch runs this width's kernel)
    ora = inp.oracle()
    obs = _start(inp, eng).cpu().numpy()
    assert rel_err(obs, ora.reset()).max() < 5e-6
    np.testing.assert_array_equal(eng.ctx_idx.cpu().numpy(), ora.ctx_idx)
    rows32 = inp.rows.astype(np.float32)

    par, steps, seen = Parity(), [], set()
    for t in range(inp.steps):
        before = eng.ctx_idx.cpu().numpy()
        o, rew, term, trunc, out = step_both(eng, ora, inp.acts[t], par, t)
        steps.append((o.clone(), rew.clone(), term.clone(), trunc.clone(), eng.final_obs.clone(), eng.branch_sig.clone()))
        done = (term.cpu().numpy() | trunc.cpu().numpy()) != 0
        idx = eng.ctx_idx.cpu().numpy()
        # the selector and the episode bookkeeping: integers, exact (step_both has re-joined the few lanes whose
        # `terminated` differs; they are counted and bounded with the excluded share)
        np.testing.assert_array_equal(idx, ora.ctx_idx)
        np.testing.assert_array_equal(eng.elapsed.cpu().numpy(), ora.elapsed)
        np.testing.assert_array_equal(eng.episodes_done.cpu().numpy(), ora.episodes_done)
        assert (idx[done] != before[done]).all() and (idx[~done] == before[~done]).all()
        # the context observation is the SAMPLED row of the env's current context, not the clamped masses
        np.testing.assert_array_equal(eng.ctx_obs.cpu().numpy(), rows32[idx].T)
        same_flag = (term.cpu().numpy() != 0) == (out.terminated != 0)
        # the observation returned on a done step is the reset observation of the next episode, in the NEXT context
        sel = done & same_flag
        assert rel_err(o.cpu().numpy()[sel], out.obs[sel]).max(initial=0.0) < 5e-6, t
        seen.update(idx[done].tolist())
    assert int(eng.episodes_done.min()) >= 2 and len(seen) == CTX_N_CTX  # every row was entered by an in-window reset
    _assert_bars(par, case, label)

    # the same env steps fused: one rollout launch from the same reset (the `load_ctx` inside the step loop)
    roll = _engine(inp, s, device)
    _start(inp, roll)
    acts = torch.as_tensor(inp.acts, device=device)
    out = roll.rollout(acts, roll.alloc_rollout(inp.steps, final_obs=True, branch_record=True))
    for t, (o, rew, term, trunc, fin, sig) in enumerate(steps):
        assert torch.equal(out["obs"][t], o) and torch.equal(out["reward"][t], rew), t
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), t
        d = (term | trunc).bool()
        assert torch.equal(out["final_obs"][t][d], fin[d]), t
        assert torch.equal(out["branch_sig"][t], sig), t
    for name in COUNTERS:
        assert torch.equal(getattr(roll, name), getattr(eng, name)), name


@pytest.mark.parametrize("case", CTX_CASES, ids=str)
def test_every_width_gives_bit_identical_transitions_under_moving_contexts(device, case):
    """`BraxVecEngine.autotune` picks the width by time alone: a 6-step rollout on the context-matrix rows, every env
    auto-resetting onto other masses inside, comes out the same bit for bit at every width the class lists."""
    T = 6
    inp = ctx_inputs(case)
    widths = lane_widths(inp.sys, case.flags)
    assert len(widths) >= 2 and set(case.widths) <= set(widths)
    acts = torch.as_tensor(inp.acts[:T], device=device)
    ref = None
    for width in widths:
        eng = _engine(inp, inp.pinned(width), device)
        _start(inp, eng)
        out = eng.rollout(acts, eng.alloc_rollout(T, final_obs=True))
        cur = {k: out[k] for k in ("obs", "reward", "terminated", "truncated", "final_obs")}
        cur.update({k: getattr(eng, k) for k in COUNTERS})
        if ref is None:
            ref = (width, cur)
            assert int(eng.episodes_done.min()) >= 1
        else:
            for k, v in cur.items():
                assert torch.equal(v, ref[1][k]), (case.label, k, ref[0], width)


@pytest.mark.parametrize("label,width", [("planar", 16), ("multi", 16), ("ant_f32", 9), ("lean", 16)])
def test_large_batch_fragment_schedule_equals_repeated_step_under_moving_contexts(device, label, width):
    """More env groups than the chip holds wavefronts (3 072): the rollout hands an env's work between wavefronts at step
    boundaries (brax_kernels.hip.h: run()) -- with it the env's context record and mass rows, which an in-launch reset
    has just rewritten.  The smallest n with more groups than that at this width; T = 7 with a TimeLimit of 5."""
    case = BY_LABEL[label]
    inp = ctx_inputs(case)
    T, per_wave = 7, 64 // width
    n = 3072 * per_wave + 1
    assert -(-n // per_wave) > 3072 and -(-(n - 1) // per_wave) <= 3072
    s = inp.pinned(width)
    rng = np.random.default_rng(12)
    rows = context_matrix_rows(case, rng, CTX_N_CTX)
    acts = torch.as_tensor(rng.uniform(inp.lo, inp.hi, (T, n, s.n_act)).astype(np.float32), device=device)
    kw = dict(selector=O.SEL_ROUND_ROBIN, selector_stride=CTX_STRIDE, seed=5, max_episode_steps=5)
    e1, e2 = (_engine(inp, s, device, n=n, rows=rows, **kw) for _ in range(2))
    for e in (e1, e2):
        _start(inp, e)
    out = e1.rollout(acts, e1.alloc_rollout(T, final_obs=True))
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew), t
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), t
        d = (term | trunc).bool()
        assert torch.equal(out["final_obs"][t][d], e2.final_obs[d]), t
    for name in COUNTERS:
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    assert int(e1.episodes_done.min()) >= 1  # TimeLimit 5 < T: every env changed context inside the launch
