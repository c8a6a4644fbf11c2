"""Parity of the HIP lane engine (through the C ABI) with the CPU oracle -- needs an MI355X.

Tolerances (north_star): floating-point transition outputs within 1e-5 of the float64
oracle, measured as |d| <= 1e-5 * (1 + |x|); discrete outputs (terminated / truncated,
context ids, elapsed counters, compacted index lists) and reset states bit-exact.  A
done flag may legitimately differ only where the float64 margin to its threshold is
below fp32 resolution; such rows are counted and bounded, not ignored.

Acrobot: the reference evaluates `_terminal` on its unrounded float64 state (gymnasium acrobot.py keeps
`self.state` in float64; oracle/classic_control.inc does the same); the kernel evaluates it on the STORED float32
angles (one trig evaluation per step serves the next RK4 stage, `_terminal` and the observation: DESIGN 4.3a), which
sit <= 1.2e-7 from the unrounded ones -- the flag can differ only for states whose float64 margin
|-cos t1 - cos(t1 + t2) - 1| is < 4e-7.  That is inside the 1e-6 margin every flag comparison below allows
(`flag_margin`), and such rows are counted.  Putting the decision back on the unrounded angles, even behind a rare
wave-uniform branch, keeps two more float64 values live across the step's tail: the pair kernel of BASELINE config 3
then spills (126 -> 128 VGPRs + 64 B of scratch; measured with tools/kernel_resources.sh in round 6), so the stored-angle
rule stays and is stated here.
"""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _engine(family, table, n, device, **kw):
    from carl_amd.engine import VecEngine

    return VecEngine(family, table, n, device, **kw)


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / (1.0 + np.abs(want))


def random_table(fam, rng, n_ctx):
    """contexts inside the reference's feature bounds (SURVEY.md 8d distributions + more)"""
    t = np.tile(O.default_row(fam), (n_ctx, 1))
    U = rng.uniform
    if fam == O.CARTPOLE:
        t[:, 0] = U(5, 15, n_ctx); t[:, 1] = U(0.5, 2, n_ctx); t[:, 2] = U(0.05, 0.3, n_ctx)
        t[:, 3] = U(0.3, 1.0, n_ctx); t[:, 4] = U(5, 15, n_ctx); t[:, 5] = U(0.01, 0.03, n_ctx)
    elif fam == O.PENDULUM:
        t[:, 0] = U(1, 20, n_ctx); t[:, 2] = U(1, 20, n_ctx); t[:, 4] = U(0.5, 2.0, n_ctx)
        t[:, 3] = U(0.5, 2.0, n_ctx)
    elif fam == O.ACROBOT:
        t[:, 0] = U(0.5, 2, n_ctx); t[:, 2] = U(0.5, 2, n_ctx); t[:, 3] = U(0.5, 2, n_ctx)
        t[:, 4] = U(0.3, 0.7, n_ctx); t[:, 5] = U(0.3, 0.7, n_ctx)
    elif fam == O.MOUNTAINCAR:
        t[:, 5] = U(5e-4, 2e-3, n_ctx); t[:, 6] = U(1.5e-3, 3.5e-3, n_ctx); t[:, 3] = U(0.3, 0.55, n_ctx)
    else:
        t[:, 5] = U(5e-4, 3e-3, n_ctx); t[:, 3] = U(0.3, 0.55, n_ctx)
    return t.astype(np.float32).astype(np.float64)


def random_actions(fam, rng, shape):
    if fam == O.PENDULUM:
        return rng.uniform(-2.5, 2.5, shape).astype(np.float32)
    if fam == O.MOUNTAINCAR_CONT:
        return rng.uniform(-1.2, 1.2, shape).astype(np.float32)
    return rng.integers(0, 2 if fam == O.CARTPOLE else 3, shape).astype(np.int32)


def flag_margin(fam, ctx_rows, next_state):
    """|distance| of the float64 next state to the nearest termination threshold"""
    s = next_state
    if fam == O.CARTPOLE:
        return np.minimum(np.abs(np.abs(s[:, 0]) - 2.4), np.abs(np.abs(s[:, 2]) - 12 * 2 * np.pi / 360))
    if fam == O.ACROBOT:
        return np.abs(-np.cos(s[:, 0]) - np.cos(s[:, 1] + s[:, 0]) - 1.0)
    if fam in (O.MOUNTAINCAR, O.MOUNTAINCAR_CONT):
        return np.minimum(np.abs(s[:, 0] - ctx_rows[:, 3]), np.abs(s[:, 1] - ctx_rows[:, 4]) + 1e-3 * (s[:, 1] != ctx_rows[:, 4]))
    return np.full(s.shape[0], np.inf)


def state_from_obs(fam, obs):
    """the state a family's observation determines (angles modulo 2 pi, which the dynamics do not see)"""
    o = np.asarray(obs, dtype=np.float64)
    if fam == O.PENDULUM:
        return np.stack([np.arctan2(o[:, 1], o[:, 0]), o[:, 2]], axis=1)
    if fam == O.ACROBOT:
        return np.stack([np.arctan2(o[:, 1], o[:, 0]), np.arctan2(o[:, 3], o[:, 2]), o[:, 4], o[:, 5]], axis=1)
    return o  # CartPole, MountainCar(Continuous): the observation IS the state


def restep_rollout_with_oracle(fam, table, s0, acts, out, t_max=None, max_edge_flags=8):
    """Tie a fused rollout's OUTPUT to the oracle directly: every (t, lane) of the rollout is
    re-stepped by `O.transitions` from the state the PREVIOUS row of the same output determines (on a done step the
    returned observation is the reset observation = the next episode's first state, so the chain never breaks) and
    the kernel's transition must match within 1e-5: observation (the terminal one where `final_obs` was written,
    else done rows are skipped for the observation only), reward, `terminated`.  Flags may differ only on rows whose
    float64 next state sits within 1e-5 of a threshold (counted, bounded).  Returns the number of rows checked."""
    T = int(acts.shape[0]) if t_max is None else min(int(t_max), int(acts.shape[0]))
    prev = np.asarray(s0, dtype=np.float64)
    have_final = "final_obs" in out
    rows, edge = 0, 0
    worst = 0.0
    for t in range(T):
        a = acts[t].cpu().numpy()
        w_s, w_obs, w_rew, w_term = O.transitions(fam, table, prev, a)
        obs_t = out["obs"][t].cpu().numpy()
        term = out["terminated"][t].cpu().numpy()
        done = (term | out["truncated"][t].cpu().numpy()) != 0
        got = np.where(done[:, None], out["final_obs"][t].cpu().numpy(), obs_t) if have_final else obs_t
        bad_flag = term != w_term
        if bad_flag.any():
            assert (flag_margin(fam, table[bad_flag], w_s[bad_flag]) < 1e-5).all(), (t, int(bad_flag.sum()))
            edge += int(bad_flag.sum())
        use = ~bad_flag if have_final else (~bad_flag & ~done)
        e = rel_err(got[use], w_obs[use]).max(initial=0.0)
        # (CartPole's reward on a step AFTER termination is 0 in gymnasium; with auto-reset that step does not exist)
        er = rel_err(out["reward"][t].cpu().numpy()[~bad_flag], w_rew[~bad_flag]).max(initial=0.0)
        worst = max(worst, float(e), float(er))
        assert e <= TOL and er <= TOL, (O.FAMILY_NAMES[fam], t, float(e), float(er))
        rows += int(use.sum())
        prev = state_from_obs(fam, obs_t)  # what the kernel continues from (reset state on done rows)
    assert edge <= max_edge_flags, edge
    print(f"restep {O.FAMILY_NAMES[fam]}: {rows} rows re-stepped by the oracle, worst {worst:.2e}, {edge} threshold-edge flags",
          flush=True)
    return rows


def run_transitions(fam, ctx_rows, state, action, device, **kw):
    """one engine step from prescribed (context, state, action) rows, lane i <-> row i"""
    n = state.shape[0]
    eng = _engine(fam, ctx_rows, n, device, selector=0, auto_reset=False, **kw)
    eng.reset()
    eng.state.copy_(torch.as_tensor(np.ascontiguousarray(state.T, dtype=np.float32)))
    obs, rew, term, trunc = eng.step(torch.as_tensor(action))
    torch.cuda.synchronize()
    return (eng.state.t().cpu().numpy(), obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(),
            trunc.cpu().numpy())


# ------------------------------------------------------------------ single transitions
@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
def test_golden_fixture_transitions(fam, device, golden_dir):
    """committed vectors (tests/golden/transitions_*.npz, float64 oracle) through the C ABI"""
    g = np.load(os.path.join(golden_dir, f"transitions_{O.FAMILY_NAMES[fam]}.npz"))
    s2, obs, rew, term, trunc = run_transitions(fam, g["ctx"].astype(np.float64), g["state"], g["action"], device)
    assert rel_err(s2, g["next_state"]).max() <= TOL
    assert rel_err(obs, g["obs"]).max() <= TOL
    assert rel_err(rew, g["reward"]).max() <= TOL
    diff = term != g["terminated"]
    margin = flag_margin(fam, g["ctx"].astype(np.float64), g["next_state"])
    assert (margin[diff] < 1e-6).all(), "a done flag differs away from its threshold"
    assert diff.sum() <= 2
    assert not trunc.any()


@pytest.mark.parametrize("fam", [O.MOUNTAINCAR, O.MOUNTAINCAR_CONT], ids=["mountaincar", "mountaincarcont"])
def test_mountaincar_wide_track_contexts(fam, device):
    """min_position / max_position are context features without bounds (carl_mountaincar.py:15-50): positions far
    outside the default [-1.2, 0.6] -- where the kernel's short double-angle cosine is not fitted and the lane takes
    the range-reduced one -- mixed lane by lane with ordinary ones, incl. huge arguments (|3 p| > 1e5)."""
    rng = np.random.default_rng(77 + fam)
    n = 65536
    ctx = random_table(fam, rng, n)
    ctx[:, 0], ctx[:, 1] = -3.0e5, 3.0e5  # MIN_POS, MAX_POS
    pos = np.where(rng.random(n) < 0.5, rng.uniform(-1.2, 0.6, n), rng.uniform(-40, 40, n))
    pos[::97] = rng.integers(-200000, 200000, pos[::97].shape)  # whole numbers: 3 p is exact in float32 too
    pos[1::97] = rng.choice([-1.2334, 1.2334, -1.2333, 1.2333], pos[1::97].shape)  # |1.5 p| either side of 1.85
    s = np.stack([pos, rng.uniform(-0.07, 0.07, n)], 1).astype(np.float32)
    a = random_actions(fam, rng, n)
    s2, obs, rew, term, _ = run_transitions(fam, ctx, s, a, device)
    w_s2, w_obs, w_rew, w_term = O.transitions(fam, ctx, s.astype(np.float64), a, precision="f64")
    # the cosine enters the velocity times gravity (<= 3.5e-3); float32 rounding of 3 p at |p| = 40 alone is 1.3e-8
    assert np.abs(s2[:, 1] - w_s2[:, 1]).max() <= 5e-8
    assert rel_err(s2, w_s2).max() <= TOL
    assert rel_err(obs, w_obs).max() <= TOL
    assert rel_err(rew, w_rew).max() <= TOL
    # a lane's result does not depend on its wave mates: the same rows in another order give the same bits
    perm = rng.permutation(n)
    p_s2, *_ = run_transitions(fam, ctx[perm], s[perm], a[perm], device)
    assert np.array_equal(p_s2, s2[perm])


def test_cartpole_pole_angle_through_every_sincos_path(device):
    """Without auto-reset a lane keeps stepping after termination and the pole swings through every angle, so CartPole's
    inlined `sincos_fast_smallarg` meets all of its paths: the bare polynomials (|theta| <= 0.78 in the whole wave), the
    fall-through into `sincos_fast` (0.78f and its neighbours, up to +-40 rad) and that function's library path beyond
    1e5 -- mixed lane by lane, so most waves hold all of them."""
    rng = np.random.default_rng(4242)
    n = 65536
    ctx = random_table(O.CARTPOLE, rng, n)
    U = rng.uniform
    g = np.float32(0.78)
    edge = np.array([g, np.nextafter(g, np.float32(0)), np.nextafter(g, np.float32(1))], dtype=np.float32)
    kind = rng.integers(0, 5, n)
    theta = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                      [U(-0.21, 0.21, n), U(0.21, 0.78, n) * rng.choice([-1, 1], n),
                       rng.choice(np.concatenate([edge, -edge]), n).astype(np.float64), U(-40, 40, n)],
                      np.round(U(1.0e5, 4.0e5, n)) * rng.choice([-1, 1], n))  # whole numbers: exact in float32
    s = np.stack([U(-2.5, 2.5, n), U(-3, 3, n), theta, U(-3, 3, n)], 1).astype(np.float32)
    assert all(((np.abs(s[:, 2]) > lo) & (np.abs(s[:, 2]) <= hi)).sum() > 10000 for lo, hi in ((-1, 0.21), (0.21, 0.78), (0.78, 40), (1e5, 4e5)))
    a = random_actions(O.CARTPOLE, rng, n)
    s2, obs, rew, term, _ = run_transitions(O.CARTPOLE, ctx, s, a, device)
    w_s2, w_obs, w_rew, w_term = O.transitions(O.CARTPOLE, ctx, s.astype(np.float64), a, precision="f64")
    print(f"cartpole, every sincos path: worst rel_err state {rel_err(s2, w_s2).max():.2e}, obs {rel_err(obs, w_obs).max():.2e}, "
          f"reward {rel_err(rew, w_rew).max():.2e}", flush=True)
    assert rel_err(s2, w_s2).max() <= TOL
    assert rel_err(obs, w_obs).max() <= TOL
    assert rel_err(rew, w_rew).max() <= TOL
    # a lane's result does not depend on its wave mates: the same rows in another order give the same bits
    perm = rng.permutation(n)
    p_s2, p_obs, *_ = run_transitions(O.CARTPOLE, ctx[perm], s[perm], a[perm], device)
    assert np.array_equal(p_s2.view(np.uint32), s2[perm].view(np.uint32))
    assert np.array_equal(p_obs.view(np.uint32), obs[perm].view(np.uint32))


def _pendulum_wide_angles(rng, n):
    U = rng.uniform
    g = np.float32(1.0e5)
    edge = np.array([g, np.nextafter(g, np.float32(0)), np.nextafter(g, np.float32(np.inf))], dtype=np.float32)
    kind = rng.integers(0, 4, n)
    theta = np.select([kind == 0, kind == 1, kind == 2],
                      [U(-10, 10, n), U(-1.0e4, 1.0e4, n),
                       np.where(rng.random(n) < 0.3, rng.choice(np.concatenate([edge, -edge]), n).astype(np.float64),
                                U(0.99e5, 1.01e5, n) * rng.choice([-1, 1], n))],
                      U(1.0e5, 1.0e6, n) * rng.choice([-1, 1], n))
    s = np.stack([theta, U(-8, 8, n)], 1).astype(np.float32)
    return s


def _pendulum_wide_run(device):
    rng = np.random.default_rng(777)
    n = 65536
    ctx = random_table(O.PENDULUM, rng, n)
    s = _pendulum_wide_angles(rng, n)
    a = random_actions(O.PENDULUM, rng, n)
    got = run_transitions(O.PENDULUM, ctx, s, a, device)
    want = O.transitions(O.PENDULUM, ctx, s.astype(np.float64), a, precision="f64")
    return rng, ctx, s, a, got, want


def test_pendulum_angle_through_every_sincos_path(device):
    """Pendulum never normalises its stored angle, so `sincos_fast_pk` meets what a long rollout or a context with a huge
    initial angle feeds it: |theta| <= 10, up to +-1e4 (the three-term reduction), either side of the 1e5 guard and the
    outlined library call beyond it, mixed lane by lane.  At these magnitudes the float32 state's own rounding exceeds the
    bar (ulp(1e5) = 7.8e-3), so each output is held to what the kernel computes from exact inputs: the new velocity
    against the oracle at TOL; the new angle against theta + omega' dt within one float32 ulp of the result; the
    observation against float64 cos / sin of the RETURNED float32 angle (the kernel takes its trig at the stored angle)."""
    rng, ctx, s, a, (s2, obs, rew, term, _), (w_s2, w_obs, w_rew, w_term) = _pendulum_wide_run(device)
    n = s.shape[0]
    assert all(((np.abs(s[:, 0]) > lo) & (np.abs(s[:, 0]) <= hi)).sum() > 5000 for lo, hi in ((-1, 10), (10, 1e4), (0.99e5, 1e5), (1e5, 1e6)))
    th2 = s[:, 0].astype(np.float64) + s2[:, 1].astype(np.float64) * ctx[:, 1]  # theta + omega' dt from the RETURNED omega'
    e_v = rel_err(s2[:, 1], w_s2[:, 1]).max()
    e_th = (np.abs(s2[:, 0].astype(np.float64) - th2) / np.spacing(np.abs(th2).astype(np.float32)).astype(np.float64)).max()
    trig = np.stack([np.cos(s2[:, 0].astype(np.longdouble)), np.sin(s2[:, 0].astype(np.longdouble))], 1).astype(np.float64)
    e_o = max(rel_err(obs[:, :2], trig).max(), rel_err(obs[:, 2], w_obs[:, 2]).max())
    print(f"pendulum, every sincos path: velocity {e_v:.2e}, angle {e_th:.2f} ulp, observation {e_o:.2e}", flush=True)
    assert e_v <= TOL
    assert e_th <= 1.0
    assert e_o <= TOL
    assert np.array_equal(obs[:, 2].view(np.uint32), s2[:, 1].view(np.uint32)) and not term.any()
    perm = rng.permutation(n)
    p_s2, p_obs, p_rew, *_ = run_transitions(O.PENDULUM, ctx[perm], s[perm], a[perm], device)
    assert np.array_equal(p_s2.view(np.uint32), s2[perm].view(np.uint32))
    assert np.array_equal(p_obs.view(np.uint32), obs[perm].view(np.uint32))
    assert np.array_equal(p_rew.view(np.uint32), rew[perm].view(np.uint32))


def test_pendulum_reward_at_every_angle_magnitude(device):
    """the reward of the same transitions (computed from the exact float32 inputs: angle_normalize(theta)^2 + ...) against
    the oracle at TOL"""
    rng, ctx, s, a, (s2, obs, rew, term, _), (w_s2, w_obs, w_rew, w_term) = _pendulum_wide_run(device)
    e = rel_err(rew, w_rew)
    for lo, hi in ((0, 10), (10, 1e2), (1e2, 1e3), (1e3, 1e4), (1e4, 1e5), (1e5, 1e6)):
        m = (np.abs(s[:, 0]) > lo) & (np.abs(s[:, 0]) <= hi)
        print(f"pendulum reward, {lo:g} < |theta| <= {hi:g}: worst rel_err {e[m].max(initial=0):.2e} over {int(m.sum())} rows", flush=True)
    assert e.max() <= TOL


@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
def test_random_transitions_100k(fam, device):
    """>= 1e5 random (context, state, action) triples per family vs the float64 oracle"""
    rng = np.random.default_rng(10 + fam)
    n = 131072
    ctx = random_table(fam, rng, n)
    U = rng.uniform
    if fam == O.CARTPOLE:
        s = np.stack([U(-2.5, 2.5, n), U(-3, 3, n), U(-0.22, 0.22, n), U(-3, 3, n)], 1)
    elif fam == O.PENDULUM:
        s = np.stack([U(-10, 10, n), U(-8, 8, n)], 1)
    elif fam == O.ACROBOT:
        s = np.stack([U(-np.pi, np.pi, n), U(-np.pi, np.pi, n), U(-4 * np.pi, 4 * np.pi, n),
                      U(-9 * np.pi, 9 * np.pi, n)], 1)
    else:
        s = np.stack([U(-1.2, 0.6, n), U(-0.07, 0.07, n)], 1)
    s = s.astype(np.float32)
    a = random_actions(fam, rng, n)
    s2, obs, rew, term, _ = run_transitions(fam, ctx, s, a, device)
    w_s2, w_obs, w_rew, w_term = O.transitions(fam, ctx, s.astype(np.float64), a, precision="f64")
    assert rel_err(s2, w_s2).max() <= TOL
    assert rel_err(obs, w_obs).max() <= TOL
    assert rel_err(rew, w_rew).max() <= TOL
    diff = term != w_term
    margin = flag_margin(fam, ctx, w_s2)
    assert (margin[diff] < 1e-6).all()
    assert diff.mean() < 1e-4


def wide_context_rows(fam, rng, n, span):
    """every physics feature scaled by an independent log-uniform factor in [1 / span, span] around the reference's default"""
    scaled = {O.CARTPOLE: [0, 1, 2, 3, 4, 5], O.PENDULUM: [1, 2, 3, 4], O.ACROBOT: [0, 2, 3, 4, 5, 6, 7, 8],
              O.MOUNTAINCAR: [2, 5, 6], O.MOUNTAINCAR_CONT: [2, 5]}[fam]
    ctx = np.tile(O.default_row(fam), (n, 1))
    for c in scaled:
        ctx[:, c] *= np.exp(rng.uniform(-np.log(span), np.log(span), n))
    if fam == O.ACROBOT:  # LINK_COM_POS_1 / _2: inside their declared bounds (0, 1], and on the link
        ctx[:, 4] = np.minimum(ctx[:, 4], np.minimum(ctx[:, 0], 1.0))
        ctx[:, 5] = np.minimum(ctx[:, 5], 1.0)
    ctx = ctx.astype(np.float32).astype(np.float64)
    U = rng.uniform
    if fam == O.CARTPOLE:
        s = np.stack([U(-2.5, 2.5, n), U(-3, 3, n), U(-0.22, 0.22, n), U(-3, 3, n)], 1)
    elif fam == O.PENDULUM:
        s = np.stack([U(-10, 10, n), U(-8, 8, n)], 1)
    elif fam == O.ACROBOT:  # velocities over the whole (scaled) range [-MAX_VEL, MAX_VEL]
        s = np.stack([U(-np.pi, np.pi, n), U(-np.pi, np.pi, n), U(-1, 1, n) * ctx[:, 7], U(-1, 1, n) * ctx[:, 8]], 1)
    else:
        s = np.stack([U(-1.2, 0.6, n), U(-1, 1, n) * ctx[:, 2]], 1)
    return ctx, s.astype(np.float32)


@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
def test_random_transitions_wide_contexts(fam, device):
    """Far outside the usual ranges but inside the reference's declared feature bounds (carl_acrobot.py:15-69: masses /
    lengths / MOI in [0.1, 10], MAX_VEL up to x 10; likewise the other families): each physics feature x a log-uniform
    factor in [1/10, 10] (Acrobot [1/3, 3]: beyond that some rows have a near-singular mass matrix, the new angle is
    ~1e9 rad and the reference's own `while x > pi: x -= 2 pi`, restated faithfully in the oracle, spins for minutes).
    CartPole / Pendulum / MountainCar stay within 1e-5 everywhere.  Acrobot at the scaled velocity bounds is STIFF: a
    transition amplifies an error of its stage trig by up to 1e8, so a row can only be compared where the float64 oracle
    itself holds still -- rows above the bar must be (nearly all) rows whose oracle moves by > 1e-7 when its input state
    moves by 1e-15 relative, and few.  (With the 6e-11 cosine of rounds 4-5 this test finds 265 rows above the bar, worst
    0.11; with the r^4 / 24 term back: 5, of which 4 ill-conditioned, the fifth at 1.4e-5 -- DESIGN 4.3b.)"""
    rng = np.random.default_rng(1000 + fam)
    n = 131072
    ctx, s = wide_context_rows(fam, rng, n, 3.0 if fam == O.ACROBOT else 10.0)
    a = random_actions(fam, rng, n)
    s2, obs, rew, term, _ = run_transitions(fam, ctx, s, a, device)
    w_s2, w_obs, w_rew, w_term = O.transitions(fam, ctx, s.astype(np.float64), a, precision="f64")
    assert np.isfinite(np.asarray(w_s2)).all()
    e = np.maximum(rel_err(s2, w_s2).max(1), np.maximum(rel_err(obs, w_obs).max(1), rel_err(rew, w_rew)))
    bad = np.nonzero(e > TOL)[0]
    diff = term != w_term
    assert (flag_margin(fam, ctx, np.asarray(w_s2))[diff] < 1e-6).all()
    if fam != O.ACROBOT:
        assert bad.size == 0, e.max()
        return
    assert bad.size <= 20, bad.size  # (measured 5 of 131 072)
    p_s2, p_obs, _, _ = O.transitions(fam, ctx[bad], s[bad].astype(np.float64) * (1.0 + 1e-15), a[bad], precision="f64")
    moved = np.maximum(rel_err(p_s2, np.asarray(w_s2)[bad]).max(1), rel_err(p_obs, np.asarray(w_obs)[bad]).max(1))
    well = moved <= 1e-7
    assert well.sum() <= 3 and (e[bad][well] <= 1e-4).all(), (int(well.sum()), e[bad][well].max() if well.any() else 0.0)


def test_cartpole_recompute_mode(device):
    """derived='recompute' (NOT reference behaviour) vs the oracle's recompute variant"""
    rng = np.random.default_rng(3)
    n = 4096
    ctx = random_table(O.CARTPOLE, rng, n)
    s = rng.uniform(-0.2, 0.2, (n, 4)).astype(np.float32)
    a = random_actions(O.CARTPOLE, rng, n)
    s2, _, _, _, _ = run_transitions(O.CARTPOLE, ctx, s, a, device, cartpole_recompute=True)
    want, _, _, _ = O.transitions(O.CARTPOLE, ctx, s.astype(np.float64), a, cartpole_recompute=True)
    assert rel_err(s2, want).max() <= TOL
    stale, _, _, _ = O.transitions(O.CARTPOLE, ctx, s.astype(np.float64), a)
    assert rel_err(s2, stale).max() > 1e-3  # the two modes really differ


def test_acrobot_fp32_mode_is_close_on_typical_states(device):
    rng = np.random.default_rng(4)
    n = 8192
    ctx = random_table(O.ACROBOT, rng, n)
    s = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-3, 3, n),
                  rng.uniform(-6, 6, n)], 1).astype(np.float32)
    a = random_actions(O.ACROBOT, rng, n)
    s2, _, _, _, _ = run_transitions(O.ACROBOT, ctx, s, a, device, acrobot_fp32=True)
    want, _, _, _ = O.transitions(O.ACROBOT, ctx, s.astype(np.float64), a)
    assert rel_err(s2, want).max() <= 5e-5


def test_cartpole_reward_after_termination(device):
    eng = _engine(O.CARTPOLE, [O.default_row(O.CARTPOLE)], 1, device, auto_reset=False)
    eng.reset()
    eng.state.copy_(torch.tensor([[2.39], [3.0], [0.0], [0.0]]))
    _, r, t, _ = eng.step(torch.tensor([1]))
    assert int(t[0]) == 1 and float(r[0]) == 1.0
    _, r, t, _ = eng.step(torch.tensor([1]))
    assert int(t[0]) == 1 and float(r[0]) == 0.0


# ------------------------------------------------------------------ reset / RNG
@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
@pytest.mark.parametrize("sel", [O.SEL_STATIC, O.SEL_ROUND_ROBIN, O.SEL_RANDOM], ids=["static", "rr", "random"])
def test_reset_bit_exact(fam, sel, device):
    """init states (Philox + one fma), context ids, counters and context observations are
    bit-identical to the oracle, over three successive resets and a masked reset"""
    rng = np.random.default_rng(fam * 7 + sel)
    n, n_ctx = 5000, 37
    table = random_table(fam, rng, n_ctx)
    if fam == O.ACROBOT:
        table[:, 10:14] = np.float32([-0.2, 0.3, -0.5, 0.4])
    kw = dict(selector=sel, selector_stride=3, seed=1234567891011, lane_offset=10_000_000_000)
    eng = _engine(fam, table, n, device, **kw)
    ora = O.Engine(fam, table, n, precision="f32", **kw)
    for k in range(3):
        obs = eng.reset().cpu().numpy()
        want = ora.reset()
        np.testing.assert_array_equal(eng.state.t().cpu().numpy(), ora.state)
        np.testing.assert_array_equal(eng.ctx_idx.cpu().numpy(), ora.ctx_idx)
        np.testing.assert_array_equal(eng.n_calls.cpu().numpy(), ora.n_calls)
        np.testing.assert_array_equal(eng.episode.cpu().numpy().view(np.uint32), ora.episode)
        assert rel_err(obs, want).max() <= TOL
        ctx_obs = eng.ctx_obs.cpu().numpy()  # [F, n]
        np.testing.assert_array_equal(ctx_obs, table[ora.ctx_idx].T.astype(np.float32))
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    eng.reset(torch.as_tensor(mask))
    ora.reset(mask)
    np.testing.assert_array_equal(eng.state.t().cpu().numpy(), ora.state)
    np.testing.assert_array_equal(eng.ctx_idx.cpu().numpy(), ora.ctx_idx)
    np.testing.assert_array_equal(eng.n_calls.cpu().numpy(), ora.n_calls)


def test_reset_seed_reproducible_and_distribution(device):
    fam, n = O.CARTPOLE, 200_000
    eng = _engine(fam, [O.default_row(fam)], n, device, selector=0, seed=7)
    a = eng.reset().clone()
    eng.seed(7)
    b = eng.reset().clone()
    assert torch.equal(a, b)
    eng.seed(8)
    c = eng.reset()
    assert not torch.equal(a, c)
    x = a.cpu().numpy()
    assert x.min() >= -0.1 and x.max() < 0.1
    assert abs(x.mean()) < 1e-3 and abs(x.std() - 0.2 / np.sqrt(12)) < 1e-3
    # lanes and state dimensions are uncorrelated
    assert abs(np.corrcoef(x[:-1, 0], x[1:, 0])[0, 1]) < 0.01
    assert abs(np.corrcoef(x[:, 0], x[:, 1])[0, 1]) < 0.01


# ------------------------------------------------------------------ engine rollouts
@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
@pytest.mark.parametrize("sel", [O.SEL_STATIC, O.SEL_ROUND_ROBIN, O.SEL_RANDOM], ids=["static", "rr", "random"])
def test_engine_vs_oracle_stepwise_resync(fam, sel, device):
    """per-step engine semantics with auto-reset, TimeLimit, selectors, episode stats.
    Each step starts from identical fp32 state (the oracle is re-synchronised to the GPU
    state after every step), so 1e-5 applies per transition while flags, counters and
    reset draws must agree exactly for hundreds of steps, episodes included."""
    rng = np.random.default_rng(100 + fam * 3 + sel)
    n, n_ctx = 2048, 11
    table = random_table(fam, rng, n_ctx)
    max_steps = {O.CARTPOLE: 60, O.PENDULUM: 25, O.ACROBOT: 40, O.MOUNTAINCAR: 30, O.MOUNTAINCAR_CONT: 30}[fam]
    kw = dict(selector=sel, selector_stride=2, seed=99, lane_offset=7, max_steps=max_steps)
    ekw = dict(kw)
    ekw["max_episode_steps"] = ekw.pop("max_steps")
    eng = _engine(fam, table, n, device, **ekw)
    ora = O.Engine(fam, table, n, precision="f64", **kw)
    eng.reset()
    ora.reset()
    n_flag_diff = 0
    T = 150
    for t in range(T):
        ora.state[:] = eng.state.t().cpu().numpy()
        a = random_actions(fam, rng, n)
        obs, rew, term, trunc = eng.step(torch.as_tensor(a))
        out = ora.step(a)
        term, trunc = term.cpu().numpy(), trunc.cpu().numpy()
        np.testing.assert_array_equal(trunc, out.truncated)
        fd = term != out.terminated
        n_flag_diff += int(fd.sum())
        ok = ~fd
        assert rel_err(rew.cpu().numpy(), out.reward)[ok].max() <= TOL
        assert rel_err(obs.cpu().numpy(), out.obs)[ok].max() <= TOL
        done = (term | trunc).astype(bool)
        if done.any():
            fo = eng.final_obs.cpu().numpy()
            assert rel_err(fo[done & ok], out.final_obs[done & ok]).max() <= TOL
        if fd.any():
            # only possible for a lane sitting within fp32 resolution of a threshold; its
            # bookkeeping (reset vs no reset) now differs, so stop comparing counters
            assert n_flag_diff <= 2, "termination flags differ on more than threshold-edge lanes"
            return
        np.testing.assert_array_equal(eng.elapsed.cpu().numpy(), ora.elapsed)
        np.testing.assert_array_equal(eng.ctx_idx.cpu().numpy(), ora.ctx_idx)
        np.testing.assert_array_equal(eng.n_calls.cpu().numpy(), ora.n_calls)
        np.testing.assert_array_equal(eng.episodes_done.cpu().numpy(), ora.episodes_done)
        np.testing.assert_array_equal(eng.last_length.cpu().numpy(), ora.last_length)
        assert rel_err(eng.last_return.cpu().numpy(), ora.last_return).max() <= 1e-4
    assert int(eng.episodes_done.sum()) > n  # every lane finished episodes on average


@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
def test_short_free_running_rollout(fam, device):
    """<= 32 steps WITHOUT re-synchronisation from a common reset: fp32 state vs float64
    state drift stays small on these chaotic systems only over short horizons, hence the
    looser 1e-3 here (SURVEY.md section 7 'fp32 vs the reference's fp64 state')."""
    rng = np.random.default_rng(fam)
    n = 1024
    table = random_table(fam, rng, n)
    eng = _engine(fam, table, n, device, selector=0, auto_reset=False, seed=5)
    ora = O.Engine(fam, table, n, selector=0, autoreset=False, seed=5, precision="f64")
    eng.reset()
    ora.reset()
    T = 32 if fam != O.ACROBOT else 8
    for t in range(T):
        a = random_actions(fam, rng, n)
        obs, rew, term, trunc = eng.step(torch.as_tensor(a))
        out = ora.step(a)
    assert rel_err(obs.cpu().numpy(), out.obs).max() <= 1e-3


@pytest.mark.parametrize("n,direct", [(3000, True), (3000, False), (3008, False)],
                         ids=["generic-kernel", "staged-kernel-padded-rows", "staged-kernel"])
@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
def test_rollout_equals_repeated_step_bit_exact(fam, n, direct, device):
    """the fused T-step kernel and T per-call launches are the same arithmetic: round-robin context
    switches on reset (parameter re-gather, ctx_obs rewrite), the finished-episode log and terminal
    observations, through the direct-store kernel (CARL_FLAG_ROLLOUT_DIRECT: dense rows of a lane count that is not
    a multiple of 16), the LDS-staged one on rows padded to a multiple of 16 lanes (round 6: what such a lane count
    takes now) and the LDS-staged one on dense rows (ragged last workgroup)"""
    from carl_amd import _lib

    rng = np.random.default_rng(fam + 50)
    T, n_ctx = 70, 13
    table = random_table(fam, rng, n_ctx)
    acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
    kw = dict(selector=O.SEL_ROUND_ROBIN, seed=3, max_episode_steps=23, fin_capacity=1 << 16)
    e1 = _engine(fam, table, n, device, **kw)
    e2 = _engine(fam, table, n, device, **kw)
    if direct:
        e1.b.flags |= _lib.FLAG_ROLLOUT_DIRECT
    assert e1.rollout_variant() == (_lib.ROLLOUT_DIRECT_FLAG if direct else _lib.ROLLOUT_STAGED)
    e1.reset()
    e2.reset()
    out = e1.rollout(acts, e1.alloc_rollout(T, final_obs=True))
    assert out["reward"].stride(0) == (n if direct else (n + 15) // 16 * 16)
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew)
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc)
        d = (term | trunc).bool()
        assert torch.equal(out["final_obs"][t][d], e2.final_obs[d])
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "last_return", "last_length",
                 "episodes_done", "ctx_obs"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    # finished-episode logs hold the same multiset of (lane, return, length)
    l1, r1, n1, d1 = e1.drain_finished()
    l2, r2, n2, d2 = e2.drain_finished()
    assert d1 == 0 and d2 == 0 and l1.numel() == int(e1.episodes_done.sum())
    k1 = sorted(zip(l1.tolist(), r1.tolist(), n1.tolist()))
    k2 = sorted(zip(l2.tolist(), r2.tolist(), n2.tolist()))
    assert k1 == k2


@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
@pytest.mark.parametrize("T,n", [(1, 1024), (7, 1024), (8, 1024), (9, 1024), (37, 1024), (9, 1008), (17, 272), (8, 16)])
def test_staged_rollout_equals_repeated_step_bit_exact(fam, T, n, device):
    """n % 16 == 0 takes the LDS-staged-output kernel (records drained by the storer waves with
    16-byte stores); chunk boundaries (8 steps), ragged step tails and a ragged LAST WORKGROUP
    (n % 256 != 0) must not matter, and nothing may be written past a row's n entries.
    int64 actions exercise the converting loader path."""
    rng = np.random.default_rng(fam * 10 + T)
    n_ctx = n  # lane <-> context identity, global table
    table = random_table(fam, rng, n_ctx)
    a_np = random_actions(fam, rng, (T, n))
    acts = torch.as_tensor(a_np, device=device)
    if fam not in O.CONTINUOUS and T % 2 == 1:
        acts = acts.to(torch.int64)
    kw = dict(selector=O.SEL_STATIC, seed=3, max_episode_steps=5, ctx_idx0=np.arange(n))
    e1 = _engine(fam, table, n, device, **kw)
    e2 = _engine(fam, table, n, device, **kw)
    e1.reset()
    e2.reset()
    buf = e1.alloc_rollout(T + 1, final_obs=True)  # one sentinel row behind the last step
    buf["obs"][T].fill_(-7.0)
    buf["reward"][T].fill_(-7.0)
    buf["terminated"][T].fill_(9)
    buf["truncated"][T].fill_(9)
    out = e1.rollout(acts, buf)
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew)
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc)
        d = (term | trunc).bool()
        assert torch.equal(out["final_obs"][t][d], e2.final_obs[d])
    assert bool((buf["obs"][T] == -7.0).all()) and bool((buf["reward"][T] == -7.0).all())
    assert bool((buf["terminated"][T] == 9).all()) and bool((buf["truncated"][T] == 9).all())
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name


def test_lds_staged_context_table_matches_global_path(device):
    """C << N stages the [F, C] table in LDS; must be bit-identical to the gather path"""
    fam = O.ACROBOT
    rng = np.random.default_rng(8)
    n, n_ctx, T = 8192, 16, 40  # 16 contexts * 8 <= 8192 lanes -> LDS path
    table = random_table(fam, rng, n_ctx)
    acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
    kw = dict(selector=O.SEL_RANDOM, seed=11, max_episode_steps=17)
    e_lds = _engine(fam, table, n, device, **kw)
    # same contexts, padded with unused rows so that 8 * C > N forces the global path
    big = np.concatenate([table, np.tile(table[:1], (n // 8, 1))])
    e_glb = _engine(fam, big, n, device, ctx_idx0=np.arange(n) % n_ctx, selector=O.SEL_STATIC, seed=11,
                    max_episode_steps=17)
    e_ref = _engine(fam, table, n, device, ctx_idx0=np.arange(n) % n_ctx, selector=O.SEL_STATIC, seed=11,
                    max_episode_steps=17)
    for e in (e_glb, e_ref):
        e.reset()
        o = e.rollout(acts)
    assert torch.equal(e_glb.state, e_ref.state)
    # and the random-selector LDS engine against the oracle's ids
    ora = O.Engine(fam, table, n, selector=O.SEL_RANDOM, seed=11, max_steps=17, precision="f32")
    e_lds.reset()
    ora.reset()
    np.testing.assert_array_equal(e_lds.ctx_idx.cpu().numpy(), ora.ctx_idx)
    np.testing.assert_array_equal(e_lds.state.t().cpu().numpy(), ora.state)


# ------------------------------------------------------------------ compaction
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 5000, 131072, 1_000_003])
@pytest.mark.parametrize("p", [0.0, 0.02, 0.5, 1.0])
def test_done_compact_bit_exact(n, p, device):
    from carl_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(n + int(p * 100))
    term = (rng.random(n) < p).astype(np.uint8)
    trunc = (rng.random(n) < p / 2).astype(np.uint8)
    t_d, u_d = torch.as_tensor(term, device=device), torch.as_tensor(trunc, device=device)
    idx = torch.full((max(n, 1),), -1, dtype=torch.int32, device=device)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=device)
    scratch = torch.zeros(int(lib.carl_done_compact_scratch_elems(n)), dtype=torch.int32, device=device)
    _lib.check(lib.carl_done_compact(t_d.data_ptr(), u_d.data_ptr(), n, idx.data_ptr(), cnt.data_ptr(),
                                     scratch.data_ptr(), torch.cuda.current_stream().cuda_stream))
    want = O.done_compact(term, trunc)
    k = int(cnt.item())
    assert k == want.shape[0]
    np.testing.assert_array_equal(idx[:k].cpu().numpy(), want)


def test_explicit_reset_path_equals_autoreset(device):
    """step (auto-reset off) + done_compact + reset_indexed == step with auto-reset on"""
    fam = O.MOUNTAINCAR
    rng = np.random.default_rng(21)
    n, n_ctx, T = 4096, 9, 90
    table = random_table(fam, rng, n_ctx)
    kw = dict(selector=O.SEL_ROUND_ROBIN, seed=2, max_episode_steps=20)
    e_auto = _engine(fam, table, n, device, auto_reset=True, **kw)
    e_expl = _engine(fam, table, n, device, auto_reset=False, **kw)
    e_auto.reset()
    e_expl.reset()
    for t in range(T):
        a = torch.as_tensor(random_actions(fam, rng, n), device=device)
        o1, r1, t1, u1 = e_auto.step(a)
        o2, r2, t2, u2 = e_expl.step(a)
        assert torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(u1, u2)
        e_expl.reset_done()
        assert torch.equal(o1, e_expl.obs)
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls"):
        assert torch.equal(getattr(e_auto, name), getattr(e_expl, name)), name


# ------------------------------------------------------------------ sharding invariance
def test_lane_sharding_is_invariant(device):
    """1 x N lanes == 4 shards x N/4 lanes with lane_offset (the multi-GPU partition,
    emulated on one device): identical transitions, bit for bit"""
    fam = O.PENDULUM
    rng = np.random.default_rng(33)
    n, T, G = 8192, 50, 4
    table = random_table(fam, rng, n)  # lane i <-> context i, table sharded with the lanes
    acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
    kw = dict(selector=O.SEL_STATIC, seed=77, max_episode_steps=19)
    full = _engine(fam, table, n, device, **kw)
    full.reset()
    out = full.rollout(acts)
    m = n // G
    for g in range(G):
        sl = slice(g * m, (g + 1) * m)
        shard = _engine(fam, table[sl], m, device, lane_offset=g * m, ctx_idx0=np.arange(m), **kw)
        shard.reset()
        o = shard.rollout(acts[:, sl].contiguous())
        assert torch.equal(o["obs"], out["obs"][:, sl])
        assert torch.equal(o["reward"], out["reward"][:, sl])
        assert torch.equal(o["truncated"], out["truncated"][:, sl])
        assert torch.equal(shard.state, full.state[:, sl])


# ------------------------------------------------------------------ full-size properties
def test_full_size_config2_pendulum_properties(device):
    """BASELINE config 2 (65 536 contexts over g and l) at full size: oracle parity on the
    whole batch for one step, then size-independent properties over a long fused rollout"""
    fam, n, T = O.PENDULUM, 65536, 400
    rng = np.random.default_rng(0)
    table = np.tile(O.default_row(fam), (n, 1))
    table[:, 2] = rng.uniform(1, 20, n)
    table[:, 4] = rng.uniform(0.5, 2.0, n)
    table = table.astype(np.float32).astype(np.float64)
    eng = _engine(fam, table, n, device, selector=O.SEL_STATIC, seed=0)
    eng.reset()
    s0 = eng.state.t().cpu().numpy()
    acts = torch.as_tensor(rng.uniform(-2, 2, (T, n)).astype(np.float32), device=device)
    out = eng.rollout(acts)
    w_s, w_obs, w_rew, _ = O.transitions(fam, table, s0.astype(np.float64), acts[0].cpu().numpy())
    assert rel_err(out["obs"][0].cpu().numpy(), w_obs).max() <= TOL
    assert rel_err(out["reward"][0].cpu().numpy(), w_rew).max() <= TOL
    obs = out["obs"]
    assert torch.isfinite(obs).all() and torch.isfinite(out["reward"]).all()
    assert float((obs[..., 0] ** 2 + obs[..., 1] ** 2 - 1).abs().max()) < 1e-5  # cos^2 + sin^2
    assert float(obs[..., 2].abs().max()) <= 8.0  # max_speed clip
    assert float(out["reward"].max()) <= 0.0 and float(out["reward"].min()) >= -(np.pi**2 + 6.4 + 0.004) - 1e-4
    assert int(out["terminated"].sum()) == 0
    trunc = out["truncated"].cpu().numpy()
    assert (trunc[199] == 1).all() and (trunc[399] == 1).all() and trunc.sum() == 2 * n  # TimeLimit 200
    assert (eng.episodes_done == 2).all() and (eng.elapsed == 0).all()
    # the bench's exact kernel (rollout_staged_kernel<Pendulum, PLAIN>) against the oracle, row by row: 16.4 M rows
    assert restep_rollout_with_oracle(fam, table, s0, acts, out, t_max=250) >= 250 * n - n


def test_full_size_config3_mixed_batch_properties(device):
    """BASELINE config 3: Acrobot + MountainCar, 65 536 contexts each, done lanes reset
    in-kernel; checks the episode accounting identities at full size"""
    rng = np.random.default_rng(1)
    n, T = 65536, 600
    for fam in (O.ACROBOT, O.MOUNTAINCAR):
        table = random_table(fam, rng, n)
        eng = _engine(fam, table, n, device, selector=O.SEL_STATIC, seed=4, fin_capacity=1 << 22)
        eng.reset()
        s0 = eng.state.t().cpu().numpy()
        acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
        out = eng.rollout(acts, eng.alloc_rollout(T, final_obs=True))
        # every transition of the first 250 steps re-stepped by the oracle (16.4 M rows per family)
        assert restep_rollout_with_oracle(fam, table, s0, acts, out, t_max=250) >= 250 * n - 8
        done = (out["terminated"] | out["truncated"]).bool()
        # sum over time of done flags == episodes finished == entries in the compact log
        assert torch.equal(done.sum(0).to(torch.int32), eng.episodes_done)
        lanes, rets, lens, dropped = eng.drain_finished()
        assert dropped == 0 and lanes.numel() == int(done.sum())
        limit = 500 if fam == O.ACROBOT else 200
        assert int(lens.max()) <= limit and int(lens.min()) >= 1
        # every step's reward is -1 except the terminating Acrobot step (0): return = -(len) (+1)
        if fam == O.MOUNTAINCAR:
            assert torch.equal(rets, -lens.float())
        assert int(eng.elapsed.max()) < limit
        # elapsed + sum of finished lengths = T for every lane
        total = torch.zeros(n, dtype=torch.int64, device=device).index_add_(0, lanes, lens.long())
        assert torch.equal(total + eng.elapsed.long(), torch.full((n,), T, device=device))


def test_absurd_actions_do_not_spin_the_acrobot(device):
    """an action far outside Discrete(3) (gymnasium asserts on it) sends the angle to ~1e9 rad; the
    reference's `while` wrap loops would spin a wavefront for minutes -- the kernel reduces such an
    angle in one go"""
    import time

    fam = O.ACROBOT
    n = 512
    e = _engine(fam, random_table(fam, np.random.default_rng(0), n), n, device, selector=O.SEL_STATIC, seed=0,
                ctx_idx0=np.arange(n))
    e.reset()
    acts = torch.full((40, n), 1_000_000_000, dtype=torch.int32, device=device)
    t0 = time.perf_counter()
    out = e.rollout(acts)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 5.0  # (values are garbage in, garbage out -- possibly non-finite)
    e.reset()                               # ... and the engine is usable afterwards
    out = e.rollout(torch.ones((10, n), dtype=torch.int32, device=device))
    assert torch.isfinite(out["obs"]).all()


@pytest.mark.parametrize("fam", range(5), ids=O.FAMILY_NAMES)
@pytest.mark.parametrize("T,n,max_steps", [(9, 1024, 5), (37, 1008, 5), (200, 1024, 0), (64, 272, 3)])
def test_staged_rollout_without_optional_outputs_equals_repeated_step(fam, T, n, max_steps, device):
    """The fused rollout in its leanest configuration -- static selector, no terminal observations, no
    finished-episode log -- which for short-episode families (CartPole) runs a done path compiled
    WITHOUT those features (rollout_staged_kernel<Fam, A64, PLAIN = true>) and with the init-state words
    drawn ahead per chunk: bit-identical to T per-call steps of an engine that has them all switched
    on, in every output and every counter, through resets of every lane (max_steps 3 / 5: several
    finishes inside one 8-step chunk) and natural terminations (max_steps 0 = the family's limit)."""
    rng = np.random.default_rng(fam * 7 + T)
    table = random_table(fam, rng, n)
    acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
    kw = dict(selector=O.SEL_STATIC, seed=11, ctx_idx0=np.arange(n))
    if max_steps:
        kw["max_episode_steps"] = max_steps
    e1 = _engine(fam, table, n, device, **kw)                       # lean: PLAIN where the family has it
    e2 = _engine(fam, table, n, device, fin_capacity=1 << 15, **kw)  # everything on, per-call kernel
    e1.reset()
    e2.reset()
    out = e1.rollout(acts, e1.alloc_rollout(T, final_obs=False))
    n_done = 0
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew), t
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), t
        n_done += int((term | trunc).sum())
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "last_return", "last_length",
                 "episodes_done"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    assert int(e1.episodes_done.sum()) == n_done
    if max_steps:
        assert n_done >= n * (T // max_steps)


def test_full_size_cartpole_65536_dense_done_path_properties(device):
    """north_star's workload at full size: CARLCartPole x 65 536 sampled contexts, 250 fused steps, random policy
    (an episode ends every ~22 steps, so the dense done handling of the staged rollout runs on every step).
    (i) the lean kernel (no terminal observations) equals the kernel with terminal observations, and -- a third
    engine with the finished-episode log on -- the generic kernel (the branchy `finish_episodes` path), bit for
    bit in every output and counter; (ii) size-independent
    identities: reward is 1 on every step, an episode's return equals its length, the done flags add up to the
    finished-episode counters, elapsed + finished lengths = T per lane, a terminal observation is out of bounds
    exactly when `terminated` is set, and every reset observation lies inside the CARL init box."""
    fam, n, T = O.CARTPOLE, 65536, 250
    rng = np.random.default_rng(3)
    table = random_table(fam, rng, n)
    acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
    kw = dict(selector=O.SEL_STATIC, seed=21, ctx_idx0=np.arange(n))
    e1 = _engine(fam, table, n, device, **kw)
    e2 = _engine(fam, table, n, device, **kw)
    e1.reset()
    e2.reset()
    e3 = _engine(fam, table, n, device, fin_capacity=1 << 22, **kw)
    e3.reset()
    s0 = e1.state.t().cpu().numpy()
    o1 = e1.rollout(acts)                                      # dense, lean
    o2 = e2.rollout(acts, e2.alloc_rollout(T, final_obs=True))  # dense, terminal observations
    o3 = e3.rollout(acts, e3.alloc_rollout(T, final_obs=True))  # generic done path (finished-episode log on)
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(o1[k], o2[k]) and torch.equal(o1[k], o3[k]), k
    assert torch.equal(o2["final_obs"][(o1["terminated"] | o1["truncated"]).bool()],
                       o3["final_obs"][(o1["terminated"] | o1["truncated"]).bool()])
    for k in ("state", "elapsed", "episode", "n_calls", "ep_return", "last_return", "last_length", "episodes_done"):
        assert torch.equal(getattr(e1, k), getattr(e2, k)) and torch.equal(getattr(e1, k), getattr(e3, k)), k
    assert int(e3.fin_count) == int(e1.episodes_done.sum())
    done = (o1["terminated"] | o1["truncated"]).bool()
    assert float(o1["reward"].min()) == 1.0 and float(o1["reward"].max()) == 1.0
    assert torch.equal(done.sum(0).to(torch.int32), e1.episodes_done)
    assert 8 < T * n / int(done.sum()) < 80  # tens of steps per episode (tau 0.01 .. 0.03; a few lanes survive all 250)
    fin = e1.episodes_done > 0
    assert torch.equal(e1.last_return[fin], e1.last_length[fin].float())
    # terminal observations: out of bounds <=> terminated (x threshold 2.4, theta threshold 12 degrees)
    fo = o2["final_obs"][done]
    term = o1["terminated"][done].bool()
    oob = (fo[:, 0].abs() > 2.4) | (fo[:, 2].abs() > 12 * 2 * np.pi / 360)
    assert torch.equal(oob, term)
    # the observation returned on a done step is the RESET observation: inside the init box of the lane's context
    lo = torch.as_tensor(table[:, 6], device=device, dtype=torch.float32)
    hi = torch.as_tensor(table[:, 7], device=device, dtype=torch.float32)
    t_idx, l_idx = done.nonzero(as_tuple=True)
    ro = o1["obs"][t_idx, l_idx]
    assert bool(((ro >= lo[l_idx, None]) & (ro <= hi[l_idx, None])).all())
    # (iii) the headline's exact kernel -- rollout_staged_kernel<CartPole, PLAIN, AR>, whose outputs equal o2's bit for
    # bit (above) -- against the oracle DIRECTLY: all 65 536 x 250 = 16.4 M transitions re-stepped by `O.transitions`
    # (terminal observations from o2's `final_obs`)
    assert restep_rollout_with_oracle(fam, table, s0, acts, o2) >= T * n - 8


@pytest.mark.parametrize("selector", [O.SEL_ROUND_ROBIN, O.SEL_RANDOM], ids=["round_robin", "random"])
@pytest.mark.parametrize("n_ctx", [37, 3000], ids=["lds_table", "global_table"])
@pytest.mark.parametrize("final", [False, True], ids=["lean", "final_obs"])
@pytest.mark.parametrize("T,n,max_steps", [(41, 1024, 5), (200, 4096, 0)])
def test_cartpole_dense_rollout_with_moving_contexts_equals_repeated_step(selector, n_ctx, T, n, max_steps, final, device):
    """The reference's DEFAULT selector is round robin: every reset moves the lane to another context.  The lean
    fused rollout of CartPole handles that inside its dense done path (selector rule applied and the next context's
    parameters gathered once per chunk, `rollout_staged_kernel<..., PLAIN, LDSCTX, MOVES>`; small tables from LDS,
    large ones from HBM) -- every output, the context ids, the context observation and every counter equal T
    per-call steps of an engine with all optional features on, through several resets per 8-step chunk."""
    fam = O.CARTPOLE
    rng = np.random.default_rng(n_ctx + T)
    table = random_table(fam, rng, n_ctx)
    table[:, 6] = rng.uniform(-0.15, -0.05, n_ctx)  # the init box differs per context too
    table[:, 7] = rng.uniform(0.05, 0.15, n_ctx)
    table = table.astype(np.float32).astype(np.float64)
    acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
    kw = dict(selector=selector, selector_stride=3, seed=17)
    if max_steps:
        kw["max_episode_steps"] = max_steps
    e1 = _engine(fam, table, n, device, **kw)                       # lean: dense + MOVES
    e2 = _engine(fam, table, n, device, fin_capacity=1 << 16, **kw)  # everything on, per-call kernel
    e1.reset()
    e2.reset()
    out = e1.rollout(acts, e1.alloc_rollout(T, final_obs=final))  # final: terminal observations, same dense path
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew), t
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), t
        if final:
            d = (term | trunc).bool()
            assert torch.equal(out["final_obs"][t][d], e2.final_obs[d]), t
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "last_return", "last_length",
                 "episodes_done", "ctx_obs"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    assert int(e1.episodes_done.sum()) > n  # contexts did move
    assert len(torch.unique(e1.ctx_idx)) > min(n_ctx, n) // 4


@pytest.mark.parametrize("n_ctx", [290, 400, 450])
def test_acrobot_rollout_with_a_context_table_near_the_lds_budget(n_ctx, device):
    """the fp64 Acrobot kernels carry an 8 KiB static LDS sin/cos table, and the host's
    "does the context table fit in LDS behind the record buffers" test ignored it -- tables of 16 385 .. 24 576 B
    (293 .. 438 contexts at F = 14) with a moving selector were admitted into the LDS-table kernel and overflowed the
    160 KiB at launch.  Now the static part counts (carl_amd.hip: table_fits): such a batch launches (LDS table
    where it fits, the global table otherwise) and equals repeated per-call steps bit for bit."""
    fam = O.ACROBOT
    rng = np.random.default_rng(n_ctx)
    n, T = 4096, 24
    table = random_table(fam, rng, n_ctx)
    acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
    kw = dict(selector=O.SEL_ROUND_ROBIN, selector_stride=3, seed=19, max_episode_steps=7)
    e1 = _engine(fam, table, n, device, **kw)
    e2 = _engine(fam, table, n, device, **kw)
    e1.reset()
    e2.reset()
    out = e1.rollout(acts)
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew), t
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), t
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done", "ctx_obs"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    assert int(e1.episodes_done.sum()) >= 3 * n


def test_rollout_variant_is_visible_and_odd_lane_counts_take_the_staged_kernel(device):
    """`n_lanes % 16 != 0` took the ~50 % slower direct-store rollout kernel (silently
    at first, with a warning since round 3).  Round 6 (ABI 9): the rollout's arrays carry a ROW PITCH
    (carl_step_io_t::row_pitch); `alloc_rollout` pads rows to a multiple of 16 lanes, so ANY lane count -- 10, 4 100,
    65 537, the uneven shards of `lane_shard` -- takes the staged kernel, without a warning, with the same bits as the
    direct-store kernel writes into dense rows (CARL_FLAG_ROLLOUT_DIRECT, the A/B switch) and as a caller's own dense
    buffers get (which still warn once: that layout cannot take the staged kernel)."""
    import ctypes as C
    import warnings

    from carl_amd import _lib

    rng = np.random.default_rng(5)
    for fam, n, T in ((O.PENDULUM, 4096, 20), (O.PENDULUM, 4100, 20), (O.CARTPOLE, 10, 33), (O.ACROBOT, 263, 17),
                      (O.MOUNTAINCAR, 65537, 12)):
        table = random_table(fam, rng, min(n, 4096))
        acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
        kw = dict(selector=O.SEL_STATIC, seed=2, ctx_idx0=np.arange(n) % min(n, 4096), max_episode_steps=9)
        e = _engine(fam, table, n, device, **kw)
        assert e.rollout_variant() == _lib.ROLLOUT_STAGED
        # the library's answer for DENSE rows of this lane count is unchanged
        assert e.lib.carl_rollout_variant(C.byref(e.b)) == (_lib.ROLLOUT_STAGED if n % 16 == 0 else _lib.ROLLOUT_DIRECT_SHAPE)
        e.reset()
        buf = e.alloc_rollout(T + 1)  # one sentinel row behind the last step: the padding columns must not spill into it
        for k, v in (("obs", -7.0), ("reward", -7.0), ("terminated", 9), ("truncated", 9)):
            buf[k][T].fill_(v)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ref = e.rollout(acts, buf)
        P = (n + 15) // 16 * 16
        assert ref["reward"].stride(0) == P and ref["obs"].shape == (T + 1, n, e.D)
        assert bool((buf["obs"][T] == -7.0).all()) and bool((buf["reward"][T] == -7.0).all())
        assert bool((buf["terminated"][T] == 9).all()) and bool((buf["truncated"][T] == 9).all())
        # (a) the direct-store kernel on dense rows, (b) a caller's own dense buffers
        d = _engine(fam, table, n, device, **kw)
        d.b.flags |= _lib.FLAG_ROLLOUT_DIRECT
        assert d.rollout_variant() == _lib.ROLLOUT_DIRECT_FLAG
        d.reset()
        got = d.rollout(acts)
        assert got["reward"].is_contiguous()
        c = _engine(fam, table, n, device, **kw)
        c.reset()
        own = {"obs": torch.empty((T, n, c.D), device=device), "reward": torch.empty((T, n), device=device),
               "terminated": torch.empty((T, n), dtype=torch.uint8, device=device),
               "truncated": torch.empty((T, n), dtype=torch.uint8, device=device)}
        if n % 16:
            with pytest.warns(RuntimeWarning, match="multiple of 16"):
                c.rollout(acts, own)
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                c.rollout(acts, own)
        for k in ("obs", "reward", "terminated", "truncated"):
            assert torch.equal(ref[k][:T], got[k]), (fam, n, k)
            assert torch.equal(ref[k][:T], own[k]), (fam, n, k)
        for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "last_return", "episodes_done"):
            assert torch.equal(getattr(e, name), getattr(d, name)) and torch.equal(getattr(e, name), getattr(c, name)), name
        assert int(e.episodes_done.sum()) > 0
    # two engines writing side by side into column views of ONE wider array (rows 2 080 lanes long): neither launch may
    # touch the other's columns -- an odd lane count there takes the direct-store kernel (the staged one would write the
    # padding columns, which are the neighbour's), a multiple of 16 keeps the staged kernel
    for n_a, n_b in ((1000, 1080), (1040, 1040)):
        fam = O.PENDULUM
        tab_a, tab_b = random_table(fam, rng, n_a), random_table(fam, rng, n_b)
        acts_a = torch.as_tensor(random_actions(fam, rng, (T, n_a)), device=device)
        acts_b = torch.as_tensor(random_actions(fam, rng, (T, n_b)), device=device)
        P = n_a + n_b
        wide = {"obs": torch.full((T, P, 3), -7.0, device=device), "reward": torch.full((T, P), -7.0, device=device),
                "terminated": torch.full((T, P), 9, dtype=torch.uint8, device=device),
                "truncated": torch.full((T, P), 9, dtype=torch.uint8, device=device)}
        ea = _engine(fam, tab_a, n_a, device, selector=O.SEL_STATIC, seed=2, ctx_idx0=np.arange(n_a))
        eb = _engine(fam, tab_b, n_b, device, selector=O.SEL_STATIC, seed=3, ctx_idx0=np.arange(n_b))
        ra = _engine(fam, tab_a, n_a, device, selector=O.SEL_STATIC, seed=2, ctx_idx0=np.arange(n_a))
        rb = _engine(fam, tab_b, n_b, device, selector=O.SEL_STATIC, seed=3, ctx_idx0=np.arange(n_b))
        for x in (ea, eb, ra, rb):
            x.reset()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ea.rollout(acts_a, {k: v[:, :n_a] for k, v in wide.items()})
            torch.cuda.synchronize()
            assert bool((wide["reward"][:, n_a:] == -7.0).all()) and bool((wide["terminated"][:, n_a:] == 9).all())
            assert bool((wide["obs"][:, n_a:] == -7.0).all())
            eb.rollout(acts_b, {k: v[:, n_a:] for k, v in wide.items()})
        want_a, want_b = ra.rollout(acts_a), rb.rollout(acts_b)
        for k in ("obs", "reward", "terminated", "truncated"):
            assert torch.equal(wide[k][:, :n_a], want_a[k]) and torch.equal(wide[k][:, n_a:], want_b[k]), (n_a, k)
    # a reward array that does not start on a 16-byte boundary (a column view one lane in; rows of 1 040 lanes) takes the
    # direct-store kernel: one warning over two launches, the aligned launches' results
    fam, n, P = O.PENDULUM, 1024, 1040
    tab = random_table(fam, rng, n)
    acts_u = torch.as_tensor(random_actions(fam, rng, (2, T, n)), device=device)
    u = _engine(fam, tab, n, device, selector=O.SEL_STATIC, seed=4, ctx_idx0=np.arange(n))
    r = _engine(fam, tab, n, device, selector=O.SEL_STATIC, seed=4, ctx_idx0=np.arange(n))
    u.reset()
    r.reset()
    view = {"obs": torch.zeros((T, P, 3), device=device)[:, :n], "reward": torch.zeros((T, P), device=device)[:, 1:n + 1],
            "terminated": torch.zeros((T, P), dtype=torch.uint8, device=device)[:, :n],
            "truncated": torch.zeros((T, P), dtype=torch.uint8, device=device)[:, :n]}
    for q in range(2):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            u.rollout(acts_u[q], view)
        assert [w.category for w in caught] == ([RuntimeWarning] if q == 0 else []), caught
        want = r.rollout(acts_u[q])
        for k in ("obs", "reward", "terminated", "truncated"):
            assert torch.equal(view[k], want[k]), (q, k)
    # buffers whose arrays disagree about the pitch are refused
    bad = e.alloc_rollout(T)
    bad["reward"] = torch.empty((T, n), device=device)
    with pytest.raises(ValueError, match="pitch"):
        e.rollout(acts, bad)


@pytest.mark.parametrize("fam", [O.CARTPOLE, O.PENDULUM], ids=["cartpole", "pendulum"])
def test_one_1000_step_launch_equals_four_250_step_launches_at_full_size(fam, device):
    """bench.py's headline launch length (SURVEY 8d's K = 1 000 steps in ONE launch, 65 536 lanes) against the 250-step
    launches the full-size oracle re-step test covers: same bytes in every output row and every counter."""
    n, T = 65536, 1000
    rng = np.random.default_rng(9)
    table = random_table(fam, rng, n)
    acts = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
    kw = dict(selector=O.SEL_STATIC, seed=31, ctx_idx0=np.arange(n))
    e1, e2 = _engine(fam, table, n, device, **kw), _engine(fam, table, n, device, **kw)
    e1.reset()
    e2.reset()
    o1 = e1.rollout(acts)
    for q in range(4):
        o2 = e2.rollout(acts[250 * q: 250 * (q + 1)])
        for k in ("obs", "reward", "terminated", "truncated"):
            assert torch.equal(o1[k][250 * q: 250 * (q + 1)], o2[k]), (q, k)
    for k in ("state", "elapsed", "episode", "n_calls", "ep_return", "last_return", "last_length", "episodes_done"):
        assert torch.equal(getattr(e1, k), getattr(e2, k)), k
    assert int(e1.episodes_done.sum()) >= 4 * n  # TimeLimit 200 / 500: every lane finished episodes inside the launch


# ------------------------------------------------------------------ uint8 actions (ABI 7: rollout-only input format)
@pytest.mark.parametrize("fam", [O.CARTPOLE, O.ACROBOT, O.MOUNTAINCAR], ids=["cartpole", "acrobot", "mountaincar"])
@pytest.mark.parametrize("T,n,auto_reset,max_steps", [(37, 1024, True, 5), (8, 1008, True, 0), (200, 4096, False, 0),
                                                      (5, 16, True, 3), (1000, 512, True, 0)])
def test_uint8_actions_equal_int32_actions_bit_for_bit(fam, T, n, auto_reset, max_steps, device):
    """One byte per lane-step on the launch's only per-step read stream (include/carl_amd.h: CARL_ACTION_U8): the same
    action VALUES as uint8 give the same transitions and the same engine state as int32 -- full and ragged chunks, a
    ragged last workgroup, with and without auto-reset (CartPole: both specialisations of its dense done path), and a
    sentinel row behind the last step stays untouched."""
    rng = np.random.default_rng(fam * 100 + T)
    table = random_table(fam, rng, n)
    a_np = random_actions(fam, rng, (T, n))
    a32 = torch.as_tensor(a_np, device=device)
    a8 = a32.to(torch.uint8)
    kw = dict(selector=O.SEL_STATIC, seed=11, max_episode_steps=max_steps, ctx_idx0=np.arange(n), auto_reset=auto_reset)
    e1, e2 = _engine(fam, table, n, device, **kw), _engine(fam, table, n, device, **kw)
    e1.reset()
    e2.reset()
    buf = e1.alloc_rollout(T + 1)
    for k, v in (("obs", -7.0), ("reward", -7.0), ("terminated", 9), ("truncated", 9)):
        buf[k][T].fill_(v)
    o8 = e1.rollout(a8, buf)
    o32 = e2.rollout(a32)
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(o8[k][:T], o32[k]), k
    assert bool((buf["obs"][T] == -7.0).all()) and bool((buf["terminated"][T] == 9).all())
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name


def test_uint8_actions_outside_the_lean_staged_rollout(device):
    """The library reads uint8 actions in ONE configuration; everywhere else it says CARL_ERR_UNSUPPORTED through the C
    ABI (no silent reinterpretation) and the Python engine widens the actions once -- same results: a moving selector,
    terminal observations, a lane count that is not a multiple of 16, and the per-call step."""
    import ctypes as C

    from carl_amd import _lib

    fam, T = O.CARTPOLE, 21
    rng = np.random.default_rng(5)
    for n, kw, final in ((1024, dict(selector=O.SEL_ROUND_ROBIN), False), (1024, dict(selector=O.SEL_STATIC), True),
                         (1000, dict(selector=O.SEL_STATIC), False)):
        table = random_table(fam, rng, 37)
        a32 = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device)
        a8 = a32.to(torch.uint8)
        kw = dict(seed=4, max_episode_steps=6, **kw)
        e1, e2 = _engine(fam, table, n, device, **kw), _engine(fam, table, n, device, **kw)
        e1.reset()
        e2.reset()
        # straight through the C ABI: declined, nothing launched (the odd lane count: with DENSE rows -- the engine's own
        # buffers pad the rows of such a batch to a multiple of 16 lanes, where uint8 actions are read natively)
        out = e1.alloc_rollout(T, final_obs=final)
        if n % 16:
            out = {k: torch.empty(v.shape, dtype=v.dtype, device=device) for k, v in out.items()}
        io = e1._rollout_io(a8.contiguous(), _lib.ACTION_U8, out, T)
        with torch.cuda.device(device):
            assert e1._c_rollout(io, T) == _lib.ERR_UNSUPPORTED
        assert b"uint8" in e1.lib.carl_last_error()
        # through the engine: widened, same transitions as int32
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (the odd lane count's direct-store warning)
            o8, o32 = e1.rollout(a8, out), e2.rollout(a32, e2.alloc_rollout(T, final_obs=final))
        for k in o32:
            assert torch.equal(o8[k], o32[k]), k
        assert torch.equal(e1.state, e2.state)
        if n % 16:  # ... and on the engine's padded rows the library reads the bytes itself (ABI 9)
            a8b = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device).to(torch.uint8)
            pad = e1.alloc_rollout(T)
            io = e1._rollout_io(a8b, _lib.ACTION_U8, pad, T)
            assert io.row_pitch == 1008
            with torch.cuda.device(device):
                assert e1._c_rollout(io, T) == 0
            o32 = e2.rollout(a8b.to(torch.int32))
            for k in o32:
                assert torch.equal(pad[k], o32[k]), k
            assert torch.equal(e1.state, e2.state)
    # per-call step: uint8 is widened by the engine (the C entry point declines it)
    obs8, *_ = e1.step(a8[0])
    obs32, *_ = e2.step(a32[0])
    assert torch.equal(obs8, obs32)
    io = _lib.StepIO()
    io.action, io.action_dtype = a8[0].contiguous().data_ptr(), _lib.ACTION_U8
    io.obs, io.reward = e1.obs.data_ptr(), e1.reward.data_ptr()
    io.terminated, io.truncated = e1.terminated.data_ptr(), e1.truncated.data_ptr()
    with torch.cuda.device(device):
        assert e1.lib.carl_step(C.byref(e1.b), C.byref(io), e1._stream()) == _lib.ERR_UNSUPPORTED
    # a misaligned uint8 pointer is an invalid argument, not a fault
    n = 1024
    e3 = _engine(fam, random_table(fam, rng, n), n, device, selector=O.SEL_STATIC, ctx_idx0=np.arange(n))
    e3.reset()
    big = torch.zeros(T * n + 8, dtype=torch.uint8, device=device)
    out = e3.alloc_rollout(T)
    io = e3._rollout_io(big[1:1 + T * n].view(T, n), _lib.ACTION_U8, out, T)
    with torch.cuda.device(device):
        assert e3._c_rollout(io, T) == _lib.ERR_INVALID_ARGUMENT
    e3.rollout(big[1:1 + T * n].view(T, n), out)  # the engine re-homes such a view
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
@pytest.mark.parametrize("fam", [O.PENDULUM, O.MOUNTAINCAR_CONT], ids=["pendulum", "mountaincarcont"])
@pytest.mark.parametrize("T,n", [(37, 1024), (8, 1008), (5, 16), (1000, 512)])
def test_half_precision_actions_equal_their_float32_widening_bit_for_bit(fam, dtype, T, n, device):
    """CARL_ACTION_F16 / BF16 (Box families, rollout-only): two bytes per lane-step, widened exactly in the loader wave --
    the transitions are those of the float32 launch fed ``actions.float()``; incl. values outside the action bounds,
    zeros of both signs, subnormal halves, and (configurations the lean kernel does not cover) the engine's widening."""
    rng = np.random.default_rng(fam * 100 + T)
    table = random_table(fam, rng, n)
    a = torch.as_tensor(random_actions(fam, rng, (T, n)), device=device).to(dtype)
    a[0, :8] = torch.tensor([0.0, -0.0, 6.0e-8, -6.0e-8, 3.0, -3.0, 1.0, -1.0], device=device).to(dtype)
    kw = dict(selector=O.SEL_STATIC, seed=11, max_episode_steps=7, ctx_idx0=np.arange(n))
    e1, e2 = _engine(fam, table, n, device, **kw), _engine(fam, table, n, device, **kw)
    e1.reset()
    e2.reset()
    buf = e1.alloc_rollout(T + 1)
    buf["obs"][T].fill_(-7.0)
    oh = e1.rollout(a, buf)
    of = e2.rollout(a.float())
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(oh[k][:T], of[k]), k
    assert bool((buf["obs"][T] == -7.0).all())
    for name in ("state", "elapsed", "episode", "ep_return", "episodes_done"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    if T == 37:  # declined by the library (terminal observations), widened by the engine
        from carl_amd import _lib

        out = e1.alloc_rollout(T, final_obs=True)
        io = e1._rollout_io(a.contiguous(), _lib.ACTION_F16 if dtype == torch.float16 else _lib.ACTION_BF16, out, T)
        with torch.cuda.device(device):
            assert e1._c_rollout(io, T) == _lib.ERR_UNSUPPORTED
        o1, o2 = e1.rollout(a, out), e2.rollout(a.float(), e2.alloc_rollout(T, final_obs=True))
        for k in o2:
            assert torch.equal(o1[k], o2[k]), k
