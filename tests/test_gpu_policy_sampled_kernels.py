"""Every sampled closed-loop policy kernel (carl_policy_sample.hip: policy_rollout_sampled_kernel<Fam, H, SUMMARY,
LOGP> and policy_episodes_sampled_kernel<Fam, H>: 6 step types x H in {0, 32, 64} x transitions with log_prob,
transitions, summary, episodes = 72 instances) through policy_checks.check_sampled_launch: a float64 reference of the
sampling rule on the exact host reference of the packed policy, within derived bounds (check_rule), every other variant
pinned bit for bit to that launch.  The module's end asserts that all 72 instances were launched and that the exempted
share of discrete lane-steps stayed below 1e-3."""
import numpy as np
import pytest
import torch

import sampling_ref as SR
from carl_amd import _lib
from carl_amd.policy import MLPPolicy
from oracle import oracle as O
from policy_cases import (CTX_MODES, LOG_STDS, OPTIONS, STEP_TYPES, make_engine, make_policy, stacked_policy,
                          zero_head_policy)
from policy_checks import (LAUNCHED, SAMPLED_SEED, SAMPLED_STATS, SAMPLED_VARIANTS, check_sampled_launch,
                           sampled_launch_shape_case, teacher)

pytestmark = pytest.mark.gpu

SAMPLED_ACTS = ["identity", "relu", "tanh"]  # (the order the matrix cycles through)


@pytest.fixture(scope="module", autouse=True)
def every_instance_and_statistics(request):
    yield
    st = SAMPLED_STATS
    line = (f"sampled policies: {st['exempt']} of {st['lane_steps']} discrete lane-steps exempted near a prefix-sum "
            f"boundary; largest log_prob |err| / bound {st['lp_worst_frac']:.3f}; {len(LAUNCHED)} of 72 instances "
            "launched")
    capman = request.config.pluginmanager.getplugin("capturemanager")
    if capman is not None:
        with capman.global_and_fixture_disabled():
            print("\n" + line)
    else:
        print("\n" + line)
    assert SAMPLED_STATS["exempt"] < 1e-3 * max(SAMPLED_STATS["lane_steps"], 1)
    if MATRIX_RUN == set(MATRIX_IDS):  # (the whole matrix ran: not a -k selection)
        want = {(s, H, v) for s in STEP_TYPES for H in (0, 32, 64) for v in SAMPLED_VARIANTS}
        assert want <= LAUNCHED, sorted(want - LAUNCHED)


# ---------------------------------------------------------------- 1 + 2. every instance through every variant
def _matrix():
    """(step type, widths, activation, context mode, clip, log_std, wide head) per case: H = 0, 32, 64 for each step
    type; activation, context mode and clip cycled; Box families cycle log_std; every other discrete case has a wide
    head (logit gaps up to 30 - 90)"""
    shapes = {0: [()], 32: [(31,), (32, 7)], 64: [(64,), (33, 64)]}
    cases = []
    for si, s in enumerate(STEP_TYPES):
        box = STEP_TYPES[s][0] in (_lib.PENDULUM, _lib.MOUNTAINCAR_CONT)
        for hi, H in enumerate((0, 32, 64)):
            k = len(cases)
            ws = shapes[H][si % len(shapes[H])]
            cases.append((s, ws, SAMPLED_ACTS[(si + hi) % 3], CTX_MODES[k % 5], 2.0 if k % 2 else None,
                          LOG_STDS[k % 4] if box else None, not box and (si + hi) % 2 == 0))
    return cases


MATRIX = _matrix()
MATRIX_IDS = [f"{s}-" + ("x".join(map(str, w)) or "linear") + f"-{a}-{c}" + ("-clip" if cl else "")
              + (f"-logstd{ls:g}" if ls is not None else "") + ("-wide" if wide else "")
              for s, w, a, c, cl, ls, wide in MATRIX]
MATRIX_RUN = set()


def widen_head(eng, pol, clip, gap=60.0):
    """pol with its last logit's bias lowered by `gap`: that logit trails the mode by 30 - 90 on every lane-step, so its
    exp(y_k - m) vanishes below S's resolution, while (three actions) the other two still make a real choice.  (A bias
    moves the logits by exact amounts: the forward bound, and with it the exempted share, stays as small as it was.)"""
    layers = [(W.astype(np.float64), b.astype(np.float64)) for W, b in pol.layers]
    W, b = layers[-1]
    b = b.copy()
    b[-1] -= gap
    layers[-1] = (W, b)
    return MLPPolicy.for_env(eng, layers, pol.activation, input_shift=pol.shift, input_scale=pol.scale,
                             input_clip=clip, context_features=pol.ctx_rows)


@pytest.mark.parametrize("step_type, widths, act, ctx, clip, log_std, wide", MATRIX, ids=MATRIX_IDS)
def test_sampled_kernel_matrix(step_type, widths, act, ctx, clip, log_std, wide):
    """n = 1000 (a partial last workgroup, 8 padding lanes); episodes cut at 12 steps and half the lanes reset after 5
    warm-up steps, so that with K = 3 and T = 33 lanes both finish K episodes and fall short of it"""
    k = MATRIX.index((step_type, widths, act, ctx, clip, log_std, wide))
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, 1000, seed=100 + k, max_episode_steps=12, **opts)
    rng = np.random.default_rng(2000 + k)
    pol = make_policy(eng, widths, act, rng, ctx, clip=clip, log_std=log_std)
    if wide:
        pol = widen_head(eng, pol, clip)
    a0 = torch.zeros(eng.n, dtype=torch.int32 if eng.info.action_is_discrete else torch.float32, device=eng.device)
    for _ in range(5):  # (per-call steps: the teacher reads the observation buffer, which a launch does not refresh)
        eng.step(a0)
    eng.reset(torch.arange(eng.n, device=eng.device) % 2)
    out, x, _, _, count = check_sampled_launch(eng, pol, 33, K=3, seed=SAMPLED_SEED + k)
    assert (count == 3).any() and (count < 3).any(), np.bincount(count)
    if wide:
        y = O.policy_forward(pol.params, pol.n_in, pol.widths, pol.n_out, pol.activation, x.reshape(-1, pol.n_in)).y64
        gap = np.sort(y.max(axis=1, keepdims=True) - y, axis=1)[:, 1:]  # the non-mode gaps of each lane-step
        assert gap[:, -1].min() >= 30 and gap[:, -1].max() <= 90, (gap[:, -1].min(), gap[:, -1].max())
        if gap.shape[1] > 1:
            assert (gap[:, 0] < 2).mean() > 0.05, "the other two logits must make a real choice"
        assert np.all(out["action"][:33].cpu().numpy() != pol.n_out - 1)
    MATRIX_RUN.add(MATRIX_IDS[k])


# ---------------------------------------------------------------- 3. launch shapes, with canaries
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 8, 9, 13, 17])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_step_counts(step_type, T):
    sampled_launch_shape_case(step_type, 257, T)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4112])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_lane_counts(step_type, n):
    sampled_launch_shape_case(step_type, n, 13)


# ---------------------------------------------------------------- 4. weight sets
@pytest.mark.parametrize("lanes_per_set", [256, 512])
@pytest.mark.parametrize("step_type", ["cartpole", "pendulum", "acrobot_fast", "mountaincar_cont"])
def test_each_lane_uses_its_own_weight_set(step_type, lanes_per_set):
    n = 1000  # the last set only partly filled, and one set more than the lanes need
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, n, seed=lanes_per_set, max_episode_steps=10, **opts)
    pol = stacked_policy(eng, -(-n // lanes_per_set) + 1, lanes_per_set, np.random.default_rng(lanes_per_set + family))
    assert 3 <= pol.n_sets <= 5
    check_sampled_launch(eng, pol, 21, K=1, plain=False)


# ---------------------------------------------------------------- 5. engine options and offsets
SAMPLED_OPTIONS = {**OPTIONS, "lane_offset_hi": (_lib.PENDULUM, dict(lane_offset=5_000_000_000))}


@pytest.mark.parametrize("option", list(SAMPLED_OPTIONS))
def test_engine_options(option):
    family, opts = SAMPLED_OPTIONS[option]
    n = 600
    eng = make_engine(family, n, seed=7, **opts)
    rng = np.random.default_rng(7)
    if option.startswith("lane_offset"):  # the weight-set index is LOCAL: lane // lanes_per_set, whatever the offset
        check_sampled_launch(eng, stacked_policy(eng, 3, 256, rng, widths=(31,), act="identity"), 29)
        return
    box = family in (_lib.PENDULUM, _lib.MOUNTAINCAR_CONT)
    pol = make_policy(eng, (32, 32), "relu", rng, "all", clip=2.0, log_std=-0.5 if box else None)
    check_sampled_launch(eng, pol, 29)


@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.ACROBOT])
def test_equal_logits_take_the_words_of_global_lanes(family):
    """an engine of n lanes at lane_offset L draws the words of global lanes L .. L + n - 1 (the counter's hi word
    non-zero): exact, as test_equal_logits_take_the_documented_words"""
    n, T, L = 512, 200 if family == _lib.CARTPOLE else 600, 5_000_000_000
    eng = make_engine(family, n, _lib.SEL_RANDOM, n_contexts=16, seed=3, lane_offset=L)
    pol = zero_head_policy(eng, widths=(8,))
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SAMPLED_SEED, log_prob=True)
    acts = out["action"][:T]
    assert bool((out["terminated"] | out["truncated"]).any()), "the launch must cross auto-resets"
    _, e, el = teacher(eng, pol, snap, acts)
    w = SR.sample_words(SAMPLED_SEED, np.broadcast_to(L + np.arange(n, dtype=np.uint64), (T, n)), e, el)
    na = int(eng.info.n_actions)
    np.testing.assert_array_equal(acts.cpu().numpy(), SR.categorical_equal_logits(SR.u_categorical(w[0]), na))
    np.testing.assert_allclose(out["log_prob"][:T].cpu().numpy(), np.full((T, n), -np.log(na)), rtol=2.5e-7, atol=0)
    lo = SR.sample_words(SAMPLED_SEED, np.broadcast_to(np.arange(n, dtype=np.uint64) + (L & 0xFFFFFFFF), (T, n)), e, el)
    assert (SR.categorical_equal_logits(SR.u_categorical(lo[0]), na) != acts.cpu().numpy()).mean() > 0.3
