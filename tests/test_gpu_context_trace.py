"""carl_policy_context_trace on the GPU: the context each step of a closed-loop launch ran in, rebuilt from the launch's
flag rows, against ``ctx_idx`` read before each of T per-call steps that replay the recorded actions from a restored
snapshot -- three selectors, auto-reset on and off, a moving round robin of stride 3 over 7 contexts, episodes of 5 steps
(every lane resets at least twice in 12 steps), global lane ids above 2^32, dense and padded rows."""
import numpy as np
import pytest
import torch

import policy_cases as PC
import ppo_ref as R
from carl_amd import _lib

pytestmark = pytest.mark.gpu

T, N, C = 12, 80, 7
CANARY = -12345


@pytest.fixture(scope="module", params=sorted(PC.SELECTORS))
def traced(request):
    """per selector and auto-reset setting: (engine, ctx_idx0, episode0, the launch's output, the per-call ctx_idx rows)"""
    runs = {}
    for auto_reset in (True, False):
        eng = PC.make_engine(_lib.CARTPOLE, N, PC.SELECTORS[request.param], n_contexts=C, seed=11, selector_stride=3,
                             lane_offset=(1 << 32) + 5, max_episode_steps=5, auto_reset=auto_reset)
        pol = PC.random_policy(eng, seed=3, widths=(8,))
        snap = eng.snapshot()
        ctx0, ep0 = eng.ctx_idx.clone(), eng.episode.clone()
        out = eng.rollout_policy(pol, T, deterministic=False, sample_seed=3)
        eng.restore(snap)
        want = torch.empty((T, N), dtype=torch.int32, device=eng.device)
        for t in range(T):
            want[t] = eng.ctx_idx
            eng.step(out["action"][t])
        runs[auto_reset] = (eng, ctx0, ep0, out, want.cpu().numpy())
    return request.param, runs


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_auto_reset"])
@pytest.mark.parametrize("pitch", [N, 96], ids=["dense", "padded"])
def test_trace_equals_per_call_ctx_idx(traced, auto_reset, pitch):
    selector, runs = traced
    eng, ctx0, ep0, out, want = runs[auto_reset]
    flags = {}
    for k in ("terminated", "truncated"):
        full = torch.zeros((T, pitch), dtype=torch.uint8, device=eng.device)
        full[:, :N] = out[k][:T]
        full[:, N:] = 1  # (a padding column's flags must not matter)
        flags[k] = full[:, :N]
    buf = torch.full((T, pitch), CANARY, dtype=torch.int32, device=eng.device)
    got = eng.context_trace(ctx0, ep0, flags["terminated"], flags["truncated"], out=buf[:, :N])
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert (buf[:, N:] == CANARY).all()
    done = (out["terminated"][:T] | out["truncated"][:T]).cpu().numpy().astype(bool)
    assert done.sum(axis=0).min() >= 2  # every lane was reset at least twice (or stayed done, without auto-reset)
    if auto_reset and selector != "static":
        assert (want != want[0]).any()  # the contexts moved
    else:
        assert (want == want[0]).all()
    # the host restatement of the walk agrees
    ref = R.context_walk(ctx0.cpu().numpy(), ep0.cpu().numpy(), out["terminated"][:T].cpu().numpy(),
                         out["truncated"][:T].cpu().numpy(), PC.SELECTORS[selector], 3, C, 11, (1 << 32) + 5, auto_reset)
    np.testing.assert_array_equal(ref, want)


def test_trace_allocates_rows_of_the_flags_pitch():
    eng = PC.make_engine(_lib.PENDULUM, 20, n_contexts=C, max_episode_steps=5)
    pol = PC.random_policy(eng, widths=())
    ctx0, ep0 = eng.ctx_idx.clone(), eng.episode.clone()
    out = eng.rollout_policy(pol, 7)  # rows of carl_rollout_pitch(20) = 32 lanes
    got = eng.context_trace(ctx0, ep0, out["terminated"], out["truncated"])
    assert got.shape == (7, 20) and got.stride(0) == 32
    ref = R.context_walk(ctx0.cpu().numpy(), ep0.cpu().numpy(), out["terminated"].cpu().numpy(),
                         out["truncated"].cpu().numpy(), _lib.SEL_ROUND_ROBIN, 1, C, 0, 0, True)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    with pytest.raises(ValueError, match="ctx_idx0"):
        eng.context_trace(ctx0.long(), ep0, out["terminated"], out["truncated"])
