"""carl_brax_policy_context_trace on the GPU (BraxVecEngine.context_trace): 300 inverted pendulums, 8 steps under a
TimeLimit of 3, so every env is reset twice inside the launch and its context changes there.  Every selector, the default
and the first-state auto-reset modes, auto-reset off, a lane offset far from zero.  The device trace must equal the host
walk of brax_ppo_ref.py exactly, and the walk's continuation past the last step must be the engine's own ctx_idx after the
launch -- the launch and the trace agree on where every env ended up."""
import numpy as np
import pytest
import torch

import brax_policy_cases as BPC
import brax_ppo_ref as BR
from carl_amd import _lib
from carl_amd.brax_engine import BraxVecEngine

pytestmark = pytest.mark.gpu

N, T, N_CTX, STRIDE, SEED = 300, 8, 5, 2, 0x1234567890ABCDEF
SELECTORS = {"static": _lib.SEL_STATIC, "round_robin": _lib.SEL_ROUND_ROBIN, "random": _lib.SEL_RANDOM, "host": _lib.SEL_HOST}
MODES = {"redraw": dict(auto_reset=True, autoreset_mode="redraw"), "first_state": dict(auto_reset=True, autoreset_mode="first_state"),
         "off": dict(auto_reset=False)}


# every selector x mode at lane offset 0; the offset enters the random selector's draws alone: there, both auto-reset modes
CASES = [(s, m, 0) for s in sorted(SELECTORS) for m in sorted(MODES)] + [("random", m, (1 << 32) + 17)
                                                                           for m in ("redraw", "first_state")]


@pytest.mark.parametrize("selector,mode,lane_offset", CASES, ids=[f"{s}-{m}-offset{o}" for s, m, o in CASES])
def test_device_trace_is_the_host_walk(selector, mode, lane_offset):
    dev = "cuda"
    sys_t, names, default = BPC.build_model("inverted_pendulum")
    rows = BPC.context_rows(np.random.default_rng(3), N_CTX, default, names)
    eng = BraxVecEngine(sys_t, len(names), rows, N, dev, selector=SELECTORS[selector], selector_stride=STRIDE, seed=SEED,
                        max_episode_steps=3, lane_offset=lane_offset, **MODES[mode])
    eng.reset()
    ctx0, ep0 = eng.ctx_idx.clone(), eng.episode.clone()
    gen = torch.Generator(device=dev).manual_seed(1)
    actions = torch.rand((T, N, sys_t.n_act), device=dev, generator=gen) * 2 - 1
    buf = eng.rollout(actions)
    te, tr = buf["terminated"][:T], buf["truncated"][:T]
    got = eng.context_trace(ctx0, ep0, te, tr)
    assert got.dtype == torch.int32 and tuple(got.shape) == (T, N)
    te_h, tr_h = te.cpu().numpy() != 0, tr.cpu().numpy() != 0
    assert (te_h | tr_h)[:3].any(axis=0).all() and tr_h.any()  # the TimeLimit: no episode outlives its third step
    ext = lambda a: np.concatenate([a, np.zeros((1, N), bool)])  # noqa: E731  (one more row: the walk's continuation)
    want = BR.context_walk(ctx0.cpu().numpy(), ep0.cpu().numpy().view(np.uint32), ext(te_h), ext(tr_h), SELECTORS[selector],
                           STRIDE, N_CTX, SEED, lane_offset, MODES[mode]["auto_reset"], mode == "first_state")
    np.testing.assert_array_equal(got.cpu().numpy(), want[:T])
    np.testing.assert_array_equal(eng.ctx_idx.cpu().numpy(), want[T])
    moves = selector in ("round_robin", "random") and mode == "redraw"
    assert (want[0] != want[T]).any() == moves
    # into a caller's buffer: the same bits, nothing else written
    out = torch.full((T + 1, N), -7, dtype=torch.int32, device=dev)
    eng.context_trace(ctx0, ep0, te, tr, out=out[:T])
    np.testing.assert_array_equal(out[:T].cpu().numpy(), want[:T])
    assert (out[T] == -7).all()
