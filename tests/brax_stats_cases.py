"""Toolkit of the tests of the input statistics of the Brax closed-loop rollout (test_gpu_brax_stats.py and
test_gpu_brax_stats_es.py on the GPU, test_brax_stats_abi.py on the host; include/carl_amd.h:
carl_brax_evaluate_policy_stats, carl_brax_policy_stats_slabs, carl_brax_policy_stats_merge).

The reference input trace: the episodes launch is bit-identical to a per-call replay of the transitions launch's actions
(brax_episodes_cases.reference), so reading eng.obs and eng.ctx_idx before each step of that replay gives every raw input
the policy acted on, exactly: x[t, env] = the context-table values of that ctx_idx in the policy's row order, then that
observation.  stats_ref.input_sums turns the trace into float64 sums and the scales of the bound.

The bound, from the header's operation list: every term is exact in float64 and a slab entry is a recursive float64 sum, per
wavefront-step over at most `envs per wavefront` terms from +0.0 and then over the wavefront's steps, so with u = 2^-53 it is
within (s + envs per wavefront) u sum|terms| of exact, s the wavefront-steps of the slab.  The tests add the slabs in slab
order (n_slabs - 1 more additions) and compare with a NumPy pairwise sum of T n terms (ceil(log2(T n)) roundings per
term): bound_factor() adds the four counts.  No measured figure enters it.

A plain module: importing it allocates nothing and touches no device."""
import math

import numpy as np
import torch

import brax_episodes_cases as BE
import brax_policy_cases as BP
import stats_ref as SR
from carl_amd import _lib

U64 = 2.0 ** -53


def make_engine_with_rows(model, width, n, device, seed, rows_of, **kw):
    """brax_episodes_cases.make_engine with the context rows edited by rows_of(rows, names) before the engine is built"""
    from carl_amd.brax_engine import BraxVecEngine
    from brax_kernel_cases import touch_down
    from oracle import oracle as O

    s, names, default = BP.build_model(model)
    s.lanes_per_env = width
    rng = np.random.default_rng(seed)
    rows = BP.context_rows(rng, BE.N_CTX, default, names)
    rows_of(rows, names)
    kw.setdefault("max_episode_steps", BE.TIME_LIMIT)
    eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_ROUND_ROBIN, seed=seed,
                        ctx_obs_rows=[names.index("gravity"), names.index("friction")], **kw)
    assert width in eng.lane_widths()
    eng.reset()
    if model in BP.GROUND:
        eng.set_state64(touch_down(eng.sys, eng.state64().cpu().numpy()))
    return eng, names


def input_trace(eng, pol, snap, actions, steps):
    """x [steps, n, n_in] float32: every env's raw policy inputs before each step of a per-call replay of `actions` from
    `snap`.  Leaves the engine wherever the replay ends."""
    eng.restore(snap)
    tab = eng.ctx_table.cpu().numpy()[list(pol.ctx_rows)]  # [n_ctx, C]
    xs = []
    for t in range(steps):
        c = eng.ctx_idx.cpu().numpy().astype(np.int64)
        xs.append(np.concatenate([tab[:, c].T.astype(np.float32), eng.obs.cpu().numpy()], axis=1))
        eng.step(actions[t].contiguous())
    x = np.stack(xs)
    assert x.dtype == np.float32 and x.shape == (steps, eng.n, pol.n_in)
    return x


def env_shift(pol, n):
    """[n, n_in] float32: the shift of each env's own weight set"""
    sec = np.asarray(pol.transform_section(), np.float32)[:, : pol.n_in]
    per = pol.lanes_per_set if pol.lanes_per_set is not None else n
    return sec[np.arange(n) // per]


def slab_count(eng, pol, max_steps):
    st = pol.struct(eng.n, None)
    return int(_lib.load().carl_brax_policy_stats_slabs(eng.b, eng.sys, st, max_steps))


def shape_of(eng, pol, max_steps):
    code, sh = BP.launch_shape(eng.b, eng.sys, pol.struct(eng.n, None), max_steps)
    assert code == 0
    return sh


def bound_factor(eng, pol, max_steps, n_slabs):
    """the factor of u sum|terms| the sum of the slabs in slab order may differ from stats_ref.input_sums by (module
    docstring): the most wavefront-steps of one slab, the envs per wavefront, the slabs, the reference's own depth"""
    sh = shape_of(eng, pol, max_steps)
    per_wave = {}
    for wg, wave, _, t_lo, t_hi, _, _ in BP.fragments(sh, eng.n, max_steps):
        per_wave[(wg, wave)] = per_wave.get((wg, wave), 0) + (t_hi - t_lo)
    s = max(per_wave.values())
    return s + 64 // sh.lanes_per_env + n_slabs + math.ceil(math.log2(max_steps * eng.n)) + 1


def slab_sums(partial, n_in):
    """(S1, S2) [n_in]: the slabs added in slab order, as carl_brax_policy_stats_merge adds them"""
    p = partial.cpu().numpy() if isinstance(partial, torch.Tensor) else np.asarray(partial)
    s1, s2 = np.zeros(n_in), np.zeros(n_in)
    for w in range(p.shape[0]):
        s1 = s1 + p[w, 0, :n_in]
        s2 = s2 + p[w, 1, :n_in]
    return s1, s2


def check_sums(eng, pol, partial, x, steps, max_steps, label=""):
    """the device slabs against the reference over each env's first steps[env] steps, per input, within the derived bound;
    entries at and beyond n_in are +0.0.  Prints each figure before it asserts."""
    n_in = pol.n_in
    p = partial.cpu().numpy()
    assert p.dtype == np.float64 and p.shape[1:] == (2, SR.MAX_IN)
    tail = np.ascontiguousarray(p[:, :, n_in:])
    assert not tail.view(np.uint64).any(), "entries at and beyond n_in must be +0.0 (bit pattern 0)"
    w1, w2, a1 = SR.input_sums(x, steps, env_shift(pol, eng.n))
    s1, s2 = slab_sums(p, n_in)
    f = bound_factor(eng, pol, max_steps, p.shape[0]) * U64
    e1, e2 = np.abs(s1 - w1), np.abs(s2 - w2)
    print(f"{label}: {p.shape[0]} slabs, factor {f / U64:.0f} u; max |dS1| / (f sum|d|) = "
          f"{np.max(e1 / np.maximum(f * a1, 1e-300)):.3f}, max |dS2| / (f sum d^2) = {np.max(e2 / np.maximum(f * w2, 1e-300)):.3f}")
    assert np.all(e1 <= f * a1), (e1, f * a1)
    assert np.all(e2 <= f * w2), (e2, f * w2)
    return s1, s2


def hand_over_count(steps):
    """the smallest Ant env count at 16 lanes per env whose closed-loop launch of `steps` steps has a wait_head fragment:
    (n, launch shape, the wait_head fragments) -- test_gpu_brax_episodes.py's search, restated (test files are not imported)"""
    s = BP.build_model("ant")[0]
    s.lanes_per_env = 16

    def shape(n):
        b = _lib.Batch()
        b.n_lanes, b.flags = n, _lib.FLAG_AUTORESET
        code, sh = BP.launch_shape(b, s, _lib.Policy(), steps)
        assert code == 0 and sh.lanes_per_env == 16
        return sh

    g = 1
    while g < 1 << 13:
        sh = shape(4 * (g - 1) + 1)
        if sh.grid * sh.waves_per_workgroup < g:
            break
        g += 1
    n = 4 * (g - 1) + 1
    sh = shape(n)
    wait = [f for f in BP.fragments(sh, n, steps) if f[5]]
    assert wait, "no wait_head fragment"
    return n, sh, wait
