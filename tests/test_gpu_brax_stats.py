"""Input statistics inside the Brax episodes launch (include/carl_amd.h: carl_brax_evaluate_policy_stats;
BraxVecEngine.evaluate_episodes(..., input_stats=True)) and their merge (carl_brax_policy_stats_merge; InputStats with a
BraxMLPPolicy template) on the GPU.

The statistics launch IS the episodes launch: its records and engine state are held to the same two references
(brax_episodes_cases.check_records / check_state), bit for bit.  Its slabs are held to stats_ref.input_sums of the exact
input trace (brax_stats_cases.input_trace) within the bound the header states, derived in brax_stats_cases' docstring.
Shapes are the episodes tests': 77 envs, TimeLimit 5, 12 steps, 5 round-robin contexts, brax_episodes_cases.spread_start."""
import faulthandler

import numpy as np
import pytest
import torch

import brax_episodes_cases as BE
import brax_policy_cases as BP
import brax_stats_cases as BS
import stats_ref as SR
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import InputStats

pytestmark = pytest.mark.gpu

N, T = BE.N, BE.MAX_STEPS
CANARY = 16  # slabs of canaries behind the last slab


def bits64(t):
    return t.contiguous().view(torch.int64)


def stats_launch(eng, pol, snap, K, steps, n_slabs=None):
    """one statistics launch from `snap` into a slab buffer with NaN canaries behind it -> (result, full_state after)"""
    n_slabs = BS.slab_count(eng, pol, steps) if n_slabs is None else n_slabs
    assert n_slabs > 0
    buf = torch.full((n_slabs + CANARY, 2, SR.MAX_IN), float("nan"), dtype=torch.float64, device=eng.device)
    out = eng.alloc_policy_episodes(K)
    out["input_partial"] = buf[:n_slabs]
    eng.restore(snap)
    res = eng.evaluate_episodes(pol, K, steps, out=out, input_stats=True)
    assert res is out and res["input_partial"].data_ptr() == buf.data_ptr()
    assert bool(torch.isnan(buf[n_slabs:]).all()), "a canary behind the last slab was written"
    assert not bool(torch.isnan(buf[:n_slabs]).any()), "a slab was not written in full"
    return res, BE.full_state(eng)


def check_stats_launch(eng, pol, snap, ref, x, K, steps, label):
    """records, state, slabs, repeatability and slab count of one statistics launch -> (result, stop steps)"""
    res, after = stats_launch(eng, pol, snap, K, steps)
    stop = BE.check_records(res, snap, ref, K, steps)
    BE.check_state(eng, pol, snap, after, stop)
    sh = BS.shape_of(eng, pol, steps)
    assert res["input_partial"].shape[0] == sh.grid * sh.waves_per_workgroup
    BS.check_sums(eng, pol, res["input_partial"], x, stop, steps, label)
    again, _ = stats_launch(eng, pol, snap, K, steps)
    assert torch.equal(bits64(res["input_partial"]), bits64(again["input_partial"]))
    return res, stop


def frozen_beside_live(eng, stop):
    """a wavefront with an env already frozen while another is still live: two distinct stop steps in one wavefront"""
    per = BE.envs_per_wavefront(eng)
    return any(len(set(stop[g: g + per].tolist())) >= 2 for g in range(0, stop.size, per))


@pytest.mark.parametrize("model,width", BP.instance_cases(), ids=str)
def test_every_kernel_instance(device, model, width):
    """test 1: every instantiated (class, width), K = 2, from spread_start: envs of one wavefront freeze at different
    steps, and 77 envs leave a partial last wavefront at every width but 9 (7 envs per wavefront)"""
    case = BP.instance_cases().index((model, width))
    seed = 11000 + 100 * list(BP.MODELS).index(model) + width
    eng = BE.make_engine(model, width, N, device, seed)
    widths, act = BP.NETWORKS[case % len(BP.NETWORKS)]
    pol = BE.make_policy(eng, widths, act, seed + 1)
    assert pol.shift.any() and np.any(pol.scale != 1)  # d is taken before the scale and the clip
    snap = BE.spread_start(eng, seed + 2)
    ref = BE.reference(eng, pol, snap, T)
    x = BS.input_trace(eng, pol, snap, ref[0]["action"], T)
    res, stop = check_stats_launch(eng, pol, snap, ref, x, 2, T, f"{model}/{width}")
    assert frozen_beside_live(eng, stop) and stop.min() < T
    # the same launch without the statistics: the same records, and the reused dict loses the key
    eng.restore(snap)
    keep = {k: v.clone() for k, v in res.items() if k != "input_partial"}
    plain = eng.evaluate_episodes(pol, 2, T, out=res)
    assert plain is res and "input_partial" not in res
    for k, v in keep.items():
        a, b = (t.view(torch.int32) if t.is_floating_point() else t for t in (v, res[k]))
        assert torch.equal(a, b), k


def test_liveness_is_what_is_counted(device):
    """test 2: one snapshot at K = 1 and K = 3.  The K = 1 sums are the reference over each env's first steps[env] steps
    only: a kernel that also counts the steps a frozen env computes along, or an env past the end of the batch (hopper at 4
    lanes per env: 16 envs per wavefront, 77 = 4 x 16 + 13), fails the bound by whole terms."""
    eng = BE.make_engine("hopper", 4, N, device, 201)
    assert N % BE.envs_per_wavefront(eng) != 0
    pol = BE.make_policy(eng, (32,), "relu", 202)
    snap = BE.spread_start(eng, 203)
    ref = BE.reference(eng, pol, snap, T)
    x = BS.input_trace(eng, pol, snap, ref[0]["action"], T)
    res1, stop1 = check_stats_launch(eng, pol, snap, ref, x, 1, T, "K=1")
    res3, stop3 = check_stats_launch(eng, pol, snap, ref, x, 3, T, "K=3")
    assert frozen_beside_live(eng, stop1)
    assert (stop1 < stop3).any() and stop1.sum() < stop3.sum()
    assert int(res1["steps"].sum()) == stop1.sum()
    # the check is sharp: the steps the frozen envs compute along (K = 3 has them live) move the reference's friction sum by
    # more than a million times what the bound admits
    w1, _, a1 = SR.input_sums(x, stop1, BS.env_shift(pol, N))
    w3 = SR.input_sums(x, stop3, BS.env_shift(pol, N))[0]
    f = BS.bound_factor(eng, pol, T, res1["input_partial"].shape[0]) * BS.U64
    assert abs(w3[1] - w1[1]) > 1e6 * f * a1[1]


def test_two_weight_sets_with_different_shifts_inside_one_wavefront(device):
    """test 3: Ant at 9 lanes per env is 7 envs per wavefront; 512 envs in sets of 256: wavefront 36 holds envs of both
    sets, whose shifts differ"""
    n, steps = 512, 8
    eng = BE.make_engine("ant", 9, n, device, 41)
    assert (256 // 7) * 7 < 256 < (256 // 7 + 1) * 7
    pol = BraxMLPPolicy.stack([BE.make_policy(eng, (64, 64), "relu", 400 + k) for k in range(2)], 256)
    sh = BS.env_shift(pol, n)
    assert sh.shape == (n, pol.n_in) and np.all(sh[0] != sh[256]) and np.array_equal(sh[255], sh[0])
    snap = BE.spread_start(eng, 42)
    ref = BE.reference(eng, pol, snap, steps)
    x = BS.input_trace(eng, pol, snap, ref[0]["action"], steps)
    res, stop = check_stats_launch(eng, pol, snap, ref, x, 1, steps, "two sets")
    assert len(set(stop[252:259].tolist())) >= 2  # the wavefront of both sets has envs frozen at different steps
    # under one set's shift for every env the sums are far from the device's: the launch used each env's own
    w1 = SR.input_sums(x, stop, sh[0])[0]
    s1, _ = BS.slab_sums(res["input_partial"], pol.n_in)
    assert np.all(np.abs(s1 - w1) > 1e-3 * np.abs(sh[0] - sh[256]) * stop[256:].sum())


@pytest.mark.parametrize("K", [1, 3])
def test_fragment_hand_over(device, K):
    """test 4: a group cut between two wavefronts -- both wavefronts sum their own steps of it.  Runs once under its own time
    limit, as the episodes test does: a launch that does not finish ends the process."""
    n, sh, wait = BS.hand_over_count(T)
    eng = BE.make_engine("ant", 16, n, device, 51)
    pol = BE.make_policy(eng, (64, 64), "tanh", 52)
    snap = BE.spread_start(eng, 53)
    ref = BE.reference(eng, pol, snap, T)
    x = BS.input_trace(eng, pol, snap, ref[0]["action"], T)
    n_slabs = BS.slab_count(eng, pol, T)
    assert n_slabs == sh.grid * sh.waves_per_workgroup
    torch.cuda.synchronize()
    faulthandler.dump_traceback_later(120, exit=True)  # (a hung launch ends the process: nothing more runs on the GPU)
    try:
        res, after = stats_launch(eng, pol, snap, K, T, n_slabs)
        torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()
    stop = BE.check_records(res, snap, ref, K, T)
    BE.check_state(eng, pol, snap, after, stop)
    BS.check_sums(eng, pol, res["input_partial"], x, stop, T, f"hand-over K={K}")
    if K == 3:
        assert [f for f in wait if (stop[4 * f[2]: 4 * f[2] + 4] > f[3]).any()], "no live env crossed a hand-over"


def _section(block, pol):
    off = pol.weight_floats
    return block.reshape(-1, pol.set_floats)[:, off: off + 2 * pol.n_in].cpu().numpy()


def test_merge_and_the_constant_rule(device):
    """test 5: friction is the same in all 5 contexts, gravity differs; both start with shift 0 (nothing centred).  One
    launch and one InputStats.update: friction's scale is exactly 0 and its shift fp32(friction), gravity's scale is not 0,
    every decided input equals stats_ref.merge of the device slabs bit for bit; a second launch under the new shift and a
    second merge equal the reference's Chan update; the rest of the written sets keeps its bits."""
    friction = 0.8125

    def rows_of(rows, names):
        rows[:, names.index("friction")] = friction

    eng, names = BS.make_engine_with_rows("hopper", 4, N, device, 301, rows_of)
    tab = eng.ctx_table.cpu().numpy()
    g_row, f_row = names.index("gravity"), names.index("friction")
    assert len(set(tab[f_row].tolist())) == 1 and len(set(tab[g_row].tolist())) == BE.N_CTX
    tmpl = BE.make_policy(eng, (32,), "tanh", 302)
    assert list(tmpl.ctx_rows) == [g_row, f_row]
    n_in, off, S = tmpl.n_in, tmpl.weight_floats, tmpl.set_floats
    host = np.stack([tmpl.params[0], BE.make_policy(eng, (32,), "tanh", 303).params[0]])
    host[:, off: off + 2 * n_in + 1] = host[0, off: off + 2 * n_in + 1]  # one transform for both sets
    host[:, off: off + 2] = 0.0                                          # gravity and friction: nothing centred
    block = torch.as_tensor(host).to(device).contiguous()
    pol = BraxMLPPolicy.on_device(tmpl, block, 256)
    assert type(pol) is BraxMLPPolicy
    stats = InputStats(tmpl, device)
    snap = BE.spread_start(eng, 304)
    ref, rtol = SR.fresh(n_in), 1e-12
    for launch in range(2):
        before = block.clone()
        shift = before[0, off: off + n_in].cpu().numpy()
        eng.restore(snap)
        res = eng.evaluate_episodes(pol, 2, T, input_stats=True)
        stats.update(res, pol, n_write=1)
        n_b = int(res["steps"].sum())
        ref, sh, sc = SR.merge(ref, res["input_partial"].cpu().numpy(), n_b, shift)
        assert int(stats.count) == ref["count"] and n_b > 0
        np.testing.assert_allclose(stats.mean.cpu().numpy(), ref["mean"], rtol=rtol, atol=0)
        np.testing.assert_allclose((stats.var * stats.count).cpu().numpy(), ref["m2"], rtol=rtol, atol=1e-300)
        ok = SR.settled(ref, stats.eps, stats.min_std, 4 * rtol)
        assert ok[:2].all() and ok.sum() >= n_in - 2, ok
        sec = _section(block, tmpl)
        np.testing.assert_array_equal(sec[0, :n_in][ok].view(np.uint32), sh[ok].view(np.uint32))
        np.testing.assert_array_equal(sec[0, n_in:][ok].view(np.uint32), sc[ok].view(np.uint32))
        assert sec[0, n_in + 1] == 0.0 and sec[0, 1] == np.float32(friction) == tab[f_row][0]
        assert sec[0, n_in] > 0.0 and np.all(sec[0, n_in + 2:] > 0.0)
        keep = torch.ones(S, dtype=torch.bool, device=device)
        keep[off: off + 2 * n_in] = False
        assert torch.equal(block[0, keep].view(torch.int32), before[0, keep].view(torch.int32))
        assert torch.equal(block[1].view(torch.int32), before[1].view(torch.int32))  # beyond n_write
        block[1, off: off + 2 * n_in] = block[0, off: off + 2 * n_in]  # the next launch: one shift for every set
    assert not np.array_equal(shift[:2], np.zeros(2, np.float32))  # the second launch ran centred
    # transform / apply_to / state_dict with a Brax template
    sh, sc = SR.transform(ref)
    got_sh, got_sc = stats.transform()
    np.testing.assert_array_equal(got_sh[ok], sh[ok])
    np.testing.assert_array_equal(got_sc[ok], sc[ok])
    applied = stats.apply_to(tmpl)
    assert type(applied) is BraxMLPPolicy
    np.testing.assert_array_equal(applied.shift, got_sh)
    np.testing.assert_array_equal(applied.scale, got_sc)
    other = InputStats(tmpl, device)
    other.load_state_dict(stats.state_dict())
    for k, v in other.state_dict().items():
        assert torch.equal(v, stats.state_dict()[k]), k


@pytest.mark.parametrize("model,width,mode", [("hopper", 4, "redraw"), ("ant", 9, "first_state")], ids=str)
def test_auto_reset_modes_caller_buffers_and_no_steps(device, model, width, mode):
    """test 7: both auto-reset modes; a caller-provided `out` with 'input_partial'; max_steps = 0 writes every slab
    carl_brax_policy_stats_slabs reports for it (the count of a one-step launch) as zeros and leaves the state alone"""
    eng = BE.make_engine(model, width, N, device, 61, autoreset_mode=mode)
    if mode == "first_state":
        eng.reset()  # (the first_state copy is taken by an explicit reset)
    pol = BE.make_policy(eng, (32,), "relu", 62)
    snap = BE.spread_start(eng, 63)
    ref = BE.reference(eng, pol, snap, T)
    x = BS.input_trace(eng, pol, snap, ref[0]["action"], T)
    check_stats_launch(eng, pol, snap, ref, x, 2, T, f"{model} {mode}")
    n0 = BS.slab_count(eng, pol, 0)
    assert n0 == BS.slab_count(eng, pol, 1) > 0
    eng.restore(snap)
    before = BE.full_state(eng)
    res0, now = stats_launch(eng, pol, snap, 2, 0, n0)
    assert not bits64(res0["input_partial"]).any()  # +0.0 everywhere
    assert int(res0["episodes"].abs().sum()) == 0 and int(res0["steps"].abs().sum()) == 0
    assert bool(torch.isnan(res0["return"]).all()) and bool((res0["context_id"] == -1).all())
    for k, a in before.items():
        b = now[k]
        if a.is_floating_point():
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k
    stats = InputStats(pol, device)  # an empty launch merges to nothing
    blk = torch.as_tensor(pol.params).to(device).contiguous().clone()
    stats.update(res0, blk, policy=BraxMLPPolicy.on_device(pol, blk.clone(), 256))
    assert int(stats.count) == 0 and torch.equal(blk.view(torch.int32), torch.as_tensor(pol.params).to(device).view(torch.int32))
    bad = eng.alloc_policy_episodes(2)
    bad["input_partial"] = torch.zeros((n0 + 1, 2, SR.MAX_IN), dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match="input_partial"):
        eng.evaluate_episodes(pol, 2, 0, out=bad, input_stats=True)
