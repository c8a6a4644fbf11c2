"""The edges of the two PPO gradient units on the GPU -- carl_ppo_grad (ppo_net_kernel<H>, both networks) and
carl_brax_ppo_grad (its own actor kernel, ppo_net_kernel<H> for the critic) -- that test_gpu_ppo_grad.py and
test_gpu_brax_ppo_grad.py leave open.  The cases are ppo_ref.py's and brax_ppo_ref.py's; the checks shared with the CPU
tests of the same helpers (test_ppo_reference.py, test_brax_ppo_reference.py) are ppo_checks.py's.

A. The second pass of the persistent tile loop.  M = 256 x 256 + 3 x 256 + 7 samples: workgroups 0 .. 2 run a full second
   tile, workgroup 3 one of 7 samples.  Samples with advantage 0 and the device's own value as their return add exact zeros
   to every sum (ent_coef = 0, no advantage normalisation), so one tile's contribution stands alone inside the large
   launch and is compared with a one-tile launch of the same samples: ppo_checks.check_tile_identities.
B. Entries of idx outside the buffer or on a padding lane, against the float64 reference over the valid samples.  Every
   column is a view into a larger allocation whose padding lanes and surroundings hold NaN (out-of-range integers for
   context_id and discrete actions), and every bad index stays inside them: a kernel that read one would produce NaN.
C. The clip decision at r == 1 exactly (the old log-probabilities are the forward pass's own bits, as in the first
   minibatch after a collection), with clip_range 0 and 0.2, and with ratios of 1/2, 1 and 2 under clip_range 0.

Every launch runs twice on canaried outputs (ppo_checks.run_twice): a canary behind every output and the workspace, and
the same bits both times."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import brax_policy_cases as BPC
import brax_ppo_ref as BR
import ppo_checks as PK
import ppo_ref as R
import sampling_ref as SR
import value_cases as VC
from carl_amd import _lib
from carl_amd.engine import VecEngine
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


class Unit:
    """One case on the device: its columns uploaded once behind guard bands (part B's docstring), and run(), one
    canaried double launch of a minibatch `idx` with some columns or coefficients replaced."""

    def __init__(self, mod, spec):
        self.mod, self.case = mod, mod.make_case(spec)
        c = self.case
        self.brax = mod is BR
        self.actor, self.critic = c["actor"], c["critic"]
        self.N, self.P, self.T = c["N"], c["P"], c["T"]
        self.band = 2 * self.P
        self.discrete = not self.brax and self.actor.discrete
        self.cid = self.column(c["context_id"], mod.N_CONTEXTS)
        self.obs = self.column(c["obs"], NAN)
        self.action = self.column(c["action"], self.actor.n_out if self.discrete else NAN)
        self.obs0 = PK.guarded(c["obs0"], self.band * c["obs0"].shape[1], NAN, DEV)
        self.memo = {}
        if self.brax:
            self.lib = _lib.load()
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
            self.params = [up(self.actor.params), up(self.critic.params), up(self.actor.log_std), up(c["table"])]
            self.pol = self.actor.struct(self.N, self.params[0].data_ptr())
            self.crit = self.critic.struct(self.N, self.params[1].data_ptr())
            self.sys_t = BR.fake_sys(c["shape"])
        else:
            self.eng = VecEngine(c["family"], c["table"].T.astype(np.float64), self.N, DEV)

    def column(self, a, fill):
        """a [T, P, ...] column: its padding lanes and 2 * P rows' worth of elements on both sides hold `fill`"""
        a = a.copy()
        a[:, self.N:] = fill
        return PK.guarded(a, self.band * int(np.prod(a.shape[2:], dtype=np.int64)), fill, DEV)[:, : self.N]

    def weight_floats(self):
        return {"grad_actor": self.actor.weight_floats, "grad_critic": self.critic.weight_floats,
                "grad_log_std": self.actor.n_out if self.brax else 1}

    def run(self, idx, columns=None, clip_range=R.CLIP, ent_coef=R.ENT, adv_norm="case"):
        c = self.case
        col = {**c, **(columns or {})}
        f32 = {k: self.column(np.asarray(col[k], np.float32), NAN) for k in ("log_prob", "advantage", "ret")}
        norm = c["adv_norm"] if isinstance(adv_norm, str) else adv_norm
        norm_t = None if norm is None else torch.as_tensor(np.asarray(norm, np.float32)).to(DEV)
        idx_t = torch.as_tensor(np.asarray(idx, np.int32)).to(DEV)
        M = int(idx_t.numel())
        sizes = {"grad_actor": self.actor.set_floats, "grad_critic": self.critic.set_floats,
                 "grad_log_std": self.weight_floats()["grad_log_std"], "stats": 6, "new_log_prob": M, "new_value": M}
        if self.discrete:
            del sizes["grad_log_std"]
        if self.brax:
            ptr = {"obs0": self.obs0, "obs": self.obs, "context_id": self.cid, "ctx_table": self.params[3],
                   "action": self.action, "log_prob": f32["log_prob"], "advantage": f32["advantage"], "ret": f32["ret"],
                   "idx": idx_t, "adv_norm": norm_t}
            pb = BR.ppo_batch(c, {k: (None if v is None else v.data_ptr()) for k, v in ptr.items()})
            pb.n_samples, pb.clip_range, pb.ent_coef = M, clip_range, ent_coef
            need = int(self.lib.carl_brax_ppo_workspace_floats(C.byref(self.pol), C.byref(self.crit), M))
            assert need > 0

            def launch(out, ws):
                po = _lib.PpoOut(*(out[k].data_ptr() for k in ("grad_actor", "grad_critic", "grad_log_std", "stats",
                                                                "new_log_prob", "new_value")), ws.data_ptr(), need)
                _lib.check(self.lib.carl_brax_ppo_grad(C.byref(pb), C.byref(self.sys_t), C.byref(self.pol), C.byref(self.crit),
                                                       self.params[2].data_ptr(), C.byref(po),
                                                       torch.cuda.current_stream().cuda_stream))
        else:
            buf = {"action": self.action, "obs": self.obs, "log_prob": f32["log_prob"], "advantage": f32["advantage"],
                   "return": f32["ret"]}
            need = self.eng.ppo_workspace(self.actor, self.critic, M).numel()

            def launch(out, ws):
                self.eng.ppo_grad(self.actor, self.critic, buf, self.obs0, self.cid, idx=idx_t, adv_norm=norm_t,
                                  clip_range=clip_range, vf_coef=R.VF, ent_coef=ent_coef, forward=True, out=out, workspace=ws)

        return PK.check_canaries_and_bits(PK.run_twice(sizes, need, launch, DEV))

    def check_forward(self, pos, got, ref):
        """new_value / new_log_prob at the positions `pos` of the minibatch, at the closed-loop tests' tolerances, as
        test_gpu_ppo_grad.py and test_gpu_brax_ppo_grad.py check them; ref: the float64 reference over those positions"""
        c, actor = self.case, self.actor
        x, f = c["x"][pos], c["flat"][pos]
        VC.check_values(self.critic, x, got["new_value"][pos])
        if self.brax:
            _, y64, ybound = BPC.reference_actions(actor, x)
            lp64, bound = PK.gaussian_log_prob_reference(y64, ybound, actor.log_std, c["action"].reshape(-1, actor.n_out)[f])
        else:
            fwd = O.policy_forward(actor.params, actor.n_in, actor.widths, actor.n_out, actor.activation, x)
            a = c["action"].reshape(-1)[f]
            if actor.discrete:
                lp64 = SR.categorical_log_prob64(fwd.y64, a)
                bound = SR.categorical_log_prob_bound(fwd.y64, fwd.bound, a)
            else:
                lp64, bound = PK.gaussian_log_prob_reference(fwd.y64[:, :1], fwd.bound[:, :1], actor.log_std[:1], a)
        PK.check_log_prob(got["new_log_prob"][pos], lp64, bound, ref["new_log_prob"])


CASES = {spec[0]: (mod, spec) for mod in (R, BR)
         for spec in mod.tile_loop_cases() + mod.skipped_cases() + mod.clip_edge_cases()}


@functools.lru_cache(maxsize=2)
def unit(name):
    return Unit(*CASES[name])


def ids(*lists):
    return [spec[0] for cases in lists for spec in cases]


def test_the_tile_and_the_workgroup_cap_are_the_cases():
    lib = _lib.load()
    assert lib.carl_ppo_tile() == R.TILE == lib.carl_brax_ppo_tile()
    assert lib.carl_ppo_grad_workgroups(R.M_TILES) == R.WORKGROUPS_CAP == lib.carl_brax_ppo_grad_workgroups(R.M_TILES)


# ---------------------------------------------------------------- A: the second pass of the tile loop
@pytest.mark.parametrize("w", R.TILE_LOOP_WORKGROUPS)
@pytest.mark.parametrize("name", ids(R.tile_loop_cases(), BR.tile_loop_cases()))
def test_the_second_pass_of_the_tile_loop(name, w):
    """Workgroup w's first tile A and second tile B (w = 3: 7 samples), each isolated inside the launch of all M samples
    by zero-signal samples everywhere else, against one-tile launches of the same samples:
      small_A, small_B within K * 2^-24 * S of the float64 reference (the chain's tie to the reference);
      M big_A against |A| small_A within 3 * 2^-24 |A| |small_A| (likewise B);
      M big_AB against |A| small_A + |B| small_B within 4 * 2^-24 (|A| |small_A| + |B| |small_B|).
    The slab entry of workgroup w is the fp32 accumulator a (big_A, small_A), b (big_B, small_B) or rn32(a + b) (big_AB);
    every other workgroup's is +-0; the reduction multiplies the float64 slab sum by 1 / n_samples and rounds once.  So
    big_A = rn32(a / M) and small_A = rn32(a / |A|): two fp32 roundings of one number, 2 * 2^-24, and 3 with the float64
    terms.  For big_AB the rounding rn32(a + b), the final rounding and the two small runs' roundings each cost 2^-24 of
    at most |a| + |b|: 3 units where the roundings align, 4 with room for the float64 terms.  Entries below 2^-126 get one
    subnormal step; at least half of each gradient's weight entries are non-zero in both small runs
    (ppo_checks.check_tile_identities).  A second pass that dropped or doubled its tile sum, or that met stale rows in the
    tile buffers, moves big_B and big_AB by whole contributions."""
    u = unit(name)
    case, mod = u.case, u.mod
    M = case["flat"].size
    assert M == R.M_TILES

    def device(pos, columns):
        key = "forward" if pos is None and columns is None else None
        if key in u.memo:
            return u.memo[key]
        got = u.run(case["flat"] if pos is None else case["flat"][pos], columns, ent_coef=0.0, adv_norm=None)
        if key:
            u.memo[key] = got
        return got

    runs, A, B = R.tile_loop_runs(case, w, device)
    for label, pos in (("small_A", A), ("small_B", B)):
        ref = mod.case_reference(case, pos=pos, adv_norm=None, ent_coef=0.0)
        k = PK.grad_units(runs[label], ref)
        print(f"{name}, workgroup {w}: {label} ({pos.size} samples) largest gradient error {k:.2f} x 2^-24 S (K = {mod.K:.0f})")
        assert k <= mod.K
        u.check_forward(pos, {n: _at(device(None, None)[n], pos) for n in ("new_value", "new_log_prob")}, ref)
    worst = PK.check_tile_identities(runs, A.size, B.size, M, u.weight_floats())
    print(f"{name}, workgroup {w}: largest identity error / bound {worst:.3f}")


def _at(full, pos):
    """a [M] output with the positions `pos` kept in place (check_forward indexes by position)"""
    out = np.full_like(full, np.nan)
    out[pos] = full[pos]
    return out


# ---------------------------------------------------------------- B: skipped entries
@pytest.mark.parametrize("name", ids(R.skipped_cases(), BR.skipped_cases()))
def test_skipped_entries_contribute_zero_and_are_counted(name):
    """-1, n_steps * pitch, n_steps * pitch + 1 and (rows with padding lanes) t * pitch + n_lanes and t * pitch + pitch - 1
    at the first position of a tile, the last position of the partial tile and all through one wavefront
    (ppo_ref.with_bad_entries).  The float64 reference runs over the valid samples alone; a skipped sample adds zero to
    every sum while the divisor stays M, so its gradients, their S and the five means are rescaled by n_valid / M
    (ppo_ref.rescaled).  Gradients within K * 2^-24 * S; stats[5] == M and the other statistics within check_statistics;
    everything finite; new_log_prob / new_value right at the valid positions and unwritten at the skipped ones."""
    u = unit(name)
    case, mod = u.case, u.mod
    idx, valid = R.with_bad_entries(case["flat"], u.T, u.P, u.N)
    assert idx.min() >= -u.band and idx.max() < u.T * u.P + u.band  # (inside the guard bands)
    M, pos = idx.size, np.flatnonzero(valid)
    got = u.run(idx)
    ref = R.rescaled(mod.case_reference(case, pos=pos), pos.size, M)
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    for k in ("new_log_prob", "new_value"):
        assert (got[k][~valid] == PK.CANARY).all(), k
    u.check_forward(pos, got, ref)
    PK.check_transform_entries(got, u.actor, u.critic)
    worst = PK.grad_units(got, ref)
    print(f"{name}: {pos.size} of {M} entries valid, largest gradient error {worst:.2f} x 2^-24 S (K = {mod.K:.0f})")
    assert worst <= mod.K
    assert got["stats"][5] == M
    PK.check_statistics(got["stats"], ref["stats"], M)


# ---------------------------------------------------------------- C: the clip edge
@pytest.mark.parametrize("mixed", [False, True], ids=["r=1", "r=1/2,1,2"])
@pytest.mark.parametrize("name", ids(R.clip_edge_cases(), BR.clip_edge_cases()))
def test_the_clip_decision_at_the_edge(name, mixed):
    """The old log-probabilities are the device's own new_log_prob of a first call, so lr == 0 and r == 1 exactly.
    r = 1: with clip_range 0 (c_lo == c_hi == 1) and with 0.2 nothing is clipped and the gradient flows: approx_kl and the
    clip fraction are exactly 0, the two calls' gradients are the same bits, they are the float64 reference's with
    ratio 1 within K * 2^-24 * S, stats[0] is -mean(A') and grad_actor's weight entries are not zeros -- `r >= c_hi` in
    place of `r > c_hi` would zero every actor gradient with A' > 0.
    r = 1/2, 1, 2 (position m % 3; clip_range 0): log_prob = fl32(lp -+ ln 2).  The moved ratios are powers of two within
    a few roundings only (lp -+ ln 2 is not representable in general), and nothing below needs them exact: the reference
    takes the exact difference lp - log_prob, which the device's lr is within half an ulp of, and a ratio near 2 or 1/2 is
    on the same side of 1 either way.  The clip fraction is exactly the share of moved samples, and the gradients hold the
    reference's clipped set (A' > 0 && r > 1) || (A' < 0 && r < 1) at the K bound."""
    u = unit(name)
    case, mod = u.case, u.mod
    flat = case["flat"]
    M = flat.size
    if "first" not in u.memo:
        u.memo["first"] = u.run(flat)
    lp_dev = u.memo["first"]["new_log_prob"]
    lp64 = mod.case_reference(case)["new_log_prob"]
    dev_col, ref_col = R.clip_edge_columns(case, lp_dev, lp64, mixed)
    adv = raw = case["advantage"].reshape(-1)[flat]
    A64 = raw.astype(np.float64)
    if case["adv_norm"] is not None:
        adv = (raw - case["adv_norm"][0]) * case["adv_norm"][1]  # (float32, as the device forms A')
        A64 = (A64 - np.float64(case["adv_norm"][0])) * np.float64(case["adv_norm"][1])
    assert adv.dtype == np.float32 and (adv != 0).all() and (adv > 0).any() and (adv < 0).any()
    assert ((adv > 0) == (A64 > 0)).all()
    results = {}
    for clip in ((0.0,) if mixed else (0.0, 0.2)):
        got = results[clip] = u.run(flat, {"log_prob": dev_col}, clip_range=clip)
        ref = mod.case_reference(case, columns={"log_prob": ref_col}, clip_range=clip)
        moved = int((np.arange(M) % 3 != 0).sum()) if mixed else 0
        assert np.count_nonzero(ref["ratio"] != 1) == moved
        if mixed:
            clipped = ((A64 > 0) & (ref["ratio"] > 1)) | ((A64 < 0) & (ref["ratio"] < 1))
            assert 0 < clipped.sum() < moved and (~clipped & (ref["ratio"] > 1)).any() and (~clipped & (ref["ratio"] < 1)).any()
            assert got["stats"][4] == np.float32(moved * (1.0 / M))
        else:
            assert got["stats"][3] == 0.0 and got["stats"][4] == 0.0
            assert ref["stats"][0] == pytest.approx(-A64.mean(), rel=1e-12)
        PK.check_statistics(got["stats"], ref["stats"], M)
        worst = PK.grad_units(got, ref)
        print(f"{name}, clip_range {clip}, {moved} ratios moved: largest gradient error {worst:.2f} x 2^-24 S (K = {mod.K:.0f})")
        assert worst <= mod.K
        nz = np.count_nonzero(got["grad_actor"][: u.actor.weight_floats])
        assert 2 * nz >= u.actor.weight_floats
        u.check_forward(np.arange(M), got, ref)
    if not mixed:
        for k in PK.GRADS:
            if k in results[0.0]:
                np.testing.assert_array_equal(results[0.0][k].view(np.uint32), results[0.2][k].view(np.uint32), err_msg=k)
