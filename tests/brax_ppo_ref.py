"""Host reference of the PPO update of the Brax families (include/carl_amd.h: carl_brax_policy_context_trace,
carl_brax_ppo_grad), shared by test_brax_ppo_reference.py, test_brax_ppo_abi.py, test_gpu_brax_context_trace.py,
test_gpu_brax_ppo_grad.py and test_gpu_brax_ppo.py.  Built on ppo_ref.py: the selector walk, the sample inputs, the
forward pass and the backward pass through the layers are its functions, imported; what is added is the joint Gaussian
over up to 8 actuators with one log_std each (loss, dL/dy, grad_log_std [n_act]), the first-state rule of the walk and
the case table.  float64 from the float32 inputs (the reference) or float32 throughout (``dtype=np.float32``: the plain
restatement K0 is measured with).  A plain module: importing it touches no device.

Gradient tolerance of the device tests, as ppo_ref.py defines it: |g_dev - g_64| <= K * 2^-24 * S per packed entry, S
the mean of the absolute per-sample terms.  K0 is the largest |g_32 - g_64| / (2^-24 S) of the float32 restatement over
``grad_cases()``, measured on the CPU by
    PYTHONPATH=.:tests python tests/brax_ppo_ref.py
and K = 8 * K0 (the project's margin for the device tanh's allowed 6 * 2^-24 and a summation order other than NumPy's).
The comment above K0 below holds the printed figure and the cases that set it.

Device figures (MI355X, test_gpu_brax_ppo_grad.py, largest gradient error per case in units of 2^-24 S): see the table in
DESIGN 4.6l.
"""
import numpy as np

import ppo_ref as R
from carl_amd import _lib
from carl_amd.brax_engine import _BraxInfo
from carl_amd.brax_policy import BraxMLPPolicy

U = R.U
LN_2PI_HALF = R.LN_2PI_HALF
TILE, WORKGROUPS_CAP = R.TILE, R.WORKGROUPS_CAP  # carl_brax_ppo_tile(), the cap of carl_brax_ppo_grad_workgroups
N_CONTEXTS, N_FEATURES = 7, 6
CLIP, VF, ENT = R.CLIP, R.VF, R.ENT

# printed by measure_k0() (see the module docstring):
#   k0 = 1050.44 (hopper-2x(64,64)-13: 2 x (64, 64) ReLU, M = 255); the next: 570.17 for ant-2x(64,64)-18 (2 x (64, 64)
#   tanh, 32 inputs, 8 actuators, M = 1: one sample, so S has no other sample to average the cancelling backward sums
#   over), 52.55 for ant-2x(64,64)-second-tile (tanh, M = 65 537), 28.32 for hopper-1x32-12 (tanh, M = 1); every other
#   case is below 23.  As in ppo_ref.py the wide two-layer networks set K0: a first-layer delta is a sum over 64
#   second-layer deltas that cancels, and S sees the delta's own magnitude only.
K0 = 1050.44
K = 8 * K0


# ---------------------------------------------------------------- the trace walk
def context_walk(ctx_idx0, episode0, terminated, truncated, selector, stride, n_contexts, seed, lane_offset, autoreset,
                 first_state=False):
    """carl_brax_policy_context_trace's rule -> context_id [T, N] int32: ppo_ref.context_walk with genv = lane_offset + env,
    and under the first-state auto-reset (CARL_FLAG_AUTORESET_FIRST_STATE with a first_state buffer) a done env keeps its
    context and its episode counter: the context never moves"""
    return R.context_walk(ctx_idx0, episode0, terminated, truncated, selector, stride, n_contexts, seed, lane_offset,
                          autoreset and not first_state)


# ---------------------------------------------------------------- loss and gradients
def brax_ppo_grad_ref(actor, critic, x_raw, action, logp_old, adv, ret, adv_norm=None, clip_range=0.2, vf_coef=0.5,
                      ent_coef=0.0, dtype=np.float64, tile_order=False):
    """carl_brax_ppo_grad's outputs for the samples with raw inputs x_raw [M, n_in] (float32), actions [M, n_act] and
    their log_prob / advantage / return entries [M] (float32); every operation in `dtype`.  -> ppo_ref.ppo_grad_ref's
    dict, with grad_log_std / S_log_std [n_act]; tile_order: as ppo_ref.ppo_grad_ref takes it"""
    f = dtype
    M = x_raw.shape[0]
    lim = f(actor.clip)
    x = np.clip((x_raw.astype(f) - actor.shift.astype(f)) * actor.scale.astype(f), -lim, lim)
    y, hs_a, pre_a = R._network(actor, x, f, tile_order)
    v, hs_c, pre_c = R._network(critic, x, f, tile_order)
    V = v[:, 0]
    A = adv.astype(f)
    if adv_norm is not None:
        A = (A - f(adv_norm[0])) * f(adv_norm[1])
    c = f(np.float32(clip_range))
    ls = np.asarray(actor.log_std, np.float32).reshape(-1).astype(f)  # [n_act]
    inv = np.exp(-ls)
    z = (np.asarray(action).reshape(M, -1).astype(f) - y) * inv
    lpj = -z * z / 2 - ls - f(LN_2PI_HALF)
    lp = lpj[:, 0].copy()
    for j in range(1, lpj.shape[1]):  # in actuator order, as the sampled launch sums it
        lp = lp + lpj[:, j]
    Hj = f(0.5) + f(LN_2PI_HALF) + ls
    Hs = Hj[0]
    for j in range(1, Hj.size):
        Hs = Hs + Hj[j]
    H = np.full(M, Hs, f)
    lr = lp - logp_old.astype(f)
    r = np.exp(lr)
    surr = np.minimum(r * A, np.clip(r, 1 - c, 1 + c) * A)
    clipped = ((A > 0) & (r > 1 + c)) | ((A < 0) & (r < 1 - c))
    g_lp = np.where(clipped, f(0), -A * r)
    ec, vc = f(np.float32(ent_coef)), f(np.float32(vf_coef))
    dy = g_lp[:, None] * (z * inv)
    c_ls = g_lp[:, None] * (z * z - 1) - ec
    g_ls = R._tile_order_mean(c_ls, np.ones((M, 1), f))[:, 0] if tile_order else c_ls.sum(axis=0) / f(M)
    S_ls = np.abs(c_ls).astype(np.float64).sum(axis=0) / M
    dv = (vc * 2 * (V - ret.astype(f)))[:, None]
    g_a, S_a = R._backward(actor, dy, hs_a, pre_a, M, f, tile_order)
    g_c, S_c = R._backward(critic, dv, hs_c, pre_c, M, f, tile_order)
    pl, vl, ent = -surr.mean(), ((ret.astype(f) - V) ** 2).mean(), H.mean()
    stats = np.array([pl, vl, ent, ((r - 1) - lr).mean(), (np.abs(r - 1) > c).mean(), M], np.float64)
    return dict(new_log_prob=lp, new_value=V, entropy=H, ratio=r, y=y, z=z, pre_actor=pre_a, pre_critic=pre_c,
                grad_actor=g_a, grad_critic=g_c, grad_log_std=g_ls, S_actor=S_a, S_critic=S_c, S_log_std=S_ls, stats=stats,
                loss=pl - ec * ent + vc * vl)


# ---------------------------------------------------------------- the cases of test_gpu_brax_ppo_grad.py (made on the CPU)
# model-like shapes: name -> (obs_dim, n_act, context inputs when the case has any).  n_in = 4 (pendulum without context
# inputs), 13 (reacher / hopper with two), 32 (Ant's 27 observations with five), and 6 / 11 / 27 beside them
SHAPES = {"pendulum": (4, 1, 2), "reacher": (11, 2, 2), "hopper": (11, 3, 2), "ant": (27, 8, 5)}
NETWORKS = {"linear": (), "1x7": (7,), "1x32": (32,), "2x(64,64)": (64, 64), "2x(7,3)": (7, 3)}


def info_of(shape_name):
    D, n_act, _ = SHAPES[shape_name]
    return _BraxInfo(20, D, N_FEATURES, n_act, 0, 0, 1000, -1.0, 1.0)


def fake_sys(shape_name):
    """a carl_brax_sys_t that says what carl_brax_ppo_grad reads of one: obs_dim and n_act"""
    s = _lib.BraxSys()
    s.obs_dim, s.n_act = SHAPES[shape_name][0], SHAPES[shape_name][1]
    return s


def grad_cases():
    """(id, shape name, n_ctx, network name, activation, n_lanes, M or None (idx NULL: every sample), adv_norm?) -- every
    shape x network; the context inputs, the activation and the sample count rotate through them so that each value of
    each meets several shapes and networks; once an M just past WORKGROUPS_CAP x TILE (some workgroup runs a second tile)"""
    Ms = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, None]
    acts = ["tanh", "relu", "identity"]
    out, k = [], 0
    for shp in SHAPES:
        for net in NETWORKS:
            n_ctx = SHAPES[shp][2] if (k + k // 5) % 2 else 0
            out.append((f"{shp}-{net}-{k}", shp, n_ctx, net, acts[k % 3], 272, Ms[k % 6], k % 4 < 2))
            k += 1
    out.append(("ant-2x(64,64)-second-tile", "ant", 5, "2x(64,64)", "tanh", 272, WORKGROUPS_CAP * TILE + 1, True))
    return out


def make_case(case):
    """A synthetic dense rollout buffer and minibatch for one grad_cases() entry, NumPy only, made as ppo_ref.make_case
    makes its: random observations in the policies' normalised range, context ids, actions around the actor's mean,
    advantages and returns; a distinct log_std per actuator, some negative; old log-probabilities chosen so that every
    float64 ratio lies in [0.55, 1.45] and at least 0.01 from 1 +- CLIP; for ReLU, samples with a pre-activation below 1e-4
    in magnitude get new observations until none is left."""
    cid, shp, n_ctx, net, act, N, M, use_norm = case
    D, n_act, _ = SHAPES[shp]
    rng = np.random.default_rng(sum(map(ord, cid)))
    info = info_of(shp)
    widths = NETWORKS[net]
    rows = list(range(N_FEATURES))[:n_ctx]
    table = rng.uniform(0.5, 2.0, (N_FEATURES, N_CONTEXTS)).astype(np.float32)  # [F, C]
    o_shift, o_scale = rng.normal(0, 0.3, D), rng.uniform(0.5, 2.0, D)
    shift = np.concatenate([np.full(n_ctx, 1.25), o_shift])
    scale = np.concatenate([np.full(n_ctx, 2.0), o_scale])
    n_in = n_ctx + D

    def layers(dims):
        return [(rng.normal(0, 1.0 / np.sqrt(i), (o, i)), rng.normal(0, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]

    log_std = (-0.5 + 0.2 * np.arange(n_act) + rng.normal(0, 0.05, n_act)).astype(np.float32)  # -0.5 .. 0.9: both signs
    actor = BraxMLPPolicy(info, rows, layers([n_in, *widths, n_act]), act, shift, scale, 5.0, log_std=log_std)
    critic = BraxMLPPolicy(info, rows, layers([n_in, *widths, 1]), act, shift, scale, 5.0, head="value")
    every = M is None
    T = 3 if every else max(2, -(-M // N) + 1)
    f32 = np.float32

    def draw_obs(shape):
        return (o_shift + rng.normal(0, 1, shape + (D,)) / o_scale).astype(f32)

    obs0, obs = draw_obs((N,)), draw_obs((T, N))
    context_id = rng.integers(0, N_CONTEXTS, (T, N)).astype(np.int32)
    flat = np.arange(T * N) if every else rng.permutation(T * N)[:M]
    Mn = flat.size
    zero = np.zeros(Mn, f32)
    if act == "relu":
        for _ in range(50):
            x = R.sample_inputs(actor, table, context_id, obs0, obs, flat, N)
            ref = brax_ppo_grad_ref(actor, critic, x, np.zeros((Mn, n_act), f32), zero, zero, zero)
            bad = np.zeros(Mn, bool)
            for v in ref["pre_actor"] + ref["pre_critic"]:
                bad |= (np.abs(v) < 1e-4).any(axis=1)
            if not bad.any():
                break
            t, lane = flat[bad] // N, flat[bad] % N
            new = draw_obs((int(bad.sum()),))
            obs0[lane[t == 0]] = new[t == 0]
            obs[t[t > 0] - 1, lane[t > 0]] = new[t > 0]
    x = R.sample_inputs(actor, table, context_id, obs0, obs, flat, N)
    mu = brax_ppo_grad_ref(actor, critic, x, np.zeros((Mn, n_act), f32), zero, zero, zero)["y"]
    action = rng.normal(0, 1.5, (T, N, n_act)).astype(f32)
    # (the samples' actions around the mean, as sampled ones are: z of the order of 1 on every actuator)
    action.reshape(-1, n_act)[flat] = (mu + np.exp(log_std) * rng.normal(0, 1, (Mn, n_act))).astype(f32)
    adv = rng.normal(0.3, 1.0, (T, N)).astype(f32)
    ret = rng.normal(0, 2.0, (T, N)).astype(f32)
    a_s = action.reshape(-1, n_act)[flat]
    adv_s, ret_s = adv.reshape(-1)[flat], ret.reshape(-1)[flat]
    norm = np.array([adv_s.mean(), 1.0 / (adv_s.std() + 1e-8)], f32) if use_norm and Mn > 1 else None
    lp = brax_ppo_grad_ref(actor, critic, x, a_s, zero, adv_s, ret_s, norm, CLIP, VF, ENT)["new_log_prob"]
    target = rng.uniform(0.55, 1.45, Mn)
    for edge in (1 - CLIP, 1 + CLIP):
        near = np.abs(target - edge) < 0.01
        target[near] = edge + np.where(target[near] >= edge, 0.01, -0.01)
    logp = np.zeros((T, N), f32)
    logp.reshape(-1)[flat] = (lp - np.log(target)).astype(f32)
    return dict(id=cid, shape=shp, actor=actor, critic=critic, table=table, N=N, P=N, T=T, obs0=obs0, obs=obs,
                context_id=context_id, action=action, log_prob=logp, advantage=adv, ret=ret, flat=flat.astype(np.int32),
                every=every, adv_norm=norm, x=x)


def case_reference(case, dtype=np.float64, pos=None, columns=None, adv_norm="case", clip_range=CLIP, ent_coef=ENT,
                   tile_order=False):
    """brax_ppo_grad_ref of a case's minibatch; pos, columns, adv_norm: as ppo_ref.case_reference takes them"""
    f, x = (case["flat"], case["x"]) if pos is None else (case["flat"][pos], case["x"][pos])
    col = {**case, **(columns or {})}
    pick = lambda a: a.reshape(-1)[f]  # noqa: E731
    n_act = case["actor"].n_out
    return brax_ppo_grad_ref(case["actor"], case["critic"], x, case["action"].reshape(-1, n_act)[f], pick(col["log_prob"]),
                             pick(col["advantage"]), pick(col["ret"]),
                             case["adv_norm"] if isinstance(adv_norm, str) else adv_norm, clip_range, VF, ent_coef, dtype,
                             tile_order)


# ---------------------------------------------------------------- the cases of test_gpu_ppo_grad_edges.py
# (ppo_ref.py holds what the two units share: tile_positions, zero_signal, tile_loop_runs, with_bad_entries, rescaled,
# clip_edge_columns.)  Part A: H = 0, 32, 64 with 2 or 3 actuators; rows are dense, so the skipped entries of part B are
# the ones outside the buffer only.
def tile_loop_cases():
    return [("reacher-linear-tile-loop", "reacher", 2, "linear", "identity", 272, R.M_TILES, False),
            ("hopper-1x32-tile-loop", "hopper", 0, "1x32", "relu", 272, R.M_TILES, False),
            ("reacher-2x(64,64)-tile-loop", "reacher", 0, "2x(64,64)", "tanh", 272, R.M_TILES, False)]


def skipped_cases():
    return [("hopper-1x32-skipped", "hopper", 2, "1x32", "tanh", 260, 2 * TILE + 3, True)]


def clip_edge_cases():
    return [("reacher-1x7-clip-edge", "reacher", 2, "1x7", "tanh", 260, TILE + 1, True)]


assert_conditioned = R.assert_conditioned
grad_error_units = R.grad_error_units


def case_k(r, r64):
    """largest |g - g_64| / (2^-24 S) over the actor's, the critic's and log_std's entries"""
    k = 0.0
    for name in ("actor", "critic", "log_std"):
        k = max(k, grad_error_units(np.atleast_1d(r["grad_" + name]), np.atleast_1d(r64["grad_" + name]),
                                    np.atleast_1d(r64["S_" + name])).max(initial=0.0))
    return k


def measure_k0():
    worst = (0.0, None)
    for case in grad_cases():
        c = make_case(case)
        r64, r32 = case_reference(c), case_reference(c, np.float32)
        assert_conditioned(c, r64)
        k = case_k(r32, r64)
        print(f"{c['id']:40s} {c['actor'].activation:8s} M = {c['flat'].size:6d}  k = {k:.3f}")
        if k > worst[0]:
            worst = (k, c["id"])
    print(f"k0 = {worst[0]:.2f} ({worst[1]})")
    return worst[0]


# ---------------------------------------------------------------- carl_brax_ppo_grad through the C ABI
def ppo_batch(case, ptr):
    """carl_ppo_batch_t of a case; ptr: name -> device pointer (obs0, obs, context_id, ctx_table, action, log_prob,
    advantage, ret, idx, adv_norm)"""
    b = _lib.PpoBatch()
    b.family, b.n_lanes, b.n_steps, b.row_pitch, b.obs_dim = -1, case["N"], case["T"], 0, case["actor"].obs_dim
    b.n_contexts, b.ctx_stride, b.action_dtype, b.n_samples = N_CONTEXTS, N_CONTEXTS, _lib.ACTION_F32, case["flat"].size
    b.clip_range, b.vf_coef, b.ent_coef = CLIP, VF, ENT
    for k, v in ptr.items():
        setattr(b, k, v)
    return b


if __name__ == "__main__":
    measure_k0()
