"""Host reference of the PPO update on the device (include/carl_amd.h: carl_policy_context_trace, carl_ppo_grad), shared
by test_ppo_reference.py, test_gpu_context_trace.py, test_gpu_ppo_grad.py, test_gpu_ppo_grad_edges.py and test_gpu_ppo.py:
the selector walk, the sample inputs, and the forward pass, loss and analytic gradients of a minibatch in NumPy -- float64
from the float32 inputs (the reference), or float32 throughout (``dtype=np.float32``: the plain restatement k0 is measured
with; with ``tile_order=True`` its sums run in the device's stated order, which the zero-signal identities need).  A plain
module like policy_cases.py: importing it touches no device.

Gradient tolerance of the device tests.  Each packed gradient entry g = (1 / M) sum_s c_s must satisfy
    |g_dev - g_64| <= K * 2^-24 * S,    S = (1 / M) sum_s |c_s|
(S: ``ppo_grad_ref``'s ``S_*`` arrays: for a weight, c_s = delta_s[i] * h_s[j], so S = mean |delta_i| |h_j|).  K is not
tuned on the device: K0 is the largest |g_32 - g_64| / (2^-24 S) of the float32 restatement over the cases of
test_gpu_ppo_grad.py (``grad_cases()`` below), measured on the CPU by
    PYTHONPATH=. python tests/ppo_ref.py
which printed ``k0 = 985.62`` (cartpole, 2 x (64, 64) ReLU, M = 515; the next: 269 for pendulum's 2 x (64, 64) ReLU, at
most 19 for every other case), and K = 8 * K0: the margin covers the device tanh's allowed 6 * 2^-24 absolute error and a
summation order that differs from NumPy's.  Why the wide ReLU networks set K0: a first-layer delta is a sum over 64
second-layer deltas that cancels, so its float32 error is of the order of 2^-24 times the sum of the terms' magnitudes,
not of the delta's own magnitude, which is all that S sees; entries whose S is small then stand far out.
"""
import numpy as np

import policy_cases as PC
import sampling_ref as SR
from carl_amd import _lib
from carl_amd.policy import MLPPolicy

U = 2.0 ** -24
K0 = 985.62      # measured: see the module docstring
K = 8 * K0
LN_2PI_HALF = 0.5 * np.log(2 * np.pi)


# ---------------------------------------------------------------- the selector walk
def context_walk(ctx_idx0, episode0, terminated, truncated, selector, stride, n_contexts, seed, lane_offset, autoreset):
    """carl_policy_context_trace's rule -> context_id [T, N] int32 (the context step t's action was chosen in)"""
    T, N = terminated.shape
    c = np.asarray(ctx_idx0, np.int64).copy()
    e = np.asarray(episode0).astype(np.uint32).astype(np.uint64)
    lanes = np.arange(N, dtype=np.uint64)
    glane = (np.uint64(lane_offset % (1 << 64)) + lanes) & np.uint64(0xFFFFFFFFFFFFFFFF)
    out = np.empty((T, N), np.int32)
    for t in range(T):
        out[t] = c
        if not autoreset:
            continue
        done = (terminated[t] != 0) | (truncated[t] != 0)
        if selector == _lib.SEL_ROUND_ROBIN:
            nxt = (c + stride) % n_contexts
        elif selector == _lib.SEL_RANDOM:
            w = SR.philox(glane & np.uint64(0xFFFFFFFF), glane >> np.uint64(32), e & np.uint64(0xFFFFFFFF), 1,
                          seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
            nxt = ((w.astype(np.uint64) * np.uint64(n_contexts)) >> np.uint64(32)).astype(np.int64)
        else:
            nxt = c
        c = np.where(done, nxt, c)
        e = np.where(done, e + np.uint64(1), e)
    return out


# ---------------------------------------------------------------- a minibatch's inputs
def sample_inputs(actor, ctx_table_fc, context_id, obs0, obs, flat, pitch):
    """raw inputs x [M, n_in] float32 of the samples `flat` (t * pitch + lane): the context values of context_id[t][lane]
    at the actor's context rows, then obs0[lane] (t == 0) or obs[t - 1][lane]; arrays [T, pitch(, D)]"""
    t, lane = flat // pitch, flat % pitch
    cid = context_id.reshape(-1)[flat]
    ctx = ctx_table_fc[np.asarray(actor.ctx_rows, np.int64)][:, cid].T if actor.ctx_rows else np.zeros((flat.size, 0), np.float32)
    o = np.where((t == 0)[:, None], obs0[lane], obs[np.maximum(t - 1, 0), lane])
    return np.concatenate([ctx.astype(np.float32), o.astype(np.float32)], axis=1)


def _act(v, kind):
    return np.tanh(v) if kind == "tanh" else np.maximum(v, 0) if kind == "relu" else v


def _act_grad(v, h, kind):
    return 1 - h * h if kind == "tanh" else (v > 0).astype(h.dtype) if kind == "relu" else np.ones_like(h)


def _rows_matmul(h, Wt):
    """h @ Wt with every row's terms added in input order whatever the number of rows: a BLAS product may group a row's
    terms by the shape of the whole matrix, and then a sample's float32 forward pass depends on the minibatch it is in"""
    out = np.zeros((h.shape[0], Wt.shape[1]), h.dtype)
    for k in range(h.shape[1]):
        out += h[:, k: k + 1] * Wt[k]
    return out


def _network(pol, x, dtype, by_rows=False):
    """forward pass of normalised inputs x -> (head outputs, [layer inputs], [pre-activations]); by_rows: _rows_matmul"""
    hs, pre = [x], []
    h = x
    for k, (W, b) in enumerate(pol.layers):
        v = (_rows_matmul(h, W.astype(dtype).T) if by_rows else h @ W.astype(dtype).T) + b.astype(dtype)
        if k < len(pol.layers) - 1:
            pre.append(v)
            h = _act(v, pol.activation)
            hs.append(h)
    return v, hs, pre


def _tile_order_mean(d, h):
    """(1 / M) sum_s d[s, i] h[s, j] summed as include/carl_amd.h states it, in d's dtype: tiles of TILE samples in index
    order, blocks of 16 (each product rounded, added in sample order), the block sums added into the tile sum, tile t's sum
    into accumulator t % workgroups, the accumulators added in order in float64, times 1 / M, rounded once.  Unlike a BLAS
    product its grouping of the terms does not depend on the shapes, so a sample whose d row is +-0 changes no partial sum:
    what the zero-signal identities of test_gpu_ppo_grad_edges.py rest on (the device uses fma inside a block; the
    grouping is the same)."""
    f = d.dtype.type
    M = d.shape[0]
    n_t = -(-M // TILE)

    def tiles(a):
        return np.concatenate([a, np.zeros((n_t * TILE - M, a.shape[1]), f)]).reshape(n_t, TILE, a.shape[1])

    dp, hp = tiles(d), tiles(h)
    tile = np.zeros((n_t, d.shape[1], h.shape[1]), f)
    for b in range(0, TILE, 16):
        blk = np.zeros_like(tile)
        for s in range(b, b + 16):
            blk += dp[:, s, :, None] * hp[:, s, None, :]
        tile += blk
    n_wg = min(n_t, WORKGROUPS_CAP)
    acc = np.zeros((n_wg,) + tile.shape[1:], f)
    for t0 in range(0, n_t, n_wg):
        part = tile[t0: t0 + n_wg]
        acc[: len(part)] += part
    total = np.zeros(tile.shape[1:], np.float64)
    for g in range(n_wg):
        total += acc[g]
    return (total * (1.0 / M)).astype(f)


def _backward(pol, dy, hs, pre, M, dtype, tile_order=False):
    """packed gradient [set_floats] and its S of per-sample head gradients dy [M, n_out] (not yet divided by M);
    tile_order: the sums over the samples by _tile_order_mean and the deltas by _rows_matmul instead of matrix products"""
    grads, esses = [], []
    d = dy
    for k in range(len(pol.layers) - 1, -1, -1):
        W = pol.layers[k][0].astype(dtype)
        h = hs[k]
        if tile_order:
            grads.append((_tile_order_mean(d, h), _tile_order_mean(d, np.ones((M, 1), dtype))[:, 0]))
        else:
            grads.append((d.T @ h / dtype(M), d.sum(axis=0) / dtype(M)))
        esses.append((np.abs(d).T.astype(np.float64) @ np.abs(h).astype(np.float64) / M,
                      np.abs(d).astype(np.float64).sum(axis=0) / M))
        if k > 0:
            d = (_rows_matmul(d, W) if tile_order else d @ W) * _act_grad(pre[k - 1], hs[k], pol.activation)
    g = np.zeros(pol.set_floats, dtype)
    S = np.zeros(pol.set_floats, np.float64)
    off = 0
    for (gW, gb), (sW, sb) in zip(reversed(grads), reversed(esses)):
        g[off: off + gW.size], S[off: off + gW.size] = gW.reshape(-1), sW.reshape(-1)
        off += gW.size
        g[off: off + gb.size], S[off: off + gb.size] = gb, sb
        off += gb.size
    return g, S


def ppo_grad_ref(actor, critic, x_raw, action, logp_old, adv, ret, adv_norm=None, clip_range=0.2, vf_coef=0.5, ent_coef=0.0,
                 dtype=np.float64, tile_order=False):
    """carl_ppo_grad's outputs for the samples with raw inputs x_raw [M, n_in] (float32) and their action / log_prob /
    advantage / return entries [M] (float32), from the policies' own layer arrays; every operation in `dtype`.
    -> dict: new_log_prob, new_value, entropy, ratio [M]; pre_actor / pre_critic: the hidden pre-activations; grad_actor /
    grad_critic (packed) and grad_log_std with S_actor / S_critic / S_log_std; stats [6]; loss.  tile_order: the
    gradients' sums over the samples in the device's stated order (_tile_order_mean) and every sample's own
    arithmetic independent of the other samples (_rows_matmul)"""
    f = dtype
    M = x_raw.shape[0]
    lim = f(actor.clip)
    x = np.clip((x_raw.astype(f) - actor.shift.astype(f)) * actor.scale.astype(f), -lim, lim)
    y, hs_a, pre_a = _network(actor, x, f, tile_order)
    v, hs_c, pre_c = _network(critic, x, f, tile_order)
    V = v[:, 0]
    A = adv.astype(f)
    if adv_norm is not None:
        A = (A - f(adv_norm[0])) * f(adv_norm[1])
    c = f(np.float32(clip_range))
    ls = f(actor.log_std[0])
    if actor.discrete:
        a = np.asarray(action, np.int64)
        m = y.max(axis=1, keepdims=True)
        e = np.exp(y - m)
        s = e.sum(axis=1, keepdims=True)
        logp = (y - m) - np.log(s)
        p = e / s
        lp = logp[np.arange(M), a]
        H = -(p * logp).sum(axis=1)
    else:
        z = (action.astype(f) - y[:, 0]) * np.exp(-ls)
        lp = -z * z / 2 - ls - f(LN_2PI_HALF)
        H = np.full(M, f(0.5) + f(LN_2PI_HALF) + ls)
    lr = lp - logp_old.astype(f)
    r = np.exp(lr)
    surr = np.minimum(r * A, np.clip(r, 1 - c, 1 + c) * A)
    clipped = ((A > 0) & (r > 1 + c)) | ((A < 0) & (r < 1 - c))
    g_lp = np.where(clipped, f(0), -A * r)
    ec, vc = f(np.float32(ent_coef)), f(np.float32(vf_coef))
    if actor.discrete:
        onehot = np.zeros_like(y)
        onehot[np.arange(M), a] = 1
        dy = g_lp[:, None] * (onehot - p) + ec * p * (logp + H[:, None])
        g_ls, S_ls = f(0), 0.0
    else:
        dy = (g_lp * z * np.exp(-ls))[:, None]
        c_ls = g_lp * (z * z - 1) - ec
        g_ls = _tile_order_mean(c_ls[:, None], np.ones((M, 1), f))[0, 0] if tile_order else c_ls.sum() / f(M)
        S_ls = float(np.abs(c_ls).astype(np.float64).sum() / M)
    dv = (vc * 2 * (V - ret.astype(f)))[:, None]
    g_a, S_a = _backward(actor, dy, hs_a, pre_a, M, f, tile_order)
    g_c, S_c = _backward(critic, dv, hs_c, pre_c, M, f, tile_order)
    pl, vl, ent = -surr.mean(), ((ret.astype(f) - V) ** 2).mean(), H.mean()
    stats = np.array([pl, vl, ent, ((r - 1) - lr).mean(), (np.abs(r - 1) > c).mean(), M], np.float64)
    return dict(new_log_prob=lp, new_value=V, entropy=H, ratio=r, y=y, pre_actor=pre_a, pre_critic=pre_c, grad_actor=g_a,
                grad_critic=g_c, grad_log_std=g_ls, S_actor=S_a, S_critic=S_c, S_log_std=S_ls, stats=stats,
                loss=pl - ec * ent + vc * vl)


# ---------------------------------------------------------------- the cases of test_gpu_ppo_grad.py (made on the CPU)
FAMILIES = {"cartpole": _lib.CARTPOLE, "mountaincar": _lib.MOUNTAINCAR, "acrobot": _lib.ACROBOT, "pendulum": _lib.PENDULUM}
NETWORKS = {"linear": (), "1x1": (1,), "1x5": (5,), "2x(7,3)": (7, 3), "2x(64,64)": (64, 64)}
TILE, WORKGROUPS_CAP = 256, 256  # carl_ppo_tile(), the cap of carl_ppo_grad_workgroups (asserted in test_ppo_abi.py)
N_CONTEXTS = 7
CLIP, VF, ENT = 0.2, 0.5, 0.01


def grad_cases():
    """(id, family name, n_ctx, network name, activation, n_lanes, M or None (idx NULL: every sample), adv_norm?) --
    every family x network; n_ctx, the activation, the lane count (272: dense rows; 260: rows of carl_rollout_pitch = 272)
    and the sample count rotate through them, so that each value of each meets several families and networks; the M just
    past WORKGROUPS_CAP x TILE (some workgroup runs a second tile) once per head kind"""
    Ms = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, None]
    acts = ["tanh", "relu", "identity"]
    out, k = [], 0
    for fam in FAMILIES:
        for net in NETWORKS:
            M, n = Ms[k % 6], (272, 260)[(k // 2) % 2]
            out.append((f"{fam}-{net}-{k}", fam, (0, 2)[k % 2], net, acts[k % 3], n, M, k % 4 < 2))
            k += 1
    out.append(("cartpole-2x(64,64)-second-tile", "cartpole", 2, "2x(64,64)", "tanh", 272, WORKGROUPS_CAP * TILE + 1, True))
    out.append(("pendulum-1x5-second-tile", "pendulum", 0, "1x5", "relu", 260, WORKGROUPS_CAP * TILE + 1, False))
    return out


def make_case(case):
    """A synthetic rollout buffer and minibatch for one grad_cases() entry, NumPy only: random observations in the
    policies' normalised range, context ids, actions, advantages and returns; old log-probabilities chosen so that every
    float64 ratio lies in [0.55, 1.45] and at least 0.01 from 1 +- CLIP; for ReLU, samples with a pre-activation below 1e-4
    in magnitude get new observations until none is left."""
    cid, fam_name, n_ctx, net, act, N, M, use_norm = case
    fam = FAMILIES[fam_name]
    rng = np.random.default_rng(sum(map(ord, cid)))
    eng = PC.fake_engine(fam)
    eng.n = N
    widths = NETWORKS[net]
    rows = [0, eng.F - 1][:n_ctx]
    table = PC.context_table(fam, N_CONTEXTS, rng).astype(np.float32).T.copy()  # [F, C]
    d = PC.defaults(fam)[rows] if rows else np.zeros(0)
    o_shift, o_scale = PC.OBS_NORM[fam]
    shift = np.concatenate([d, o_shift])
    scale = np.concatenate([4.0 / np.maximum(np.abs(d), 1e-3), o_scale])
    n_in = n_ctx + eng.D
    n_out = PC.n_outputs(eng)

    def layers(dims):
        return [(rng.normal(0, 1.0 / np.sqrt(i), (o, i)), rng.normal(0, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]

    box = not eng.info.action_is_discrete
    actor = MLPPolicy.for_env(eng, layers([n_in, *widths, n_out]), act, input_shift=shift, input_scale=scale, input_clip=5.0,
                              context_features=rows, log_std=-0.3 if box else None)
    critic = MLPPolicy.for_env(eng, layers([n_in, *widths, 1]), act, input_shift=shift, input_scale=scale, input_clip=5.0,
                               context_features=rows, head="value")
    P = (N + 15) // 16 * 16
    every = M is None
    T = 3 if every else max(2, -(-M // N) + 1)
    f32 = np.float32

    def draw_obs(shape):
        return (np.asarray(o_shift) + rng.normal(0, 1, shape + (eng.D,)) / np.asarray(o_scale)).astype(f32)

    obs0, obs = draw_obs((N,)), draw_obs((T, P))
    context_id = rng.integers(0, N_CONTEXTS, (T, P)).astype(np.int32)
    if every:
        flat = (np.arange(T)[:, None] * P + np.arange(N)[None, :]).reshape(-1)
    else:
        valid = (np.arange(T)[:, None] * P + np.arange(N)[None, :]).reshape(-1)
        flat = rng.permutation(valid)[:M]
    Mn = flat.size
    if act == "relu":
        for _ in range(50):
            x = sample_inputs(actor, table, context_id, obs0, obs, flat, P)
            ref = ppo_grad_ref(actor, critic, x, np.zeros(Mn, np.int64 if not box else f32), np.zeros(Mn, f32),
                               np.zeros(Mn, f32), np.zeros(Mn, f32))
            pre = ref["pre_actor"] + ref["pre_critic"]
            bad = np.zeros(Mn, bool)
            for v in pre:
                bad |= (np.abs(v) < 1e-4).any(axis=1)
            if not bad.any():
                break
            t, lane = flat[bad] // P, flat[bad] % P
            new = draw_obs((int(bad.sum()),))
            obs0[lane[t == 0]] = new[t == 0]
            obs[t[t > 0] - 1, lane[t > 0]] = new[t > 0]
    x = sample_inputs(actor, table, context_id, obs0, obs, flat, P)
    if box:
        action = rng.normal(0, 1.5, (T, P)).astype(f32)
    else:
        action = rng.integers(0, n_out, (T, P)).astype(np.int32)
    adv = rng.normal(0.3, 1.0, (T, P)).astype(f32)
    ret = rng.normal(0, 2.0, (T, P)).astype(f32)
    a_s, adv_s, ret_s = (v.reshape(-1)[flat] for v in (action, adv, ret))
    norm = np.array([adv_s.mean(), 1.0 / (adv_s.std() + 1e-8)], f32) if use_norm and Mn > 1 else None
    lp = ppo_grad_ref(actor, critic, x, a_s, np.zeros(Mn, f32), adv_s, ret_s, norm, CLIP, VF, ENT)["new_log_prob"]
    # target ratios away from the clip boundaries
    target = rng.uniform(0.55, 1.45, Mn)
    for edge in (1 - CLIP, 1 + CLIP):
        near = np.abs(target - edge) < 0.01
        target[near] = edge + np.where(target[near] >= edge, 0.01, -0.01)
    logp = np.zeros((T, P), f32)
    logp.reshape(-1)[flat] = (lp - np.log(target)).astype(f32)
    return dict(id=cid, family=fam, actor=actor, critic=critic, table=table, N=N, P=P, T=T, obs0=obs0, obs=obs,
                context_id=context_id, action=action, log_prob=logp, advantage=adv, ret=ret, flat=flat.astype(np.int32),
                every=every, adv_norm=norm, x=x)


def case_reference(case, dtype=np.float64, pos=None, columns=None, adv_norm="case", clip_range=CLIP, ent_coef=ENT,
                   tile_order=False):
    """ppo_grad_ref of a case's minibatch; pos: positions into case["flat"] to evaluate instead of all of them (a minibatch
    of its own: M = len(pos)); columns: {"log_prob" / "advantage" / "ret": a [T, P] array of any float dtype} read instead
    of the case's; adv_norm: "case" for the case's own pair"""
    f, x = (case["flat"], case["x"]) if pos is None else (case["flat"][pos], case["x"][pos])
    col = {**case, **(columns or {})}
    pick = lambda a: a.reshape(-1)[f]  # noqa: E731
    return ppo_grad_ref(case["actor"], case["critic"], x, pick(case["action"]), pick(col["log_prob"]),
                        pick(col["advantage"]), pick(col["ret"]), case["adv_norm"] if isinstance(adv_norm, str) else adv_norm,
                        clip_range, VF, ent_coef, dtype, tile_order)


# ---------------------------------------------------------------- the cases of test_gpu_ppo_grad_edges.py
# Part A: M = 256 tiles + 3 full tiles + 7 samples, so workgroups 0 .. 2 run a full second tile and workgroup 3 one of 7
# samples; 272 lanes x 245 steps hold them.  H = 0, 32 (one and two hidden layers) and 64; a 2-action, two 3-action and the
# Box family; context inputs on two.
M_TILES = WORKGROUPS_CAP * TILE + 3 * TILE + 7
TILE_LOOP_WORKGROUPS = (0, 3)


def tile_loop_cases():
    return [("cartpole-linear-tile-loop", "cartpole", 2, "linear", "identity", 272, M_TILES, False),
            ("acrobot-1x5-tile-loop", "acrobot", 0, "1x5", "relu", 272, M_TILES, False),
            ("mountaincar-2x(7,3)-tile-loop", "mountaincar", 0, "2x(7,3)", "tanh", 272, M_TILES, False),
            ("pendulum-2x(64,64)-tile-loop", "pendulum", 2, "2x(64,64)", "tanh", 272, M_TILES, False)]


def tile_positions(M, w):
    """(A, B): the positions (into idx) of tile w and of tile w + WORKGROUPS_CAP, workgroup w's first and second pass"""
    A = np.arange(w * TILE, min((w + 1) * TILE, M))
    B = np.arange((w + WORKGROUPS_CAP) * TILE, min((w + WORKGROUPS_CAP + 1) * TILE, M))
    assert A.size and B.size
    return A, B


def zero_signal(case, keep, new_value):
    """{"advantage", "ret"}: copies of the case's columns in which every sample of the minibatch outside the positions
    `keep` has advantage 0 and return new_value[position] (new_value [M]: the forward pass's own values, so V - ret == 0
    in its arithmetic; the return column takes new_value's dtype).  With ent_coef = 0 and no advantage normalisation such
    a sample's dL/dy and grad_log_std term are +-0 whatever its inputs, action and old log-probability are."""
    off = np.ones(case["flat"].size, bool)
    off[keep] = False
    adv, ret = case["advantage"].copy(), case["ret"].astype(new_value.dtype)
    adv.reshape(-1)[case["flat"][off]] = 0
    ret.reshape(-1)[case["flat"][off]] = new_value[off]
    return {"advantage": adv, "ret": ret}


def tile_loop_runs(case, w, reference):
    """Part A's five runs of workgroup w from reference(pos, columns) -> ppo_grad_ref's dict (pos None: every position):
    small_A / small_B (the tile's samples alone), big_A / big_B / big_AB (all M samples, everything else zero-signal with
    the returns taken from reference(None, None)'s new_value) -> ({run: dict}, A, B)"""
    A, B = tile_positions(case["flat"].size, w)
    v = reference(None, None)["new_value"]
    runs = {"small_A": reference(A, None), "small_B": reference(B, None)}
    for name, keep in (("big_A", A), ("big_B", B), ("big_AB", np.concatenate([A, B]))):
        runs[name] = reference(None, zero_signal(case, keep, v))
    return runs, A, B


# Part B: M = 2 TILE + 3 from a 260-lane buffer of pitch 272, some entries replaced by bad ones
def skipped_cases():
    return [("cartpole-2x(7,3)-skipped", "cartpole", 2, "2x(7,3)", "tanh", 260, 2 * TILE + 3, True),
            ("pendulum-1x5-skipped", "pendulum", 0, "1x5", "relu", 260, 2 * TILE + 3, False)]


def bad_positions(M):
    """the first position of a tile, the last position of the partial tile, one whole wavefront"""
    assert M % TILE and M > TILE + 128
    return np.concatenate([[TILE], [M - 1], np.arange(64, 128)])


def with_bad_entries(flat, T, pitch, n_lanes):
    """(idx, valid): flat with the entries at bad_positions() replaced, in turn, by -1, T * pitch, T * pitch + 1 and, where
    the rows have padding lanes, a padding lane's index t * pitch + n_lanes and t * pitch + pitch - 1 -- each within
    2 * pitch elements of the buffer"""
    bad = [-1, T * pitch, T * pitch + 1]
    if pitch > n_lanes:
        bad += [(T // 2) * pitch + n_lanes, pitch - 1, (T - 1) * pitch + pitch - 1]
    pos = bad_positions(flat.size)
    idx = flat.astype(np.int32).copy()
    idx[pos] = [bad[k % len(bad)] for k in range(pos.size)]
    valid = np.ones(flat.size, bool)
    valid[pos] = False
    return idx, valid


def rescaled(ref, n_valid, M):
    """a reference over the n_valid valid samples of a minibatch of M as the device reports it: the skipped samples add
    zero to every sum and the divisor stays M, so the gradients, their S and the five means shrink by n_valid / M"""
    out = dict(ref)
    for k in ("grad_actor", "grad_critic", "grad_log_std", "S_actor", "S_critic", "S_log_std"):
        out[k] = np.asarray(ref[k]) * (n_valid / M)
    out["stats"] = np.concatenate([ref["stats"][:5] * (n_valid / M), [M]])
    return out


# Part C: M = TILE + 1, the old log-probabilities replaced by the forward pass's own (r == 1) or moved by +- ln 2
def clip_edge_cases():
    return [("acrobot-1x5-clip-edge", "acrobot", 2, "1x5", "tanh", 260, TILE + 1, True),
            ("pendulum-2x(7,3)-clip-edge", "pendulum", 0, "2x(7,3)", "tanh", 260, TILE + 1, False)]


LN2_F32 = np.float32(np.log(2.0))


def clip_edge_columns(case, lp_forward, lp64, mixed):
    """(device column, reference column) of old log-probabilities for part C.  The device's: the forward pass's own float32
    log-probabilities lp_forward [M], so that lr = lp - log_prob == 0 and r == 1 exactly; with `mixed`, position m keeps
    that for m % 3 == 0 and gets fl32(lp - ln 2) (r about 2) for m % 3 == 1, fl32(lp + ln 2) (r about 1/2) for m % 3 == 2.
    Those ratios are not exact powers of two: lp -+ ln 2 is rounded wherever lp has bits below the sum's last place, so lr
    is +-ln 2 within an ulp of lp.  Nothing here needs them exact: the reference's column (float64) is lp64 minus the exact
    difference lp_forward - column, the log-ratio the device's subtraction rounds -- so the reference has the device's
    ratios within half an ulp, 1 exactly where the column holds lp_forward, and every moved ratio is far from 1."""
    M = case["flat"].size
    shift = np.zeros(M, np.float32)
    if mixed:
        shift[np.arange(M) % 3 == 1] = -LN2_F32
        shift[np.arange(M) % 3 == 2] = LN2_F32
    q = (lp_forward.astype(np.float32) + shift).astype(np.float32)
    dev = case["log_prob"].copy()
    dev.reshape(-1)[case["flat"]] = q
    ref = case["log_prob"].astype(np.float64)
    ref.reshape(-1)[case["flat"]] = lp64 - (lp_forward.astype(np.float64) - q.astype(np.float64))
    return dev, ref


def assert_conditioned(case, ref):
    """every float64 ratio at least 1e-4 from 1 +- CLIP; for ReLU every pre-activation at least 1e-4 in magnitude"""
    r = ref["ratio"]
    assert np.all(np.abs(r - (1 - CLIP)) >= 1e-4) and np.all(np.abs(r - (1 + CLIP)) >= 1e-4), case["id"]
    if case["actor"].activation == "relu":
        for v in ref["pre_actor"] + ref["pre_critic"]:
            assert np.all(np.abs(v) >= 1e-4), case["id"]


def grad_error_units(g, g64, S):
    """|g - g64| / (2^-24 S) per entry with S > 0; entries with S == 0 must be exact zeros"""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    zero = S == 0
    assert np.all(g[zero] == 0) and np.all(g64[zero] == 0)
    return np.abs(g - g64)[~zero] / (U * S[~zero])


def measure_k0():
    worst = (0.0, None)
    for case in grad_cases():
        c = make_case(case)
        r64, r32 = case_reference(c), case_reference(c, np.float32)
        assert_conditioned(c, r64)
        k = 0.0
        for name in ("actor", "critic"):
            k = max(k, grad_error_units(r32["grad_" + name], r64["grad_" + name], r64["S_" + name]).max())
        if not c["actor"].discrete:
            k = max(k, abs(float(r32["grad_log_std"]) - float(r64["grad_log_std"])) / (U * r64["S_log_std"]))
        print(f"{c['id']:40s} M = {c['flat'].size:6d}  k = {k:.3f}")
        if k > worst[0]:
            worst = (k, c["id"])
    print(f"k0 = {worst[0]:.2f} ({worst[1]})")
    return worst[0]


if __name__ == "__main__":
    measure_k0()
