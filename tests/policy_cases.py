"""What a closed-loop policy test case is made of, shared by test_policy_*.py and test_gpu_policy_*.py: the constants,
the ctypes structs of the host-side refusal tests, the engine and policy builders, and the host references (NumPy:
float64, or fp32 in the device's order).  policy_checks.py runs a case on the GPU and compares.  A plain module, like
sampling_ref.py: importing it allocates nothing and touches no device (make_engine does, when called)."""
import os

import numpy as np

import sampling_ref as SR
from carl_amd import _lib
from carl_amd.engine import VecEngine
from carl_amd.envs import CARLAcrobot, CARLCartPole, CARLMountainCar, CARLMountainCarContinuous, CARLPendulum
from carl_amd.policy import MLPPolicy

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "carl_amd.h")
FAMILIES = {_lib.CARTPOLE: CARLCartPole, _lib.PENDULUM: CARLPendulum, _lib.ACROBOT: CARLAcrobot,
            _lib.MOUNTAINCAR: CARLMountainCar, _lib.MOUNTAINCAR_CONT: CARLMountainCarContinuous}
# one physics feature per family varied across the context set
VARIED = {_lib.CARTPOLE: "length", _lib.PENDULUM: "l", _lib.ACROBOT: "LINK_MASS_2", _lib.MOUNTAINCAR: "gravity",
          _lib.MOUNTAINCAR_CONT: "power"}
SELECTORS = {"static": _lib.SEL_STATIC, "round_robin": _lib.SEL_ROUND_ROBIN, "random": _lib.SEL_RANDOM}
# observation shift / scale of the test policies: each entry's typical range mapped to about +-1
OBS_NORM = {_lib.CARTPOLE: ([0, 0, 0, 0], [10, 2, 10, 2]), _lib.PENDULUM: ([0, 0, 0], [1, 1, 0.5]),
            _lib.ACROBOT: ([1, 0, 1, 0, 0, 0], [10, 10, 10, 10, 2, 2]), _lib.MOUNTAINCAR: ([-0.5, 0], [10, 300]),
            _lib.MOUNTAINCAR_CONT: ([-0.5, 0], [10, 300])}
STATE_KEYS = ["state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "last_return", "last_length",
              "episodes_done", "ctx_obs"]
# step type -> (family, engine options): AcrobotFast is Acrobot under acrobot_fp32
STEP_TYPES = {"cartpole": (_lib.CARTPOLE, {}), "pendulum": (_lib.PENDULUM, {}), "acrobot": (_lib.ACROBOT, {}),
              "acrobot_fast": (_lib.ACROBOT, {"acrobot_fp32": True}), "mountaincar": (_lib.MOUNTAINCAR, {}),
              "mountaincar_cont": (_lib.MOUNTAINCAR_CONT, {})}
ACTS = ["identity", "tanh", "relu"]
# hidden widths of the deterministic kernel matrix: padded width 32 (every width <= 32) and 64, one and two layers
HIDDEN_SHAPES = [(w,) for w in (1, 4, 31, 32, 33, 64)] + [(64, 64), (33, 7), (5, 64), (32, 32)]
CTX_MODES = ["all", "none", "one", "permuted", "repeated"]
LOG_STDS = [-20.0, -0.5, 0.0, 2.0]
OPTIONS = {
    "acrobot_fp32": (_lib.ACROBOT, dict(acrobot_fp32=True)),
    "cartpole_recompute": (_lib.CARTPOLE, dict(cartpole_recompute=True)),
    "max_episode_steps_cartpole": (_lib.CARTPOLE, dict(max_episode_steps=5)),
    "max_episode_steps_pendulum": (_lib.PENDULUM, dict(max_episode_steps=5)),
    "lane_offset": (_lib.MOUNTAINCAR, dict(lane_offset=1000)),
    "sel_host": (_lib.CARTPOLE, dict(selector=_lib.SEL_HOST)),
    "sel_random": (_lib.ACROBOT, dict(selector=_lib.SEL_RANDOM)),
    "selector_stride": (_lib.ACROBOT, dict(selector_stride=3)),
    "ctx_obs_rows_subset": (_lib.CARTPOLE, dict(ctx_obs_rows=[5, 0, 3])),
    "no_auto_reset": (_lib.CARTPOLE, dict(auto_reset=False)),
}


# ---------------------------------------------------------------- host side only: never launched
def fake_engine(family=_lib.CARTPOLE, visible=None):
    """An engine object with the attributes the policy constructors read, never launched (no GPU needed)."""
    info = _lib.family_info(family)
    eng = object.__new__(VecEngine)
    eng.family, eng.D, eng.F, eng.n = family, int(info.obs_dim), int(info.n_features), 1000
    eng.info = info
    eng.ctx_obs_rows = list(range(eng.F)) if visible is None else list(visible)
    return eng


def rand_layers(rng, dims):
    return [(rng.normal(size=(o, i)).astype(np.float32), rng.normal(size=o).astype(np.float32))
            for i, o in zip(dims[:-1], dims[1:])]


def c_batch(family=_lib.CARTPOLE, n=1000, **kw):
    """A carl_batch_t whose device pointers are never dereferenced: every call it goes to is refused on the host first.
    kw: other batch fields (ctx_obs_feat: a sequence)."""
    b = _lib.Batch()
    b.family, b.n_lanes, b.n_contexts, b.ctx_stride = family, n, 4, 4
    for f in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "ctx_table"):
        setattr(b, f, 0x1000)
    for k, v in kw.items():
        if k == "ctx_obs_feat":
            for i, f in enumerate(v):
                b.ctx_obs_feat[i] = f
        else:
            setattr(b, k, v)
    return b


def c_policy(**kw):
    """A valid carl_policy_t for c_batch() (6 -> 64 -> 64 -> 2, tanh, argmax), kw: the fields to spoil"""
    p = _lib.Policy()
    p.n_in, p.n_ctx, p.n_hidden, p.n_out = 6, 2, 2, 2
    p.ctx_rows[0], p.ctx_rows[1] = 0, 3
    p.width[0], p.width[1] = 64, 64
    p.activation, p.head, p.n_sets, p.lanes_per_set, p.params = _lib.POLICY_TANH, _lib.POLICY_HEAD_ARGMAX, 1, 1024, 0x2000
    for k, v in kw.items():
        if k == "width":
            p.width[0], p.width[1] = v
        elif k == "ctx_rows":
            p.ctx_rows[0], p.ctx_rows[1] = v
        else:
            setattr(p, k, v)
    return p


# What the entry points answer c_batch(**batch_kw) with c_policy(**pol_kw), by the case names of the refusal tests: the
# whole message after "<entry point>: ".  Every closed-loop entry point runs these checks first and words them alike.
REFUSALS = {
    "width over the limit": b"hidden width[0] = 65 outside [1, 64]",
    "width zero": b"hidden width[1] = 0 outside [1, 64]",
    "too many layers": b"n_hidden 3 outside [0, 2]",
    "discrete head width": b"head width 3, the family needs 2 (n_actions)",
    "Box head width": b"head width 2, the family needs 1 (one Box value)",
    "Brax family": b"family 5 is a Brax family -- the closed-loop rollout covers the classic-control families only",
    "lanes_per_set not a multiple": b"lanes_per_set 300 is not a positive multiple of 256 (carl_policy_lane_quantum)",
    "lanes_per_set zero": b"lanes_per_set 0 is not a positive multiple of 256 (carl_policy_lane_quantum)",
    "sets do not cover": b"3 sets x 256 lanes do not cover 1000 lanes",
    "context row >= F": b"ctx_rows[1] = 8 is not a context-table row (F = 8)",
    "context row < 0": b"ctx_rows[0] = -1 is not a context-table row (F = 8)",
    "n_in mismatch": b"n_in 7 != n_ctx 2 + obs_dim 4",
    "head kind": b"head kind 1 does not match the family's action space",
    "activation": b"unknown activation 7",
    "no params": b"params is NULL",
    "context observation feature >= F": b"ctx_obs_feat[0] = 8 out of range",
    "no contexts": b"n_contexts 0 / ctx_stride 4 invalid",
}
# the sampling checks, in the order every entry point with a carl_policy_sampling_t runs them
SAMPLING_NULL = b"sampling is NULL"
SAMPLING_LOG_STD = b"a Box family needs sampling->log_std ([n_sets] on the device)"
SAMPLING_LOG_PROB_REFUSED = (b"sampling->log_prob is a transitions-mode output (io != NULL); this mode stores nothing per "
                             b"step")
SAMPLING_LOG_PROB_REQUIRED = b"a sampled launch with a critic stores the log-probabilities: sampling->log_prob is NULL"
SAMPLING_LOG_PROB_UNALIGNED = b"sampling->log_prob is not on a 16-byte boundary"
# (batch_kw, pol_kw, the REFUSALS case reported): two arguments spoilt at once, the earlier check answers
FIRST_OF_TWO = [
    ({"family": _lib.CARL_N_FAMILIES}, {"params": None}, "Brax family"),
    ({"n_contexts": 0}, {"n_hidden": 3}, "no contexts"),
    ({}, {"n_hidden": 3, "n_out": 3}, "too many layers"),
    ({}, {"width": (65, 64), "activation": 7}, "width over the limit"),
    ({}, {"n_out": 3, "activation": 7}, "discrete head width"),
    ({}, {"activation": 7, "lanes_per_set": 300}, "activation"),
    ({}, {"activation": 7, "params": None}, "activation"),
    ({}, {"lanes_per_set": 256, "n_sets": 3, "params": None}, "sets do not cover"),
]


def c_io(**kw):
    """A carl_step_io_t in the staged layout for c_batch() (int32 actions, rows of 1008 lanes), kw: the fields to spoil"""
    io = _lib.StepIO()
    io.action, io.obs, io.reward, io.terminated, io.truncated = 0x1000, 0x1000, 0x1000, 0x1000, 0x1000
    io.action_dtype, io.row_pitch = _lib.ACTION_I32, 1008
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def check_first_of_two(who, call):
    """``call(b, p)`` -> the entry point's code for that batch and policy (its other arguments valid, or spoilt where a
    later check would answer); asserts for every FIRST_OF_TWO case that the earlier check's whole message comes back"""
    lib = _lib.load()
    for batch_kw, pol_kw, case in FIRST_OF_TWO:
        code = call(c_batch(flags=_lib.FLAG_AUTORESET, **batch_kw), c_policy(**pol_kw))
        assert code == _lib.ERR_INVALID_ARGUMENT, (who, case)
        assert lib.carl_last_error() == who + b": " + REFUSALS[case], (who, case, lib.carl_last_error())


# ---------------------------------------------------------------- engines
def defaults(family):
    return np.array([float(f.default_value) for f in FAMILIES[family].get_context_features().values()])


def context_table(family, n_contexts, rng):
    names = list(FAMILIES[family].get_context_features())
    t = np.tile(defaults(family), (n_contexts, 1))
    t[:, names.index(VARIED[family])] *= rng.uniform(0.8, 1.25, n_contexts)
    return t


def make_engine(family, n, selector=_lib.SEL_ROUND_ROBIN, n_contexts=64, seed=0, **opts):
    """A reset engine on the GPU over context_table(family, n_contexts); opts: VecEngine's (auto_reset on by default)"""
    rng = np.random.default_rng(seed)
    eng = VecEngine(family, context_table(family, n_contexts, rng), n, "cuda", selector=selector,
                    auto_reset=opts.pop("auto_reset", True), seed=seed, **opts)
    eng.reset()
    return eng


# ---------------------------------------------------------------- policies
def n_outputs(eng):
    return int(eng.info.n_actions) if eng.info.action_is_discrete else 1


def random_policy(eng, seed=0, widths=(64, 64), head_gain=3.0, clip=None):
    """A random tanh MLP that sees every context row: inputs centred / scaled by the defaults, so that its actions
    vary with state and context."""
    rng = np.random.default_rng(seed)
    n_ctx = len(eng.ctx_obs_rows)
    d = defaults(eng.family)[eng.ctx_obs_rows]
    o_shift, o_scale = OBS_NORM[eng.family]
    shift = np.concatenate([d, o_shift])
    scale = np.concatenate([1.0 / np.maximum(np.abs(d), 1e-3) * 4.0, o_scale])
    dims = [n_ctx + eng.D, *widths, n_outputs(eng)]
    layers = []
    for k, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        gain = head_gain if k == len(dims) - 2 else 1.0
        layers.append((rng.normal(0, gain / np.sqrt(i), (o, i)), rng.normal(0, 0.1, o)))
    return MLPPolicy.for_env(eng, layers, "tanh", input_shift=shift, input_scale=scale, input_clip=clip)


def ctx_rows(eng, mode, rng):
    vis = list(eng.ctx_obs_rows)
    return {"all": vis, "none": [], "one": vis[-1:], "permuted": list(rng.permutation(vis)),
            "repeated": [vis[0], vis[-1], vis[0]]}[mode]


def make_policy(eng, widths, act, rng, ctx="all", clip=None, saturate=False, log_std=None):
    """A random policy over the given context rows, inputs centred / scaled to about +-1 (clip: a bound that binds);
    saturate: first-layer pre-activations up to 100 on the engine's current inputs (tanh then returns exactly +-1 for
    many units; first_layer_pre measures what a launch reached); log_std: a Box policy's, for sampled launches."""
    rows = ctx_rows(eng, ctx, rng)
    d = defaults(eng.family)[rows] if rows else np.zeros(0)
    o_shift, o_scale = OBS_NORM[eng.family]
    shift = np.concatenate([d, o_shift])
    scale = np.concatenate([4.0 / np.maximum(np.abs(d), 1e-3), o_scale]) * rng.uniform(0.8, 1.25, len(rows) + eng.D)
    dims = [len(rows) + eng.D, *widths, n_outputs(eng)]
    layers = [(rng.normal(0, 1.5 / np.sqrt(i), (o, i)), rng.normal(0, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]
    if saturate:
        layers[0] = saturate_units(eng, rows, shift, scale, clip, *layers[0])
    return MLPPolicy.for_env(eng, layers, act, input_shift=shift, input_scale=scale, input_clip=clip,
                             context_features=rows, log_std=log_std)


def saturate_units(eng, rows, shift, scale, clip, W, b):
    """(W, b) with each unit scaled so that its largest |pre-activation| over the lanes' current inputs is 100"""
    x0 = np.concatenate([eng.ctx_table.cpu().numpy()[rows][:, eng.ctx_idx.cpu().numpy()].T, eng.obs.cpu().numpy()], 1)
    lim = np.inf if clip is None else clip
    pre = np.clip((x0 - shift) * scale, -lim, lim) @ W.T + b
    c = 100.0 / np.maximum(np.abs(pre).max(axis=0), 1e-6)
    return W * c[:, None], b * c


def zero_head_policy(eng, head_bias=None, widths=(), log_std=None):
    """every weight random except the head's, which is zero: the head outputs are its biases whatever the input"""
    rng = np.random.default_rng(5)
    n_out = n_outputs(eng)
    dims = [len(eng.ctx_obs_rows) + eng.D, *widths, n_out]
    layers = [(rng.normal(0, 0.3, (o, i)), rng.normal(0, 0.1, o)) for i, o in zip(dims[:-1], dims[1:])]
    layers[-1] = (np.zeros((n_out, dims[-2])), np.zeros(n_out) if head_bias is None else np.asarray(head_bias))
    return MLPPolicy.for_env(eng, layers, "tanh", log_std=log_std)


def stacked_policy(eng, n_sets, lanes_per_set, rng, widths=(33, 7), act="relu"):
    """n_sets distinct weight sets (Box families: each with its own log_std)"""
    box = not eng.info.action_is_discrete
    sets = [make_policy(eng, widths, act, np.random.default_rng(rng.integers(1 << 30)), "all", clip=3.0,
                        log_std=LOG_STDS[s % 4] + 0.125 * s if box else None) for s in range(n_sets)]
    return MLPPolicy.stack(sets, lanes_per_set)


# ---------------------------------------------------------------- host references
def forward64(pol, x):
    """float64 forward pass of inputs x [N, n_in] from the policy's own layer arrays (not from the packed block, which
    oracle.policy_forward reads) -> head outputs [N, n_out]"""
    h = np.clip((x.astype(np.float64) - pol.shift) * pol.scale.astype(np.float64), -float(pol.clip), float(pol.clip))
    for k, (W, b) in enumerate(pol.layers):
        h = h @ W.astype(np.float64).T + b
        if k < len(pol.layers) - 1:
            h = np.tanh(h) if pol.activation == "tanh" else np.maximum(h, 0) if pol.activation == "relu" else h
    return h


def first_layer_pre(pol, x):
    """float64 first-layer pre-activations [T * n, width] of the inputs x [T, n, n_in] (one weight set)"""
    assert pol.n_sets == 1
    z = np.clip((x.reshape(-1, x.shape[-1]).astype(np.float64) - pol.shift) * pol.scale.astype(np.float64),
                -float(pol.clip), float(pol.clip))
    W, b = pol.layers[0]
    return z @ W.astype(np.float64).T + b


def host_summary(snap, out, T):
    """episode count / fp32 return sum in step order / length sum, from the transition rows"""
    rew = out["reward"].cpu().numpy()
    done = (out["terminated"] | out["truncated"]).cpu().numpy().astype(bool)
    ep_ret = snap["ep_return"].cpu().numpy().astype(np.float32).copy()
    elapsed = snap["elapsed"].cpu().numpy().astype(np.int64).copy()
    n = ep_ret.size
    count, ret_sum, len_sum = np.zeros(n, np.int64), np.zeros(n, np.float32), np.zeros(n, np.int64)
    for t in range(T):
        ep_ret = (ep_ret + rew[t]).astype(np.float32)
        elapsed += 1
        d = done[t]
        count += d
        ret_sum = np.where(d, (ret_sum + ep_ret).astype(np.float32), ret_sum)
        len_sum += np.where(d, elapsed, 0)
        ep_ret = np.where(d, np.float32(0), ep_ret)
        elapsed = np.where(d, 0, elapsed)
    return count, ret_sum, len_sum


def host_records(snap, out, K, T):
    """(episodes, stop step, return, length, terminated, (step, lane) of each record) of each lane's first K episodes,
    from transition rows [>= T, n]; a lane's stop step: right after its K-th episode ends, else T"""
    rew = out["reward"][:T].cpu().numpy()
    te = out["terminated"][:T].cpu().numpy().astype(bool)
    done = te | out["truncated"][:T].cpu().numpy().astype(bool)
    ep_ret = snap["ep_return"].cpu().numpy().astype(np.float32).copy()
    elapsed = snap["elapsed"].cpu().numpy().astype(np.int64).copy()
    n = ep_ret.size
    count, stop = np.zeros(n, np.int64), np.full(n, T, np.int64)
    ret, length = np.full((K, n), np.nan, np.float32), np.zeros((K, n), np.int32)
    term, at_step = np.zeros((K, n), np.uint8), np.full((K, n), -1, np.int64)
    for t in range(T):
        ep_ret = (ep_ret + rew[t]).astype(np.float32)
        elapsed += 1
        idx = np.nonzero(done[t] & (count < K))[0]
        k = count[idx]
        ret[k, idx], length[k, idx], term[k, idx], at_step[k, idx] = ep_ret[idx], elapsed[idx], te[t, idx], t
        count[idx] += 1
        stop[idx[count[idx] == K]] = t + 1
        ep_ret = np.where(done[t], np.float32(0), ep_ret)
        elapsed = np.where(done[t], 0, elapsed)
    return count, stop, ret, length, term, at_step


def words(eng, e, el, seed, lanes=None):
    """the Philox words of lanes `lanes` (default: every lane, in order) at counter fields e, el [T, len(lanes)]: global
    lane ids from the engine's lane_offset"""
    T, n = e.shape
    lanes = np.arange(n) if lanes is None else np.asarray(lanes)
    return SR.sample_words(seed, np.broadcast_to(lanes, (T, n)), e, el, lane_offset=int(eng.b.lane_offset))
