"""One named configuration per reachable classic-control kernel instance, and the instance it claims to reach.

carl_amd.hip launches, per family type (the five families and AcrobotFast = AcrobotT<float>, CARL_FLAG_ACROBOT_FP32):
`rollout_staged_kernel<Fam, AK, PLAIN, LDSCTX, MOVES, FIN, AR, DEEP>` (the entries of `staged_kernel`),
`rollout_kernel<Fam, LDS, A64>` and `step_kernel<Fam, LDS, A64>` (the four-way CARL_LAUNCH), `reset_kernel<Fam, LDS>`
(launch_reset) and `rollout_staged_pair_kernel<Acrobot, FamB, false, ARB>` (launch_pair).  Which one a launch takes
follows from lane count, context count, selector, action dtype, auto-reset, `final_obs`, the finished-episode log, the
direct flag and the row layout; `carl_rollout_plan_io` reports what the library's rule decided.  tests/
test_classic_kernel_table.py holds this table against the source and the plan query on the host (a kernel without a
case, or a case the rule routes elsewhere, fails there); tests/test_gpu_classic_kernel_matrix.py runs every case
against the float64 oracle.

An instance is a tuple: ("staged", Fam, AK, PLAIN, LDSCTX, MOVES, FIN, AR, DEEP), ("direct", Fam, LDS, A64),
("step", Fam, LDS, A64), ("reset", Fam, LDS), ("pair", FamB, ARB).

Cases that share a `group` differ only in action dtype or route (staged / direct flag / direct shape) and are fed the
same contexts and action VALUES: their outputs must agree bit for bit.

AcrobotFast bar.  `ACROBOT_FAST_F32_DEVIATION` is the worst `rel_err` of the oracle's own float32 variant from its
float64 variant over exactly this table's AcrobotFast inputs (tests/test_classic_kernel_table.py measures it again and
holds the constant to it); the bar is max(5e-5, 3 x that) -- see tests/test_gpu_classic_kernel_matrix.py.
"""
import zlib

import numpy as np

from carl_amd import _lib

FAMS = ["CartPole", "Pendulum", "Acrobot", "MountainCar", "MountainCarCont", "AcrobotFast"]
FAMILY_ID = {"CartPole": _lib.CARTPOLE, "Pendulum": _lib.PENDULUM, "Acrobot": _lib.ACROBOT,
             "MountainCar": _lib.MOUNTAINCAR, "MountainCarCont": _lib.MOUNTAINCAR_CONT, "AcrobotFast": _lib.ACROBOT}
CONTINUOUS = {"Pendulum", "MountainCarCont"}
DTYPE_CODE = {"i32": _lib.ACTION_I32, "i64": _lib.ACTION_I64, "u8": _lib.ACTION_U8, "f32": _lib.ACTION_F32,
              "f16": _lib.ACTION_F16, "bf16": _lib.ACTION_BF16}
AK = {"i32": 0, "f32": 0, "i64": 1, "u8": 2, "f16": 3, "bf16": 4}
STATIC, RR, RANDOM = _lib.SEL_STATIC, _lib.SEL_ROUND_ROBIN, _lib.SEL_RANDOM
SEL_NAME = {STATIC: "static", RR: "rr", RANDOM: "random"}

N = 1003           # a partial last workgroup (3 x 256 + 235) and, through the row pitch, n % 16 = 11
N_WIDE = 1008      # rows of WIDE_PITCH lanes: the columns behind the lanes are not the launch's
WIDE_PITCH = 1040
C_LDS, C_GLOBAL = 37, 200   # 8 x 37 <= 1003 < 8 x 200: the table in LDS / in global memory
FULL = {"CartPole": 65536 + 11, "Pendulum": 32768 + 11}  # at or above the family's DEEP threshold, still ragged
BIG_STEP = 256 * 1024 + 77  # pick_block: more than 262 144 lanes take 256-thread workgroups without an LDS table

# measured on this table's AcrobotFast inputs (test_classic_kernel_table.py::test_acrobot_fast_bar_comes_from_...)
ACROBOT_FAST_F32_DEVIATION = 2.32e-6
ACROBOT_FAST_BAR = max(5e-5, 3 * ACROBOT_FAST_F32_DEVIATION)


class Case:
    def __init__(self, kind, fam, instance, *, n=N, n_ctx=C_LDS, selector=STATIC, dtype=None, auto_reset=True,
                 final_obs=False, fin=False, direct=False, layout="padded", T=9, max_steps=None, group=None, tag=""):
        self.kind, self.fam, self.instance = kind, fam, tuple(instance)
        self.n, self.n_ctx, self.selector = n, n_ctx, selector
        self.dtype = dtype or ("f32" if fam in CONTINUOUS else "i32")
        self.auto_reset, self.final_obs, self.fin, self.direct, self.layout = auto_reset, final_obs, fin, direct, layout
        self.T = T
        # episodes end inside the window: T = 1 truncates on its only step; CartPole's longer windows leave room for
        # natural terminations (a random policy drops the pole in ~20 steps) beside the truncations
        self.max_steps = max_steps if max_steps is not None else (1 if T == 1 else 5 if T < 30 else
                                                                   23 if fam == "CartPole" else 7)
        route = "flag" if direct else "shape" if layout == "dense" else layout
        self.label = "-".join(x for x in (kind, fam, tag, self.dtype, route if kind in ("staged", "direct") else "",
                                          f"n{n}") if x)
        self.group = group or self.label

    family = property(lambda self: FAMILY_ID[self.fam])
    fp32 = property(lambda self: self.fam == "AcrobotFast")
    seed = property(lambda self: zlib.crc32(self.group.encode()) & 0x7FFFFFFF)

    def __repr__(self):
        return self.label

    # ---- what the library is asked
    def flags(self):
        return (_lib.FLAG_AUTORESET if self.auto_reset else 0) | (_lib.FLAG_ACROBOT_FP32 if self.fp32 else 0) | (
            _lib.FLAG_ROLLOUT_DIRECT if self.direct else 0)

    def row_pitch(self):
        """carl_step_io_t::row_pitch of the case's buffers (0 = dense rows)"""
        if self.layout == "wide":
            return WIDE_PITCH
        if self.layout == "dense" or self.direct:
            return 0
        p = (self.n + 15) // 16 * 16
        return p if p != self.n else 0

    def host_batch_io(self):
        """carl_batch_t / carl_step_io_t of the case with dummy device pointers (never dereferenced by the plan query or by
        the argument checks): every array on a 4 KiB boundary, as an allocation of its own would be"""
        b, io = _lib.Batch(), _lib.StepIO()
        b.family, b.n_lanes, b.n_contexts, b.ctx_stride = self.family, self.n, self.n_ctx, self.n_ctx
        b.max_episode_steps, b.selector, b.selector_stride, b.flags = self.max_steps, self.selector, 3, self.flags()
        ptr = iter(range(0x100000, 0x200000, 0x1000))
        for f in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "ctx_table"):
            setattr(b, f, next(ptr))
        if self.fin:
            b.fin_capacity = 1 << 16
            for f in ("fin_count", "fin_lane", "fin_return", "fin_length"):
                setattr(b, f, next(ptr))
        io.action_dtype, io.row_pitch = DTYPE_CODE[self.dtype], self.row_pitch()
        for f in ("action", "obs", "reward", "terminated", "truncated"):
            setattr(io, f, next(ptr))
        if self.final_obs:
            io.final_obs = next(ptr)
        return b, io


def plan_of(batch, io):
    """carl_rollout_plan_io's answer for a batch with these buffers"""
    import ctypes as C

    p = _lib.RolloutPlan()
    _lib.check(_lib.load().carl_rollout_plan_io(C.byref(batch), C.byref(io), C.byref(p)))
    return p


def instance_of(case, plan):
    """the instance tuple the plan names for a launch of `case.kind` (None: the library has none / declines)"""
    fam = "AcrobotFast" if plan.acrobot_fp32 else next(f for f in FAMS if FAMILY_ID[f] == case.family)
    a64 = case.dtype == "i64"
    if case.kind == "reset":
        return ("reset", fam, bool(plan.use_lds_ctx))
    if case.kind == "step":
        return None if plan.ak >= 2 else ("step", fam, bool(plan.use_lds_ctx), a64)
    if plan.unsupported:
        return None
    if plan.variant == _lib.ROLLOUT_STAGED:
        if not plan.has_staged_kernel:
            return None
        return ("staged", fam, plan.ak) + tuple(bool(getattr(plan, k)) for k in ("plain", "ldsctx", "moves", "fin", "ar", "deep"))
    return ("direct", fam, bool(plan.use_lds_ctx), a64)


def pair_instance_of(plan_a, plan_b, fam_b):
    """launch_pair: both parts lean staged rollouts with int32 / float32 actions; the second family's AR is the only
    template argument that varies"""
    ok = plan_a.lean and plan_b.lean and plan_a.ak == 0 and plan_b.ak == 0 and not plan_a.acrobot_fp32
    return ("pair", fam_b, bool(plan_b.ar)) if ok else None


def _staged(fam, ak, plain=0, ldsctx=0, moves=0, fin=0, ar=0, deep=0):
    return ("staged", fam, ak, bool(plain), bool(ldsctx), bool(moves), bool(fin), bool(ar), bool(deep))


def _cases():
    out = []
    for fam in FAMS:
        cont = fam in CONTINUOUS
        wide, narrow = ("f32", None) if cont else ("i32", "i64")
        # ---- the generic done path (finished-episode log, terminal observations, moving contexts) and, fed the same
        # inputs, the direct-store kernels by flag and by shape: table in global memory / round robin, in LDS / random
        for tab, n_ctx, sel, lds, T in (("glb", C_GLOBAL, RR, 0, 37), ("lds", C_LDS, RANDOM, 1, 9)):
            kw = dict(n_ctx=n_ctx, selector=sel, final_obs=True, fin=True, T=T, group=f"generic-{fam}-{tab}", tag=tab)
            out.append(Case("staged", fam, _staged(fam, 0, ldsctx=lds), dtype=wide, **kw))
            if cont:  # one direct instance per table placement, by flag and by shape
                out.append(Case("direct", fam, ("direct", fam, bool(lds), False), direct=True, **kw))
                out.append(Case("direct", fam, ("direct", fam, bool(lds), False), layout="dense", **kw))
            else:
                out.append(Case("staged", fam, _staged(fam, 1, ldsctx=lds), dtype="i64", **kw))
                flag64 = bool(lds)  # glb: int32 by flag, int64 by shape; lds: the other way round
                out.append(Case("direct", fam, ("direct", fam, bool(lds), flag64), dtype="i64" if flag64 else "i32",
                                direct=True, **kw))
                out.append(Case("direct", fam, ("direct", fam, bool(lds), not flag64), dtype="i32" if flag64 else "i64",
                                layout="dense", **kw))
        # ---- the lean staged configuration
        dense_done, deep = fam == "CartPole", fam in FULL
        for ar in ((1, 0) if dense_done else (0,)):
            auto = bool(ar) if dense_done else True
            tag = ("ar" if ar else "noar") if dense_done else ""
            g = f"lean-{fam}-{tag}"
            kw = dict(auto_reset=auto, T=37 if auto else 21, tag=tag)
            # (a family with a DEEP threshold takes DEEP below it with int32 / float32 actions, the lean instance at full size)
            out.append(Case("staged", fam, _staged(fam, 0, plain=1, ar=ar, deep=deep), dtype=wide, group=g, **kw))
            if deep:
                kwf = dict(kw, n=FULL[fam], T=9)
                out.append(Case("staged", fam, _staged(fam, 0, plain=1, ar=ar), dtype=wide, group=g + "-full", **kwf))
                half = "f16" if cont else "u8"  # a narrow format above the threshold too
                out.append(Case("staged", fam, _staged(fam, AK[half], plain=1, ar=ar), dtype=half, group=g + "-full", **kwf))
            if cont:
                out.append(Case("staged", fam, _staged(fam, 3, plain=1), dtype="f16", group=g, **kw))
                out.append(Case("staged", fam, _staged(fam, 4, plain=1), dtype="bf16", group=g, **kw))
            else:
                out.append(Case("staged", fam, _staged(fam, 1, plain=1, ar=ar), dtype="i64", group=g, **kw))
                out.append(Case("staged", fam, _staged(fam, 2, plain=1, ar=ar), dtype="u8", group=g, **kw))
        if not dense_done:
            # auto-reset off where it is no template argument: a finished lane runs on (T = 1: done on the only step);
            # and rows of a wider array -- the columns behind the lanes must stay as they were
            out.append(Case("staged", fam, _staged(fam, 0, plain=1, deep=deep), dtype=wide, auto_reset=False, T=9, tag="noauto"))
            # a launch of ONE step that ends every episode: terminal observations on, so that the oracle sees the step's own
            # observation (a done row's `obs` is the next episode's)
            out.append(Case("staged", fam, _staged(fam, 0, ldsctx=1), dtype=wide, selector=RR, final_obs=True, fin=True, T=1,
                            tag="one"))
        out.append(Case("staged", fam, _staged(fam, 0 if cont else 1, plain=1, ar=dense_done, deep=cont and deep),
                        dtype="f32" if cont else "i64",
                        n=N_WIDE, layout="wide", T=21, tag="wide"))
        if dense_done:
            # ---- the dense done path: terminal observations, moving lanes, the table in LDS or not (no finished-episode log)
            for moves, ldsctx, fin, sel, T in ((0, 0, 1, STATIC, 1), (1, 0, 0, RR, 37), (1, 0, 1, RANDOM, 9),
                                               (1, 1, 0, RANDOM, 37), (1, 1, 1, RR, 21)):
                tag = f"dense{'M' if moves else ''}{'L' if ldsctx else ''}{'F' if fin else ''}"
                for dt in ("i32", "i64"):
                    out.append(Case("staged", fam, _staged(fam, AK[dt], plain=1, ldsctx=ldsctx, moves=moves, fin=fin), dtype=dt,
                                    n_ctx=C_LDS if ldsctx or not moves else C_GLOBAL, selector=sel, final_obs=bool(fin), T=T,
                                    group=f"{tag}-{fam}", tag=tag))
        # ---- per-call step: both sides of pick_block's block size without an LDS table, the LDS table, both action widths
        for dt in (("f32",) if cont else ("i32", "i64")):
            a64 = dt == "i64"
            out.append(Case("step", fam, ("step", fam, False, a64), dtype=dt, n_ctx=N, tag="b64"))
            out.append(Case("step", fam, ("step", fam, False, a64), dtype=dt, n=BIG_STEP, n_ctx=4096 * 8 + 1, tag="b256"))
            out.append(Case("step", fam, ("step", fam, True, a64), dtype=dt, n_ctx=C_LDS, tag="lds"))
        # ---- reset
        out.append(Case("reset", fam, ("reset", fam, False), n_ctx=C_GLOBAL, tag="glb"))
        out.append(Case("reset", fam, ("reset", fam, True), n_ctx=C_LDS, tag="lds"))
    return out


CASES = _cases()
BY_LABEL = {c.label: c for c in CASES}
assert len(BY_LABEL) == len(CASES), "case labels must be unique"
ROLLOUT_CASES = [c for c in CASES if c.kind in ("staged", "direct")]
STEP_CASES = [c for c in CASES if c.kind == "step"]
RESET_CASES = [c for c in CASES if c.kind == "reset"]
STEP_BLOCK = {"b64": 64, "b256": 256, "lds": 256}  # the per-call block size a step case's tag claims


def groups():
    g = {}
    for c in ROLLOUT_CASES:
        g.setdefault(c.group, []).append(c)
    return {k: v for k, v in g.items() if len(v) > 1}


# Acrobot (float64) + one other family in ONE launch; unequal lane counts, T not a multiple of the pair's 4-step chunk
PAIR_CASES = [  # (second family, its auto-reset, instance)
    ("CartPole", False, ("pair", "CartPole", False)),
    ("CartPole", True, ("pair", "CartPole", True)),
    ("Pendulum", True, ("pair", "Pendulum", False)),
    ("MountainCar", True, ("pair", "MountainCar", False)),
    ("MountainCarCont", True, ("pair", "MountainCarCont", False)),
]
PAIR_N_A, PAIR_N_B, PAIR_T = 779, 1003, 9


def pair_parts(fam_b, auto_b):
    """-> (Acrobot case, second case) of a pair launch: both lean staged, int32 / float32"""
    a = Case("staged", "Acrobot", _staged("Acrobot", 0, plain=1), n=PAIR_N_A, T=PAIR_T, group=f"pair-{fam_b}-{auto_b}-a", tag="pairA")
    b = Case("staged", fam_b, (), n=PAIR_N_B, T=PAIR_T, auto_reset=auto_b, group=f"pair-{fam_b}-{auto_b}-b", tag="pairB")
    return a, b


# instantiated, never launched: validate_io refuses int64 actions for the Box families before any launch
UNREACHABLE = sorted(
    [_staged(f, 1, plain=p, ldsctx=l) for f in CONTINUOUS for p, l in ((0, 0), (0, 1), (1, 0))]
    + [(k, f, lds, True) for k in ("step", "direct") for f in CONTINUOUS for lds in (False, True)], key=str)


# ---------------------------------------------------------------- inputs (the same on the CPU and on the GPU)
def table_and_actions(case):
    """-> (context table [C, F] float64 of float32 values, action VALUES [T, n] int32 / float32) of a case's group"""
    from test_gpu_parity import random_actions, random_table

    rng = np.random.default_rng(case.seed)
    table = random_table(case.family, rng, case.n_ctx)
    acts = random_actions(case.family, rng, (case.T, case.n))
    if case.dtype in ("f16", "bf16") or any(c.dtype in ("f16", "bf16") for c in groups().get(case.group, [])):
        import torch

        # values both half formats hold exactly (8 fraction bits survive bfloat16): the whole group is fed the same numbers
        acts = torch.as_tensor(acts).to(torch.bfloat16).to(torch.float16).to(torch.float32).numpy()
    return table, acts


def engine_kwargs(case):
    """keyword arguments common to carl_amd.engine.VecEngine and (max_steps / autoreset renamed) oracle.Engine"""
    return dict(selector=case.selector, selector_stride=3, seed=case.seed % 100003, lane_offset=7)


def step_inputs(case):
    """-> (context table, ctx_idx [n], states [n, S] float32, actions [n]) of a per-call step case: test_gpu_parity's
    random-transition distributions; AcrobotFast on the typical states its recorded 5e-5 bar was stated for"""
    from oracle import oracle as O
    from test_gpu_parity import random_actions, random_table

    rng = np.random.default_rng(case.seed)
    n, fam, U = case.n, case.family, None
    U = rng.uniform
    table = random_table(fam, rng, case.n_ctx)
    idx = (np.arange(n) % case.n_ctx).astype(np.int32)
    if fam == O.CARTPOLE:
        s = np.stack([U(-2.5, 2.5, n), U(-3, 3, n), U(-0.22, 0.22, n), U(-3, 3, n)], 1)
    elif fam == O.PENDULUM:
        s = np.stack([U(-10, 10, n), U(-8, 8, n)], 1)
    elif case.fp32:
        s = np.stack([U(-np.pi, np.pi, n), U(-np.pi, np.pi, n), U(-3, 3, n), U(-6, 6, n)], 1)
    elif fam == O.ACROBOT:
        s = np.stack([U(-np.pi, np.pi, n), U(-np.pi, np.pi, n), U(-4 * np.pi, 4 * np.pi, n), U(-9 * np.pi, 9 * np.pi, n)], 1)
    else:
        s = np.stack([U(-1.2, 0.6, n), U(-0.07, 0.07, n)], 1)
    return table, idx, s.astype(np.float32), random_actions(fam, rng, n)


def oracle_rollout(case, precision="f32"):
    """The case's rollout on the CPU oracle of `precision`, from a reset: -> (s0 [n, S], per-step context rows
    [T, n, F], outputs as [T, ...] arrays incl. final_obs).  What the matrix feeds the kernels, stepped by the
    oracle's own float32 variant: the states the kernels visit up to rounding."""
    from oracle import oracle as O

    table, acts = table_and_actions(case)
    kw = engine_kwargs(case)
    ora = O.Engine(case.family, table, case.n, autoreset=case.auto_reset, max_steps=case.max_steps, precision=precision, **kw)
    ora.reset()
    s0 = ora.state.astype(np.float64)
    ctx, outs = [], {k: [] for k in ("obs", "reward", "terminated", "truncated", "final_obs")}
    for t in range(case.T):
        ctx.append(table[ora.ctx_idx])
        o = ora.step(acts[t])
        for k in outs:
            outs[k].append(np.array(getattr(o, k)))
    return s0, np.stack(ctx), {k: np.stack(v) for k, v in outs.items()}


def flatten_rollout(case, s0, ctx, acts, out):
    """(t, lane) -> one row: the arguments of test_gpu_parity.restep_rollout_with_oracle for a rollout whose lanes may
    change contexts -- each row carries the context row its step ran in (`ctx` [T, n, F]) and starts from the state the
    previous output row determines, so ONE call re-steps the whole rollout under the helper's one cap of threshold-edge
    flags.  Without auto-reset a lane runs on after its episode ended; CartPole then pays reward 0 (gymnasium's step
    after termination, tests/test_gpu_parity.py::test_cartpole_reward_after_termination), which a single transition
    of the oracle does not model: rows of a lane that terminated earlier are left to the per-call comparison.
    -> (context rows, start states, actions [1, rows], outputs [1, rows, ...], rows kept)"""
    import torch
    from test_gpu_parity import state_from_obs

    T, n = acts.shape
    out = {k: torch.as_tensor(v)[:T].cpu() for k, v in out.items()}
    prev = [np.asarray(s0, dtype=np.float64)] + [state_from_obs(case.family, out["obs"][t].numpy()) for t in range(T - 1)]
    keep = np.ones((T, n), bool)
    if not case.auto_reset:
        term = out["terminated"].numpy() != 0
        keep[1:] = ~(np.cumsum(term, axis=0)[:-1] > 0)
    k = torch.as_tensor(keep.reshape(-1))
    flat = {name: v.reshape((T * n,) + tuple(v.shape[2:]))[k][None] for name, v in out.items()}
    k = keep.reshape(-1)
    return (ctx.reshape(T * n, -1)[k], np.concatenate(prev)[k], torch.as_tensor(np.ascontiguousarray(acts)).reshape(T * n)[k][None],
            flat, int(k.sum()))
