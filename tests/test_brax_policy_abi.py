"""Host side of the Brax closed-loop rollout (include/carl_amd.h: carl_brax_rollout_policy): everything that runs before
a HIP call.  Refusals by their messages, BraxMLPPolicy's packing against MLPPolicy's and against the layout written out
by hand, the launch-shape query, the one list of closed-loop kernel instances (brax_policy_host.hpp) against
carl_brax.hip's table and against the three units that expand it, and that the shape rule it shares with reset / step /
rollout (brax_launch.hpp) still answers for those what it did: OPEN_SHAPES holds what
carl_brax_launch_shape must report for them, recorded from the launches of the commit before the rule moved."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import brax_policy_abi_util as U
import brax_policy_cases as BP
from brax_policy_abi_util import batch as _batch, info as _info, policy as _policy
from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import MLPPolicy
from policy_cases import fake_engine, rand_layers

_refused = functools.partial(U.refused, b"carl_brax_rollout_policy: ", want=None)


def _io():
    io = _lib.StepIO()
    io.action, io.obs, io.reward, io.terminated, io.truncated = 0x1000, 0x1000, 0x1000, 0x1000, 0x1000
    io.action_dtype = _lib.ACTION_F32
    return io


def _call(b, s, p, io=None, summary=True, n_steps=10):
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    return _lib.load().carl_brax_rollout_policy(C.byref(b), 0x4000, C.byref(s), 0x5000, C.byref(p),
                                                None if io is None else C.byref(io), n_steps,
                                                C.byref(summ) if summary else None, None)


def test_refusals_by_their_messages():
    ant = BP.build_model("ant")[0]
    hum = BP.build_model("humanoid")[0]
    inv, uns = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    # Humanoid: 244 observations against CARL_POLICY_MAX_IN = 32 (whatever n_in says)
    code = _call(_batch(), hum, _policy(hum))
    assert code == inv
    _refused(code, b"2 context inputs + 244 observations are more than CARL_POLICY_MAX_IN = 32 policy inputs "
                   b"(Humanoid-size observations are out of scope)")
    code = _call(_batch(), ant, _policy(ant, n_out=1))
    assert code == inv
    _refused(code, b"head width 1, the model has 8 actuators")
    code = _call(_batch(), ant, _policy(ant, head=_lib.POLICY_HEAD_ARGMAX))
    assert code == inv
    _refused(code, b"head kind 0: the Brax families take Box actions (CARL_POLICY_HEAD_BOX)")
    code = _call(_batch(flags=_lib.FLAG_AUTORESET | _lib.FLAG_BRAX_FP32), ant, _policy(ant))
    assert code == uns
    _refused(code, b"CARL_FLAG_BRAX_FP32 is not built for the closed-loop rollout (the float64 kernel classes only)")
    code = _call(_batch(), ant, _policy(ant, lanes_per_set=256, n_sets=3))
    assert code == inv
    _refused(code, b"3 sets x 256 lanes do not cover 1000 lanes")
    code = _call(_batch(), ant, _policy(ant, lanes_per_set=300))
    assert code == inv
    _refused(code, b"lanes_per_set 300 is not a positive multiple of 256 (carl_policy_lane_quantum)")
    for io in (None, _io()):  # a summary without auto-reset, in either mode
        code = _call(_batch(flags=0), ant, _policy(ant), io=io)
        assert code == uns
        _refused(code, b"a summary needs CARL_FLAG_AUTORESET (without auto-reset a finished lane reports done on every "
                       b"later step, and its episode would be counted on each of them)")
    # further checks of the policy and the call
    code = _call(_batch(), ant, _policy(ant, n_in=30))
    _refused(code, b"n_in 30 != n_ctx 2 + obs_dim 27")
    p = _policy(ant)
    p.ctx_rows[1] = 5
    _refused(_call(_batch(), ant, p), b"ctx_rows[1] = 5 is not one of the batch's observed context rows (ctx_obs_feat)")
    _refused(_call(_batch(), ant, _policy(ant, params=0x2004)),
             b"params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)")
    _refused(_call(_batch(), ant, _policy(ant, activation=7)), b"unknown activation 7")
    p = _policy(ant)
    p.width[0] = 65
    _refused(_call(_batch(), ant, p), b"hidden width[0] = 65 outside [1, 64]")
    _refused(_call(_batch(), ant, _policy(ant), io=None, summary=False), b"summary mode (io NULL) needs all three summary arrays")
    io = _io()
    io.row_pitch = 1008
    _refused(_call(_batch(), ant, _policy(ant), io=io, summary=False), b"Brax families take dense rows (io.row_pitch = 0)")
    _refused(_call(_batch(), ant, _policy(ant), n_steps=-1), b"n_steps -1 < 0")
    # the batch is checked as carl_brax_rollout checks it
    _refused(_call(_batch(n_contexts=0), ant, _policy(ant)), b"n_contexts 0 / ctx_stride 4 invalid")
    # nothing to do: valid, nothing enqueued
    assert _call(_batch(n=0), ant, _policy(ant)) == 0


def test_the_pinned_refusals_of_the_classic_entry_points_stay():
    from carl_amd.brax_engine import BraxVecEngine

    rng = np.random.default_rng(0)
    with pytest.raises(TypeError, match="classic-control"):
        MLPPolicy.for_env(object.__new__(BraxVecEngine), rand_layers(rng, [4, 2]))
    with pytest.raises(NotImplementedError):
        object.__new__(BraxVecEngine).evaluate_policy(None, 1, 1)
    with pytest.raises(TypeError, match="BraxMLPPolicy"):  # the engine's own launch takes the Brax class only
        object.__new__(BraxVecEngine).rollout_policy(
            MLPPolicy.for_env(fake_engine(_lib.CARTPOLE, [0, 3]), rand_layers(rng, [6, 2])), 1)
    with pytest.raises(TypeError, match="not a CARLBraxEnv or BraxVecEngine"):
        BraxMLPPolicy.for_env(fake_engine(_lib.CARTPOLE, [0, 3]), rand_layers(rng, [6, 2]))


@pytest.mark.parametrize("widths,act", BP.NETWORKS)
def test_packs_the_bytes_mlp_policy_packs(widths, act):
    """for a shape both classes take -- Pendulum's: 3 observations, one Box output -- the same packed block, struct
    fields and set size; for Ant's shape (8 outputs, which carl_policy_set_floats refuses) the block written out by
    hand, and carl_brax_policy_set_floats of its struct"""
    rng = np.random.default_rng(3)
    lib = _lib.load()
    rows = [0, 3]
    layers = BP.make_layers(rng, 5, widths, 1)
    shift, scale, clip = BP.transform(rng, 5)
    classic = MLPPolicy(_lib.PENDULUM, 3, rows, layers, act, shift, scale, clip)
    brax = BraxMLPPolicy(_info(3, 1), rows, layers, act, shift, scale, clip)
    assert brax.params.tobytes() == classic.params.tobytes()
    a, b = classic.struct(1000), brax.struct(1000)
    for f, _ in _lib.Policy._fields_:
        if f not in ("ctx_rows", "width", "params"):
            assert getattr(a, f) == getattr(b, f), f
    assert list(a.ctx_rows) == list(b.ctx_rows) and list(a.width) == list(b.width)
    assert lib.carl_brax_policy_set_floats(C.byref(b)) == lib.carl_policy_set_floats(C.byref(a)) == brax.set_floats

    layers = BP.make_layers(rng, 29, widths, 8)
    shift, scale, clip = BP.transform(rng, 29)
    ant = BraxMLPPolicy(_info(27, 8), rows, layers, act, shift, scale, clip)
    np.testing.assert_array_equal(ant.params[0].view(np.int32), BP.pack(layers, shift, scale, clip).view(np.int32))
    st = ant.struct(1000)
    assert (st.n_in, st.n_out, st.head, st.lanes_per_set) == (29, 8, _lib.POLICY_HEAD_BOX, 1024)
    assert lib.carl_policy_set_floats(C.byref(st)) == -1  # (the classic limit of 4 outputs stays)
    assert lib.carl_brax_policy_set_floats(C.byref(st)) == ant.set_floats == ant.params.shape[1]
    # stack and on_device keep the class
    two = BraxMLPPolicy.stack([ant, ant], 256)
    assert type(two) is BraxMLPPolicy and two.n_sets == 2 and two.lanes_per_set == 256
    with pytest.raises(ValueError, match="same family"):
        MLPPolicy.stack([classic, brax], 256)
    with pytest.raises(ValueError, match="head width 7"):
        BraxMLPPolicy(_info(27, 8), rows, BP.make_layers(rng, 29, widths, 7), act)
    with pytest.raises(ValueError, match="at most 32"):
        BraxMLPPolicy(_info(244, 17), rows, BP.make_layers(rng, 246, widths, 17), act)


def _open_loop_entries(pattern):
    body = re.search(r"const \w+ kBraxKernels\[\] = \{(.*?)\n\};", U.source("carl_brax.hip", comments=False), re.S).group(1)
    return re.findall(pattern, body)


def _instance_list():
    """the (MULTI, K, TASK, PLANAR) of CARL_BRAX_CLOSED_LOOP_INSTANCES in its order, read off brax_policy_host.hpp"""
    body = re.search(r"#define CARL_BRAX_CLOSED_LOOP_INSTANCES\(X\)((?:[^\n]*\\\n)+[^\n]*)", U.source("brax_policy_host.hpp"))
    return re.findall(r"X\((\w+), (\d+), (\w+), (\w+)\)", body.group(1))


def test_kernel_table_is_the_float64_step_classes_of_the_open_loop_table():
    """the one list of closed-loop instances holds 16 distinct ones: the non-F32 step classes of carl_brax.hip's
    kBraxKernels at the same widths, and the models of the GPU test reach every one of them"""
    b = lambda v: v == "true"  # noqa: E731
    want = {(b(m), b(t), False, int(k)) for m, k, t in _open_loop_entries(r"CARL_BRAX\((\w+), (\d+), (\w+)\)")}
    want |= {(b(m), False, b(p), int(k)) for m, k, p, f in _open_loop_entries(r"CARL_BRAX_STEP\((\w+), (\d+), (\w+), (\w+)\)")
             if not b(f)}
    listed = _instance_list()
    assert len(listed) == 16 and len(set(listed)) == 16
    got = {(b(m), b(t), b(p), int(k)) for m, k, t, p in listed}
    assert got == want and len(got) == 16
    reached = {(*BP.MODELS[m], w) for m, w in BP.instance_cases()}
    assert reached == got


UNITS = {"carl_brax_policy.hip": "brax_policy_kernel", "carl_brax_episodes.hip": "brax_episodes_kernel",
         "carl_brax_policy_stats.hip": "brax_episodes_stats_kernel"}


def test_each_unit_expands_the_instance_list_once_with_its_own_kernel():
    """every unit's table is one expansion of the list, entry by entry its own kernel template at the entry's parameters
    (so the three tables hold the same instances in the same order: the launch-shape rule picks a width out of any of
    them, and carl_brax_policy_launch_shape answers for all three entry points); nothing else in a unit instantiates a
    closed-loop kernel or writes an instance out, and no unit names anything of the variants stacked on it"""
    for unit, kernel in UNITS.items():
        src = U.source(unit, comments=False)
        table = re.search(r"#define X\(M, K, T, P\) \{\{M, T, P, false\}, K, carl::brax::(\w+)<M, K, T, P>\},\n"
                          r"const [\w:<>]+ \w+\[\] = \{\s*CARL_BRAX_CLOSED_LOOP_INSTANCES\(X\)\};\n#undef X\n", src)
        assert table is not None and table.group(1) == kernel, unit
        rest = src.replace(table.group(0), "")
        assert "CARL_BRAX_CLOSED_LOOP_INSTANCES" not in rest, unit
        assert not re.search(r"brax_(policy|episodes|episodes_stats)_kernel\s*<", rest), unit
        assert not re.search(r"\((true|false), \d+, (true|false), (true|false)\)", rest), unit
    src = U.source("carl_brax_policy.hip")  # the closed-loop unit instantiates nothing of the episodes mode
    assert "brax_episodes_kernel" not in src and "BraxEpisodesPolicy" not in src
    for unit in ("carl_brax_episodes.hip", "carl_brax_policy.hip", "carl_brax.hip"):
        src = U.source(unit)  # the other Brax units instantiate nothing of the statistics variant
        assert "brax_episodes_stats_kernel" not in src and "BraxStatsPolicy" not in src
    from carl_amd.build import SOURCES

    assert SOURCES["carl_brax_policy_stats.hip"] == SOURCES["carl_brax_episodes.hip"] == SOURCES["carl_brax_policy.hip"]


# (model, n_lanes, pinned width or 0, n_steps) -> (grid, wavefronts per workgroup, lanes per env); 256 compute units
# (what the query assumes without a device, and what an MI355X has).  Worked out from brax_launch.hpp's rule by hand for
# the first rows: 77 Ant envs unpinned widen to 16 lanes per env (fewer than 2048 groups) = 20 groups of 4 envs, one
# wavefront each, the smallest workgroup that reaches the most wavefronts per compute unit.
SHAPES = [
    ("ant", 77, 0, 12, 5, 4, 16),              # 20 groups of 4 envs
    ("ant", 77, 9, 12, 2, 9, 9),               # 11 groups of 7 envs; 15.3 KB per wavefront: nine per compute unit, one workgroup
    ("ant", 512, 9, 12, 9, 9, 9),              # 74 groups
    ("hopper", 77, 4, 12, 1, 5, 4),            # 5 groups of 16 envs: no empty wavefront
    ("inverted_pendulum", 77, 2, 12, 3, 1, 2),  # 3 groups of 32 envs
    ("reacher", 77, 8, 12, 5, 2, 8),           # 10 groups of 8 envs; the general kernels: eight wavefronts per compute unit
    ("ant", 32768, 9, 12, 256, 9, 9),          # 4 682 groups on 256 x 9 resident wavefronts: the balanced schedule
    ("halfcheetah", 32768, 7, 12, 256, 8, 7),
]


@pytest.mark.parametrize("model,n,width,T,grid,waves,k", SHAPES, ids=str)
def test_launch_shape_query(model, n, width, T, grid, waves, k):
    s = BP.build_model(model)[0]
    s.lanes_per_env = width
    code, sh = BP.launch_shape(_batch(n), s, _policy(s), T)
    assert code == 0 and (sh.grid, sh.waves_per_workgroup, sh.lanes_per_env) == (grid, waves, k)
    assert sh.lds_bytes % (16 * waves) == 0 and sh.lds_bytes + 16 * 1024 <= 160 * 1024
    n_groups = -(-n // (64 // k))
    frags = BP.fragments(sh, n, T)
    if n_groups <= grid * waves:  # a batch the chip holds at once: every group whole, in a wavefront of its own
        assert grid == -(-n_groups // waves)
        assert sorted(f[2] for f in frags) == list(range(n_groups))
        assert all((f[3], f[4], f[5], f[6]) == (0, T, 0, 0) for f in frags)
    else:  # every group-step once; a group split between two wavefronts is handed over
        steps = sorted((f[2], t) for f in frags for t in range(f[3], f[4]))
        assert steps == [(g, t) for g in range(n_groups) for t in range(T)]
        assert sum(f[5] for f in frags) == sum(f[6] for f in frags) > 0


# The launches of modes 0 and 1 -- carl_brax_reset (step 0) and carl_brax_step / carl_brax_rollout (step 1) -- as the
# commit before the shape rule moved to brax_launch.hpp launched them: recorded from its launch_brax, built for the host
# with the values it hands to the kernel launch read out, 256 compute units.  Every kernel class, batches below and above
# what the chip holds at once, launches shorter than the balanced schedule's 4 steps, pinned and free widths, the general
# substep (a planar model on the multi-hinge kernels) and the float32 classes.
A, GEN, F32 = _lib.FLAG_AUTORESET, _lib.FLAG_AUTORESET | _lib.FLAG_BRAX_GENERIC, _lib.FLAG_AUTORESET | _lib.FLAG_BRAX_FP32
OPEN_SHAPES = [
    # model, n_lanes, pinned width or 0, batch flags, step, n_steps -> lanes per env, wavefronts, grid, LDS bytes
    ("ant", 7, 9, A, 1, 12, 9, 1, 1, 11088),
    ("ant", 77, 0, A, 1, 12, 16, 3, 7, 19104),
    ("ant", 77, 9, A, 1, 12, 9, 11, 1, 121968),
    ("ant", 512, 9, A, 1, 12, 9, 12, 7, 133056),
    ("ant", 32768, 0, A, 1, 12, 9, 12, 256, 133056),
    ("ant", 32768, 9, A, 1, 12, 9, 12, 256, 133056),
    ("ant", 32768, 9, A, 1, 3, 9, 12, 391, 133056),
    ("ant", 32768, 16, A, 1, 1, 16, 3, 2731, 19104),
    ("ant", 12289, 16, A, 1, 6, 16, 12, 256, 76416),
    ("ant", 12289, 16, A, 1, 3, 16, 3, 1025, 19104),
    ("ant", 77, 0, A, 0, 0, 16, 3, 7, 19104),
    ("ant", 32768, 9, A, 0, 0, 9, 12, 391, 133056),
    ("ant", 32768, 9, F32, 1, 12, 9, 12, 256, 133056),
    ("one_leg_ant", 77, 4, A, 1, 12, 4, 5, 1, 53200),
    ("one_leg_ant", 32768, 7, A, 1, 12, 7, 4, 768, 24128),
    ("halfcheetah", 77, 0, A, 1, 12, 16, 2, 10, 9984),
    ("halfcheetah", 32768, 7, A, 1, 12, 7, 12, 256, 133632),
    ("halfcheetah", 32768, 7, A, 0, 0, 7, 12, 304, 133632),
    ("halfcheetah", 32768, 7, GEN, 1, 12, 11, 6, 512, 37344),
    ("halfcheetah", 32768, 7, F32, 1, 12, 7, 12, 256, 133632),
    ("hopper", 77, 4, A, 1, 12, 4, 5, 1, 62160),
    ("hopper", 32768, 0, A, 1, 12, 4, 11, 187, 136752),
    ("inverted_pendulum", 77, 2, A, 1, 12, 2, 2, 2, 28576),
    ("inverted_pendulum", 32768, 2, A, 1, 12, 2, 10, 103, 142880),
    ("inverted_double_pendulum", 77, 0, A, 1, 12, 16, 2, 10, 4992),
    ("inverted_double_pendulum", 32768, 11, A, 1, 12, 11, 6, 512, 18624),
    ("reacher", 77, 8, A, 1, 12, 8, 2, 5, 10080),
    ("reacher", 32768, 4, A, 1, 12, 4, 2, 1024, 20000),
    ("reacher", 77, 0, A, 0, 0, 16, 1, 20, 2560),
    ("humanoid", 77, 0, A, 1, 12, 16, 4, 5, 35072),
    ("humanoid", 4096, 0, A, 1, 12, 16, 4, 256, 35072),
    ("humanoid", 4096, 16, A, 0, 0, 16, 4, 256, 35072),
]
POLICY_ROWS = 32 + 2 * 64 + 4  # brax_kernels.hip.h: kPolicyRows, float rows per env behind the step's


@pytest.mark.parametrize("model,n,width,flags,step,T,k,waves,grid,lds", OPEN_SHAPES, ids=str)
def test_shapes_of_modes_0_and_1_are_unchanged(model, n, width, flags, step, T, k, waves, grid, lds):
    """carl_brax_launch_shape runs the function launch_brax<0 / 1> takes its launch from (carl_brax.hip: class_and_shape)"""
    s = BP.build_model(model)[0]
    s.lanes_per_env = width
    code, sh = BP.open_launch_shape(_batch(n, flags=flags), s, step, T)
    assert code == 0, _lib.load().carl_last_error()
    assert (sh.lanes_per_env, sh.waves_per_workgroup, sh.grid, sh.lds_bytes) == (k, waves, grid, lds)
    if step and flags == A and s.obs_dim + 2 <= 32:
        # the closed-loop launch of the same batch: the same width, and each wavefront's slice larger by exactly the
        # policy's rows (164 rows of `envs` floats: a multiple of 16 bytes, so the rounding of the slice does not move)
        code, pol = BP.launch_shape(_batch(n, flags=flags), s, _policy(s), T)
        assert code == 0 and pol.lanes_per_env == k
        envs = 64 // k
        assert pol.lds_bytes % pol.waves_per_workgroup == 0 and lds % waves == 0
        assert pol.lds_bytes // pol.waves_per_workgroup - lds // waves == POLICY_ROWS * envs * 4
        if pol.waves_per_workgroup == waves:  # (larger slices may pack a compute unit best at another workgroup size)
            assert pol.lds_bytes - lds == waves * POLICY_ROWS * envs * 4


def test_a_wavefront_per_group_hands_nothing_over():
    """a launch with at least as many wavefronts as groups (grid = ceil(groups / wavefronts per workgroup): what the shape
    rule gives a batch the chip holds at once) runs every group whole in a wavefront of its own -- for every workgroup
    size, every group count up to five workgroups and a spread of larger ones, and the step counts of the GPU tests"""
    lib = _lib.load()
    buf = (C.c_int32 * (5 * 8))()
    for waves in range(1, 13):
        for groups in [*range(1, 5 * waves + 1), 1000, 3071, 3072]:
            grid = -(-groups // waves)
            for steps in (1, 4, 6, 12):
                seen = []
                for wg in range(grid):
                    for wave in range(waves):
                        k = lib.carl_brax_fragment_plan(groups, grid, waves, steps, wg, wave, buf, 8)
                        assert k in (0, 1), (waves, groups, steps, wg, wave)
                        if k:
                            assert tuple(buf[1:5]) == (0, steps, 0, 0)
                            seen.append(buf[0])
                assert sorted(seen) == list(range(groups)), (waves, groups, steps)


def test_open_launch_shape_refusals():
    s = BP.build_model("reacher")[0]
    code, _ = BP.open_launch_shape(_batch(77, flags=F32), s, 1, 12)
    assert code == _lib.ERR_UNSUPPORTED and _lib.load().carl_last_error().startswith(
        b"carl_brax_launch_shape: CARL_FLAG_BRAX_FP32 is not built for the reach / push task models")
    assert BP.open_launch_shape(_batch(0), s, 1, 12)[0] == _lib.ERR_INVALID_ARGUMENT
    assert BP.open_launch_shape(_batch(77), s, 1, 0)[0] == _lib.ERR_INVALID_ARGUMENT
    assert BP.open_launch_shape(_batch(77, flags=F32), s, 0, 0)[0] == 0  # (a reset never takes the float32 classes)


def test_launch_shape_refusals_and_the_large_batch_schedule():
    s = BP.build_model("ant")[0]
    s.lanes_per_env = 16
    code, _ = BP.launch_shape(_batch(77, flags=_lib.FLAG_BRAX_FP32), s, _policy(s), 6)
    assert code == _lib.ERR_UNSUPPORTED and b"CARL_FLAG_BRAX_FP32" in _lib.load().carl_last_error()
    assert BP.launch_shape(_batch(0), s, _policy(s), 6)[0] == _lib.ERR_INVALID_ARGUMENT
    # more groups than 256 compute units hold: exactly the resident workgroups, fragments with hand-overs
    n = 4 * 3072 + 1
    code, sh = BP.launch_shape(_batch(n), s, _policy(s), 6)
    assert code == 0 and sh.lanes_per_env == 16 and sh.grid * sh.waves_per_workgroup <= 3072
    frags = BP.fragments(sh, n, 6)
    assert any(f[5] for f in frags) and sum(f[4] - f[3] for f in frags) == 3073 * 6
    # short launches keep one wavefront per group
    code, sh = BP.launch_shape(_batch(n), s, _policy(s), 3)
    assert code == 0 and sh.grid == -(-3073 // sh.waves_per_workgroup)


def test_python_refusals_before_any_launch():
    from carl_amd.brax_engine import BraxVecEngine

    eng = object.__new__(BraxVecEngine)
    eng.D, eng.sys = 27, BP.build_model("ant")[0]
    rng = np.random.default_rng(1)
    pol = BraxMLPPolicy(_info(11, 3), [], BP.make_layers(rng, 11, (8,), 3), "relu")
    with pytest.raises(ValueError, match="11 observations and 3 actuators"):
        eng.rollout_policy(pol, 4)
    pol = BraxMLPPolicy(_info(27, 8), [], BP.make_layers(rng, 27, (8,), 8), "relu")
    with pytest.raises(ValueError, match="mode 'episodes'"):
        eng.rollout_policy(pol, 4, mode="episodes")
