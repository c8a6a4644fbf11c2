"""The closed-loop rollout's host side: the packed parameter layout MLPPolicy produces, every refusal of
carl_rollout_policy's validation and of the Python constructors, and the ctypes layout of carl_policy_t.
CPU-only: nothing here launches a kernel (the C entry point refuses before it would enqueue anything)."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from carl_amd import _lib
from carl_amd.envs import CARLCartPole
from carl_amd.policy import MLPPolicy
from policy_cases import HEADER, REFUSALS, c_batch, c_io, c_policy, check_first_of_two, fake_engine, rand_layers

CP_NAMES = list(CARLCartPole.get_context_features())  # table order of the CartPole family


class FakeCARLEnv:
    """What MLPPolicy.for_env reads of a CARLEnv: its engine, table names and observation-context options."""

    def __init__(self, visible_names, as_dict):
        class _T:
            names = CP_NAMES

        self._table = _T()
        self.obs_context_as_dict = as_dict
        self.obs_context_features = list(visible_names)
        self.env = fake_engine(_lib.CARTPOLE, [CP_NAMES.index(n) for n in visible_names])


def expected_pack(layers, shift, scale, clip):
    flat = []
    for W, b in layers:
        flat += list(np.asarray(W, np.float32).reshape(-1)) + list(np.asarray(b, np.float32))
    flat += list(shift) + list(scale) + [clip]
    flat += [0.0] * ((-len(flat)) % 4)
    return np.asarray(flat, np.float32)


def test_for_env_packs_the_documented_layout_and_flatten_order():
    rng = np.random.default_rng(0)
    # dict mode: FlattenObservation sorts the context names; vector mode keeps obs_context_features order
    vis = ["masspole", "gravity", "length"]
    env_d, env_v = FakeCARLEnv(vis, True), FakeCARLEnv(vis, False)
    n_in = 3 + 4
    layers = rand_layers(rng, [n_in, 5, 3, 2])
    shift, scale = rng.normal(size=n_in).astype(np.float32), rng.uniform(0.5, 2, n_in).astype(np.float32)
    p = MLPPolicy.for_env(env_d, layers, "relu", input_shift=shift, input_scale=scale, input_clip=5.0)
    assert p.context_names == sorted(vis) and p.ctx_rows == [CP_NAMES.index(n) for n in sorted(vis)]
    q = MLPPolicy.for_env(env_v, layers, "relu", input_shift=shift, input_scale=scale, input_clip=5.0)
    assert q.context_names == vis and q.ctx_rows == [CP_NAMES.index(n) for n in vis]
    want = expected_pack(layers, shift, scale, 5.0)
    assert p.params.shape == (1, want.size) and np.array_equal(p.params[0], want)
    s = p.struct(1000)
    assert _lib.load().carl_policy_set_floats(C.byref(s)) == want.size
    assert (s.n_in, s.n_ctx, s.n_hidden, list(s.width), s.n_out) == (7, 3, 2, [5, 3], 2)
    assert s.activation == _lib.POLICY_RELU and s.head == _lib.POLICY_HEAD_ARGMAX and s.n_sets == 1
    assert s.lanes_per_set == 1024  # one set covers the batch, in whole workgroups
    # defaults: no transform (shift 0, scale 1, clip inf); [] context features: the observation only
    lin = MLPPolicy.for_env(env_d, [(np.ones((2, 4)), np.zeros(2))], context_features=[])
    assert lin.ctx_rows == [] and lin.n_in == 4
    assert np.array_equal(lin.params[0], expected_pack([(np.ones((2, 4)), np.zeros(2))], np.zeros(4), np.ones(4), np.inf))


def test_from_sequential_matches_for_env():
    torch.manual_seed(0)
    env = FakeCARLEnv(CP_NAMES, True)
    seq = torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.Tanh(), torch.nn.Linear(16, 8), torch.nn.Tanh(),
                              torch.nn.Linear(8, 2), torch.nn.Identity())
    p = MLPPolicy.from_sequential(env, seq)
    layers = [(m.weight.detach().numpy(), m.bias.detach().numpy()) for m in seq if isinstance(m, torch.nn.Linear)]
    assert p.activation == "tanh" and p.widths == [16, 8]
    assert np.array_equal(p.params[0], expected_pack(layers, np.zeros(12), np.ones(12), np.inf))
    # a Linear without bias packs zeros; consecutive Linears are identity-activated
    seq2 = torch.nn.Sequential(torch.nn.Linear(12, 4, bias=False), torch.nn.Linear(4, 2))
    p2 = MLPPolicy.from_sequential(env, seq2)
    assert p2.activation == "identity" and np.array_equal(p2.layers[0][1], np.zeros(4, np.float32))


def test_stack_concatenates_weight_sets():
    rng = np.random.default_rng(1)
    env = FakeCARLEnv(["gravity"], False)
    ps = [MLPPolicy.for_env(env, rand_layers(rng, [5, 8, 2])) for _ in range(3)]
    st = MLPPolicy.stack(ps, lanes_per_set=512)
    assert st.n_sets == 3 and np.array_equal(st.params, np.concatenate([p.params for p in ps]))
    s = st.struct(1536)
    assert (s.n_sets, s.lanes_per_set) == (3, 512)
    with pytest.raises(ValueError, match="multiple"):
        MLPPolicy.stack(ps, lanes_per_set=300)
    with pytest.raises(ValueError, match="same"):
        MLPPolicy.stack([ps[0], MLPPolicy.for_env(env, rand_layers(rng, [5, 4, 2]))], 256)


def test_python_refusals():
    rng = np.random.default_rng(2)
    env = FakeCARLEnv(["gravity", "length"], True)
    with pytest.raises(ValueError, match="not a visible context row"):
        MLPPolicy.for_env(env, rand_layers(rng, [5, 2]), context_features=["masscart"])
    with pytest.raises(ValueError, match="hidden widths"):
        MLPPolicy.for_env(env, rand_layers(rng, [6, 65, 2]))
    with pytest.raises(ValueError, match="hidden widths"):
        MLPPolicy.for_env(env, rand_layers(rng, [6, 4, 4, 4, 2]))
    with pytest.raises(ValueError, match="head width"):
        MLPPolicy.for_env(env, rand_layers(rng, [6, 3]))
    with pytest.raises(ValueError, match="do not continue"):
        MLPPolicy.for_env(env, rand_layers(rng, [7, 2]))
    with pytest.raises(TypeError, match="Linear / Tanh / ReLU / Identity"):
        MLPPolicy.from_sequential(env, torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Sigmoid(), torch.nn.Linear(4, 2)))
    with pytest.raises(ValueError, match="head"):
        MLPPolicy.from_sequential(env, torch.nn.Sequential(torch.nn.Linear(6, 2), torch.nn.Tanh()))
    with pytest.raises(ValueError, match="one kind"):
        MLPPolicy.from_sequential(env, torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Tanh(), torch.nn.Linear(4, 4),
                                                           torch.nn.ReLU(), torch.nn.Linear(4, 2)))
    # engines out of scope
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.mixed import MixedVecEngine

    with pytest.raises(TypeError, match="classic-control"):
        MLPPolicy.for_env(object.__new__(BraxVecEngine), rand_layers(rng, [4, 2]))
    with pytest.raises(TypeError, match="out of scope"):
        MLPPolicy.for_env(object.__new__(MixedVecEngine), rand_layers(rng, [4, 2]))
    with pytest.raises(NotImplementedError):
        object.__new__(MixedVecEngine).rollout_policy(None, 1)
    # a bare engine: context inputs are table rows, refused unless visible
    eng = fake_engine(_lib.CARTPOLE, [0, 3])
    assert MLPPolicy.for_env(eng, rand_layers(rng, [6, 2])).ctx_rows == [0, 3]
    with pytest.raises(ValueError, match="visible"):
        MLPPolicy.for_env(eng, rand_layers(rng, [5, 2]), context_features=[5])


@pytest.mark.parametrize("case, batch_kw, pol_kw, msg", [
    ("width over the limit", {}, {"width": (65, 64)}, b"hidden width[0] = 65"),
    ("width zero", {}, {"width": (64, 0)}, b"hidden width[1] = 0"),
    ("too many layers", {}, {"n_hidden": 3}, b"n_hidden 3"),
    ("discrete head width", {}, {"n_out": 3}, b"head width 3"),
    ("Box head width", {"family": _lib.PENDULUM}, {"n_in": 5, "n_out": 2, "head": _lib.POLICY_HEAD_BOX}, b"head width 2"),
    ("Brax family", {"family": _lib.CARL_N_FAMILIES}, {}, b"Brax family"),
    ("lanes_per_set not a multiple", {}, {"lanes_per_set": 300}, b"lanes_per_set 300"),
    ("lanes_per_set zero", {}, {"lanes_per_set": 0}, b"lanes_per_set 0"),
    ("sets do not cover", {}, {"lanes_per_set": 256, "n_sets": 3}, b"do not cover"),
    ("context row >= F", {}, {"ctx_rows": (0, 8)}, b"ctx_rows[1] = 8"),
    ("context row < 0", {}, {"ctx_rows": (-1, 0)}, b"ctx_rows[0] = -1"),
    ("n_in mismatch", {}, {"n_in": 7}, b"n_in 7"),
    ("head kind", {}, {"head": _lib.POLICY_HEAD_BOX}, b"head kind"),
    ("activation", {}, {"activation": 7}, b"unknown activation"),
    ("no params", {}, {"params": None}, b"params is NULL"),
    # the batch checks are carl_rollout's: a context observation feature outside the context table
    ("context observation feature >= F", {"n_ctx_obs": 1, "ctx_obs": 0x4000, "ctx_obs_feat": (8,)}, {},
     b"ctx_obs_feat[0] = 8"),
])
def test_c_entry_point_refuses(case, batch_kw, pol_kw, msg):
    lib = _lib.load()
    b, p = c_batch(**batch_kw), c_policy(**pol_kw)
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), None, 10, C.byref(summ), None) == _lib.ERR_INVALID_ARGUMENT, case
    assert msg in lib.carl_last_error(), (case, lib.carl_last_error())
    assert lib.carl_last_error() == b"carl_rollout_policy: " + REFUSALS[case]


def test_c_entry_point_reports_the_earlier_of_two_bad_arguments():
    """the batch / policy checks in their order, and all of them before n_steps, io and the summary"""
    lib = _lib.load()
    for io in (None, c_io(action_dtype=_lib.ACTION_I64)):
        check_first_of_two(b"carl_rollout_policy", lambda b, p: lib.carl_rollout_policy(
            C.byref(b), C.byref(p), None if io is None else C.byref(io), -1, None, None))
    assert lib.carl_rollout_policy(None, C.byref(c_policy(params=None)), None, -1, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == b"carl_rollout_policy: batch / policy is NULL"
    assert lib.carl_rollout_policy(C.byref(c_batch(family=_lib.CARL_N_FAMILIES)), None, None, -1, None, None) == -1
    assert lib.carl_last_error() == b"carl_rollout_policy: batch / policy is NULL"
    # past the shared checks: n_steps before the summary, the io before the auto-reset a summary needs
    b, p = c_batch(), c_policy()
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), None, -1, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.carl_last_error() == b"carl_rollout_policy: n_steps -1 < 0"
    summ = _lib.PolicySummary(0x3000, 0x3000, 0x3000)
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), C.byref(c_io(row_pitch=999)), 10, C.byref(summ), None) == -1
    assert lib.carl_last_error() == b"carl_rollout_policy: io.row_pitch 999 < n_lanes 1000"


def test_c_entry_point_refuses_bad_io_and_summary():
    lib = _lib.load()
    b, p = c_batch(), c_policy()
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), None, 10, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"summary" in lib.carl_last_error()
    io = _lib.StepIO()
    io.action, io.obs, io.reward, io.terminated, io.truncated = 0x1000, 0x1000, 0x1000, 0x1000, 0x1000
    io.action_dtype = _lib.ACTION_I64
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), C.byref(io), 10, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"int32" in lib.carl_last_error()
    io.action_dtype, io.row_pitch = _lib.ACTION_I32, 1004  # not a multiple of 16: not the staged layout
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), C.byref(io), 10, None, None) == _lib.ERR_UNSUPPORTED
    assert lib.carl_rollout_policy(C.byref(b), C.byref(p), None, -1, C.byref(_lib.PolicySummary(1, 1, 1)), None) == -1
    assert lib.carl_policy_lane_quantum() == 256
    assert lib.carl_policy_set_floats(C.byref(c_policy(width=(65, 1)))) == -1
    # 6 -> 64 -> 64 -> 2: 6*64 + 64 + 64*64 + 64 + 64*2 + 2 + 6 + 6 + 1 = 4751 -> 4752
    assert lib.carl_policy_set_floats(C.byref(c_policy())) == 4752


def test_policy_struct_layout_matches_c(tmp_path):
    """sizeof / offsetof of carl_policy_t and carl_policy_summary_t from C compiled against the header"""
    prog = tmp_path / "layout.c"
    fp = [f[0] for f in _lib.Policy._fields_]
    fs = [f[0] for f in _lib.PolicySummary._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("%zu %zu\\n", sizeof(carl_policy_t), sizeof(carl_policy_summary_t));']
    lines += [f'printf("%zu\\n", offsetof(carl_policy_t, {f}));' for f in fp]
    lines += [f'printf("%zu\\n", offsetof(carl_policy_summary_t, {f}));' for f in fs]
    lines += ['printf("%d %d %d %d %d %d\\n", CARL_POLICY_MAX_IN, CARL_POLICY_MAX_HIDDEN, CARL_POLICY_MAX_WIDTH, '
              'CARL_POLICY_TANH, CARL_POLICY_RELU, CARL_POLICY_HEAD_BOX);', "return 0;}"]
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out[:2] == [C.sizeof(_lib.Policy), C.sizeof(_lib.PolicySummary)]
    assert out[2:-6] == [getattr(_lib.Policy, f).offset for f in fp] + [getattr(_lib.PolicySummary, f).offset for f in fs]
    assert out[-6:] == [_lib.POLICY_MAX_IN, _lib.POLICY_MAX_HIDDEN, _lib.POLICY_MAX_WIDTH, _lib.POLICY_TANH,
                        _lib.POLICY_RELU, _lib.POLICY_HEAD_BOX]
