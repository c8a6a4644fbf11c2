"""PPO's minibatch step, C ABI on the host: every refusal of carl_ppo_adv_stats and carl_adam_step by its message (both
are validated before anything is enqueued, so they run without a GPU), the row count and the element limit, the struct
bindings against a C program compiled with the header, carl_amd.PPO's ``fused_step`` argument and the engine methods'
checks as far as they come before a launch.  CPU-only."""
import ctypes as C
import inspect
import subprocess

import numpy as np
import pytest
import torch

import brax_policy_abi_util as U
import policy_cases as PC
from carl_amd import PPO, _lib
from carl_amd.policy import MLPPolicy
from policy_cases import HEADER

PTR = 0x10000  # a "device pointer" that is never dereferenced: every call here is refused first
ADV, ADAM = b"carl_ppo_adv_stats: ", b"carl_adam_step: "
INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("cls,name", [(_lib.PpoAdvStats, "carl_ppo_adv_stats_t"), (_lib.Adam, "carl_adam_t")])
def test_struct_layout_matches_c(tmp_path, cls, name):
    fs = [f[0] for f in cls._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             f'printf("%zu\\n", sizeof({name}));']
    lines += [f'printf("%zu\\n", offsetof({name}, {f}));' for f in fs]
    lines += ['printf("%d\\n", CARL_ADAM_MAX_TENSORS);', "return 0;}"]
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fs] + [_lib.ADAM_MAX_TENSORS]
    assert _lib.load().carl_abi_version() == _lib.CARL_ABI_VERSION == 9  # additive


def test_row_count_and_element_limit():
    lib = _lib.load()
    f = lib.carl_ppo_adv_stats_rows
    assert [f(0, 4), f(-1, 4), f(4, 0), f(4, -3)] == [0, 0, 0, 0]
    assert [f(1, 1), f(2, 1), f(2, 2), f(255, 256), f(257, 256), f(1000, 300), f(4099, 1024), f(2 ** 31 - 1, 1),
            f(2 ** 31 - 1, 2 ** 31 - 1)] == [1, 2, 1, 1, 2, 4, 5, 2 ** 31 - 1, 1]
    most = lib.carl_adam_step_max_floats()
    assert most >= 20000 and most % 1024 == 0  # two packed 2 x 64 networks and log_std; whole passes of the workgroup


# ---------------------------------------------------------------- carl_ppo_adv_stats
def adv_args(**kw):
    a = _lib.PpoAdvStats(PTR, PTR, PTR, 4096, 1000, 300, 1e-8)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ADV_REFUSALS = [
    (dict(advantage=None), b"advantage, idx and adv_norm are required"),
    (dict(idx=None), b"advantage, idx and adv_norm are required"),
    (dict(adv_norm=None), b"advantage, idx and adv_norm are required"),
    (dict(n_total=0), b"n_total 0 < 1 or batch_size 300 < 1"),
    (dict(n_total=-5), b"n_total -5 < 1 or batch_size 300 < 1"),
    (dict(batch_size=0), b"n_total 1000 < 1 or batch_size 0 < 1"),
    (dict(storage_floats=0), b"storage_floats 0 < 1"),
    (dict(storage_floats=-1), b"storage_floats -1 < 1"),
    (dict(eps=-1e-8), b"eps -1e-08 is not finite and >= 0"),
    (dict(eps=INF), b"eps inf is not finite and >= 0"),
    (dict(eps=NAN), b"eps nan is not finite and >= 0"),
]


@pytest.mark.parametrize("kw,msg", ADV_REFUSALS, ids=[str(i) for i in range(len(ADV_REFUSALS))])
def test_adv_stats_refusals(kw, msg):
    U.refused(ADV, _lib.load().carl_ppo_adv_stats(C.byref(adv_args(**kw)), None), msg)


def test_adv_stats_null_struct():
    U.refused(ADV, _lib.load().carl_ppo_adv_stats(None, None), b"the argument struct is NULL")


# ---------------------------------------------------------------- carl_adam_step
def adam_args(n=(100, 50, 1), null=(), **kw):
    a = _lib.Adam()
    a.n_tensors = len(n)
    for i, k in enumerate(n):
        a.n[i] = k
        for f in ("param", "grad", "m", "v"):
            getattr(a, f)[i] = None if (f, i) in null else PTR
    a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm = 3e-4, 0.9, 0.999, 1e-5, 0.5
    a.step, a.beta_pow, a.norm_out = PTR, PTR, None
    for k, v in kw.items():
        setattr(a, k, v)
    return a


MOST = 1 << 18
ADAM_REFUSALS = [
    (dict(n_tensors=0), b"n_tensors 0 outside [1, 4]"),
    (dict(n_tensors=5), b"n_tensors 5 outside [1, 4]"),
    (dict(n=(100, -1)), b"n[1] = -1 < 0"),
    (dict(n=(MOST, 1)), b"more than 262144 elements in all (carl_adam_step_max_floats)"),
    (dict(n=(MOST + 1,)), b"more than 262144 elements in all (carl_adam_step_max_floats)"),
    (dict(n=(2 ** 62, 2 ** 62, 2 ** 62, 2 ** 62)), b"more than 262144 elements in all (carl_adam_step_max_floats)"),
    (dict(null=(("param", 0),)), b"param, grad, m and v of tensor 0 are required"),
    (dict(null=(("grad", 1),)), b"param, grad, m and v of tensor 1 are required"),
    (dict(null=(("m", 2),)), b"param, grad, m and v of tensor 2 are required"),
    (dict(null=(("v", 2),)), b"param, grad, m and v of tensor 2 are required"),
    (dict(step=None), b"step and beta_pow are required"),
    (dict(beta_pow=None), b"step and beta_pow are required"),
    (dict(lr=-1e-3), b"lr -0.001 is not finite and >= 0"),
    (dict(lr=INF), b"lr inf is not finite and >= 0"),
    (dict(lr=NAN), b"lr nan is not finite and >= 0"),
    (dict(eps=0.0), b"eps 0 is not finite and > 0"),
    (dict(eps=-1e-5), b"eps -1e-05 is not finite and > 0"),
    (dict(eps=INF), b"eps inf is not finite and > 0"),
    (dict(beta1=1.0), b"beta1 1 / beta2 0.999 outside [0, 1)"),
    (dict(beta1=-0.1), b"beta1 -0.1 / beta2 0.999 outside [0, 1)"),
    (dict(beta2=1.5), b"beta1 0.9 / beta2 1.5 outside [0, 1)"),
    (dict(beta2=NAN), b"beta1 0.9 / beta2 nan outside [0, 1)"),
    (dict(beta1=INF), b"beta1 inf / beta2 0.999 outside [0, 1)"),
    (dict(max_grad_norm=-0.5), b"max_grad_norm -0.5 is negative or NaN (+inf: no clip)"),
    (dict(max_grad_norm=NAN), b"max_grad_norm nan is negative or NaN (+inf: no clip)"),
]


@pytest.mark.parametrize("kw,msg", ADAM_REFUSALS, ids=[str(i) for i in range(len(ADAM_REFUSALS))])
def test_adam_step_refusals(kw, msg):
    U.refused(ADAM, _lib.load().carl_adam_step(C.byref(adam_args(**kw)), None), msg)


def test_adam_step_null_struct_and_nothing_to_do():
    lib = _lib.load()
    U.refused(ADAM, lib.carl_adam_step(None, None), b"the argument struct is NULL")
    assert lib.carl_adam_step(C.byref(adam_args(n=(0, 0), max_grad_norm=INF, norm_out=PTR)), None) == 0  # nothing is enqueued
    assert lib.carl_adam_step(C.byref(adam_args(n=(0,), max_grad_norm=0.0, lr=0.0, beta1=0.0, beta2=0.0)), None) == 0


# ---------------------------------------------------------------- carl_amd.PPO and the engine methods, before a launch
def host_networks():
    eng = PC.fake_engine(_lib.CARTPOLE)
    eng.b = _lib.Batch()
    eng.b.flags = _lib.FLAG_AUTORESET
    eng.device, eng.lib = torch.device("cpu"), _lib.load()
    rng = np.random.default_rng(0)
    actor = MLPPolicy.for_env(eng, PC.rand_layers(rng, [eng.F + 4, 8, 2]))
    critic = MLPPolicy.for_env(eng, PC.rand_layers(rng, [eng.F + 4, 8, 1]), head="value")
    return eng, actor, critic


def test_ppo_takes_fused_step_off_by_default():
    p = inspect.signature(PPO.__init__).parameters
    assert p["fused_step"].default is False
    eng, actor, critic = host_networks()
    for kw, msg in ((dict(lr=-1e-3), "fused_step: lr"), (dict(lr=NAN), "fused_step: lr"), (dict(lr=INF), "fused_step: lr"),
                    (dict(max_grad_norm=-1.0), "fused_step: max_grad_norm"), (dict(max_grad_norm=NAN), "fused_step: max_grad_norm")):
        with pytest.raises(ValueError, match=msg):
            PPO(eng, actor, critic, n_steps=4, fused_step=True, **kw)


def test_engine_methods_check_their_tensors_before_the_launch():
    eng, _, _ = host_networks()
    f32, i32, f64 = torch.float32, torch.int32, torch.float64
    adv, idx = torch.zeros(4, 10), torch.zeros(12, dtype=i32)
    for a, i, kw, msg in ((adv.double(), idx, {}, "'advantage'"), (adv.t(), idx, {}, "'advantage'"),
                          (torch.zeros(8)[::2], idx, {}, "'advantage'"), (adv, idx.long(), {}, "'idx'"),
                          (adv, idx[::2], {}, "'idx'"), (adv, idx[:0], {}, "'idx'"), (adv, idx, dict(batch_size=0), "batch_size 0 < 1"),
                          (adv, idx, dict(out=torch.zeros(2, 2)), r"'out'.*\[3, 2\]"),
                          (adv, idx, dict(out=torch.zeros(3, 2, dtype=f64)), "'out'")):
        with pytest.raises(ValueError, match=msg):
            eng.ppo_adv_stats(a, i, **{"batch_size": 5, **kw})
    st = eng.adam_state([torch.zeros(3), torch.zeros(2, 2)])
    assert [tuple(t.shape) for t in st["m"] + st["v"]] == [(3,), (2, 2)] * 2 and st["step"].dtype == torch.int64
    assert st["step"].item() == 0 and st["beta_pow"].tolist() == [1.0, 1.0] and st["beta_pow"].dtype == f64
    p, g = [torch.zeros(3), torch.zeros(2, 2)], [torch.zeros(3), torch.zeros(4)]
    bad = [
        (([], [], st), {}, "0 tensors"),
        ((p * 3, g * 3, st), {}, "6 tensors"),
        ((p, g[:1], st), {}, "need 2 gradients"),
        ((p, [g[0], torch.zeros(5)], st), {}, r"grads\[1\].*4 elements"),
        ((p, [g[0].double(), g[1]], st), {}, r"grads\[0\]"),
        (([torch.zeros(6)[::2], p[1]], g, st), {}, r"params\[0\]"),
        ((p, g, {**st, "m": [st["m"][0], torch.zeros(3)]}), {}, r"state\['m'\]\[1\]"),
        ((p, g, {**st, "step": torch.zeros(1, dtype=i32)}), {}, r"state\['step'\]"),
        ((p, g, {**st, "beta_pow": torch.ones(2, dtype=f32)}), {}, r"state\['beta_pow'\]"),
        ((p, g, st), dict(norm_out=torch.zeros(2, dtype=f32)), "'norm_out'"),
    ]
    for args, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            eng.adam_step(*args, lr=3e-4, **kw)
