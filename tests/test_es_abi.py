"""Evolution strategies, C ABI and Python layer on the host: the carl_es_t layout, every refusal of carl_es_perturb /
carl_es_gradient (validated before anything is enqueued, so they run without a GPU), MLPPolicy.on_device's refusals and
the public size properties.  CPU-only."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from carl_amd import _lib
from carl_amd.policy import MLPPolicy
from policy_cases import HEADER, HIDDEN_SHAPES, fake_engine, rand_layers

PTR = 0x10000  # a 16-byte-aligned "device pointer" that is never dereferenced: every call here is refused first


def es_struct(**kw):
    es = _lib.Es()
    es.seed, es.generation, es.n_pairs, es.set_floats, es.n_noisy, es.sigma = 1, 0, 2, 28, 26, 0.1
    for k, v in kw.items():
        setattr(es, k, v)
    return es


def test_es_struct_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    fs = [f[0] for f in _lib.Es._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("%zu\\n", sizeof(carl_es_t));']
    lines += [f'printf("%zu\\n", offsetof(carl_es_t, {f}));' for f in fs]
    lines += ["return 0;}"]
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(prog)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert out == [C.sizeof(_lib.Es)] + [getattr(_lib.Es, f).offset for f in fs]


BAD_STRUCTS = [
    (dict(n_pairs=0), b"n_pairs 0 < 1"),
    (dict(n_pairs=-3), b"n_pairs -3 < 1"),
    (dict(set_floats=0), b"set_floats 0 is not a positive multiple of 4"),
    (dict(set_floats=-4), b"set_floats -4 is not a positive multiple of 4"),
    (dict(set_floats=30), b"set_floats 30 is not a positive multiple of 4"),
    (dict(n_noisy=0), b"n_noisy 0 outside [1, set_floats = 28]"),
    (dict(n_noisy=29), b"n_noisy 29 outside [1, set_floats = 28]"),
    (dict(sigma=0.0), b"sigma 0 is not finite and positive"),
    (dict(sigma=-0.5), b"sigma -0.5 is not finite and positive"),
    (dict(sigma=float("inf")), b"sigma inf is not finite and positive"),
    (dict(sigma=float("nan")), b"is not finite and positive"),
    (dict(n_pairs=1 << 20, set_floats=1024, n_noisy=1000), b"more than 2^31 - 1 parameters"),
]


@pytest.mark.parametrize("spoil,msg", BAD_STRUCTS, ids=[str(i) for i in range(len(BAD_STRUCTS))])
def test_es_entry_points_refuse_a_bad_struct(spoil, msg):
    lib = _lib.load()
    es = es_struct(**spoil)
    assert lib.carl_es_perturb(C.byref(es), PTR, PTR, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"carl_es_perturb" in lib.carl_last_error() and msg in lib.carl_last_error()
    assert lib.carl_es_gradient(C.byref(es), PTR, PTR, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"carl_es_gradient" in lib.carl_last_error() and msg in lib.carl_last_error()


def test_es_entry_points_refuse_bad_pointers():
    lib = _lib.load()
    es = es_struct()
    assert lib.carl_es_perturb(None, PTR, PTR, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"carl_es_perturb: es is NULL" in lib.carl_last_error()
    assert lib.carl_es_perturb(C.byref(es), None, PTR, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"carl_es_perturb: center is NULL" in lib.carl_last_error()
    assert lib.carl_es_perturb(C.byref(es), PTR, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"carl_es_perturb: params is NULL" in lib.carl_last_error()
    for off in (4, 8, 12):
        assert lib.carl_es_perturb(C.byref(es), PTR, PTR + off, None, None) == _lib.ERR_INVALID_ARGUMENT
        assert b"carl_es_perturb: params is not on a 16-byte boundary" in lib.carl_last_error()
    assert lib.carl_es_gradient(None, PTR, PTR, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"carl_es_gradient: es is NULL" in lib.carl_last_error()
    assert lib.carl_es_gradient(C.byref(es), None, PTR, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"carl_es_gradient: weight is NULL" in lib.carl_last_error()
    assert lib.carl_es_gradient(C.byref(es), PTR, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"carl_es_gradient: grad is NULL" in lib.carl_last_error()
    # the largest population below the limit passes the size check (and is refused for the next reason)
    ok = es_struct(n_pairs=(1 << 20) - 1, set_floats=1024, n_noisy=1000)
    assert lib.carl_es_perturb(C.byref(ok), None, PTR, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"center is NULL" in lib.carl_last_error()


def test_slice_pairs_query():
    assert _lib.load().carl_es_slice_pairs() >= 1


def _template(widths=(), family=_lib.CARTPOLE):
    eng = fake_engine(family)
    n_out = int(eng.info.n_actions) if eng.info.action_is_discrete else 1
    dims = [eng.F + eng.D, *widths, n_out]
    return MLPPolicy.for_env(eng, rand_layers(np.random.default_rng(0), dims), "tanh")


@pytest.mark.parametrize("widths", [()] + HIDDEN_SHAPES, ids=str)
def test_public_sizes_agree_with_the_library(widths):
    pol = _template(widths)
    want = _lib.load().carl_policy_set_floats(C.byref(pol.struct(1000)))
    assert pol.set_floats == want == pol.params.shape[1] and want % 4 == 0
    assert pol.weight_floats == sum(W.size + b.size for W, b in pol.layers)
    assert pol.weight_floats + 2 * pol.n_in + 1 <= pol.set_floats < pol.weight_floats + 2 * pol.n_in + 1 + 4
    # unpack() is the inverse of the packing, bit for bit
    flat = np.random.default_rng(1).normal(size=pol.set_floats).astype(np.float32)
    flat[pol.weight_floats + 2 * pol.n_in + 1:] = 0
    back = MLPPolicy.unpack(pol, flat)
    np.testing.assert_array_equal(back.params[0].view(np.uint32), flat.view(np.uint32))
    assert back.n_sets == 1 and [W.shape for W, _ in back.layers] == [W.shape for W, _ in pol.layers]


def test_on_device_refusals():
    pol = _template((33, 7))
    S = pol.set_floats
    good = torch.zeros((4, S), dtype=torch.float32)
    with pytest.raises(ValueError, match=r"is not \[n_sets, %d\]" % S):
        MLPPolicy.on_device(pol, torch.zeros((4, S + 4)), 256)
    with pytest.raises(ValueError, match=r"is not \[n_sets"):
        MLPPolicy.on_device(pol, torch.zeros(4 * S), 256)
    with pytest.raises(ValueError, match="torch.float32"):
        MLPPolicy.on_device(pol, good.double(), 256)
    with pytest.raises(ValueError, match="contiguous"):
        MLPPolicy.on_device(pol, torch.zeros((4, 2 * S))[:, ::2], 256)
    with pytest.raises(ValueError, match="must live on a GPU"):
        MLPPolicy.on_device(pol, good, 256)
    with pytest.raises(ValueError, match="torch tensor"):
        MLPPolicy.on_device(pol, good.numpy(), 256)
    two = MLPPolicy.stack([pol, pol], 256)
    with pytest.raises(ValueError, match="one-set"):
        MLPPolicy.on_device(two, good, 256)
    with pytest.raises(ValueError, match="one-set"):
        MLPPolicy.unpack(two, np.zeros(S, np.float32))
    with pytest.raises(ValueError, match="floats"):
        MLPPolicy.unpack(pol, np.zeros(S + 4, np.float32))
