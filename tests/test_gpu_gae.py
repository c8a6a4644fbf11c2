"""carl_gae on the GPU (VecEngine.gae) bit for bit against its host restatement (value_cases.gae_ref: the same fp32
operations with a correctly rounded fma), over flag patterns, shapes and layouts, and with NaNs in masked-out inputs."""
import numpy as np
import pytest
import torch

import value_cases as VC
from carl_amd import _lib
from policy_cases import make_engine

pytestmark = pytest.mark.gpu

FILL = 0x4B1D4B1D


@pytest.fixture(scope="module")
def eng():
    return make_engine(_lib.PENDULUM, 16)


def run(eng, d, gamma, lam, boot, pitch=None):
    """the device's (advantage, ret) for host arrays d; pitch: rows of that many lanes inside canary-filled arrays"""
    T, N = d["reward"].shape
    P = N if pitch is None else pitch
    full = {}

    def dev(k, a):
        if a.ndim == 1:
            return torch.as_tensor(a).to(eng.device)
        t = torch.zeros((T + 2, P), dtype=torch.as_tensor(a).dtype, device=eng.device)
        t[:T, :N] = torch.as_tensor(a).to(eng.device)
        return t[:T, :N]

    args = {k: dev(k, v) for k, v in d.items()}
    for k in ("advantage", "return"):
        full[k] = torch.full((T + 2, P + 8), FILL, dtype=torch.int32, device=eng.device).view(torch.float32)
    out = {k: v.view(-1)[: (T + 2) * P].view(T + 2, P)[:T, :N] for k, v in full.items()}
    res = eng.gae(args["reward"], args["value"], args["terminated"], args["truncated"], args["last_value"], gamma, lam,
                  boot_value=args["boot_value"] if boot else None, out=out)
    torch.cuda.synchronize()
    for k, v in full.items():  # nothing beyond column N - 1 of a row, nothing in a padding row
        rows = v.view(-1)[: (T + 2) * P].view(T + 2, P).view(torch.int32)
        assert bool((rows[:T, N:] == FILL).all()) and bool((rows[T:] == FILL).all()), k
        assert bool((v.view(-1)[(T + 2) * P:].view(torch.int32) == FILL).all()), k
        assert not bool((rows[:T, :N] == FILL).any()), k
    return res["advantage"].cpu().numpy(), res["return"].cpu().numpy()


def check(eng, d, gamma=0.99, lam=0.95, boot=True, pitch=None):
    adv, ret = run(eng, d, gamma, lam, boot, pitch)
    a, r = VC.gae_ref(d["reward"], d["value"], d["terminated"], d["truncated"], d["last_value"], gamma, lam,
                      boot_value=d["boot_value"] if boot else None)
    np.testing.assert_array_equal(adv.view(np.int32), a.view(np.int32))
    np.testing.assert_array_equal(ret.view(np.int32), r.view(np.int32))
    return adv, ret


@pytest.mark.parametrize("boot", [False, True])
@pytest.mark.parametrize("T,N,pitch", [(19, 263, 272), (43, 256, None), (1, 263, 272), (8, 256, None), (9, 70, 80)])
def test_random_inputs(eng, T, N, pitch, boot):
    d = VC.random_gae_inputs(np.random.default_rng(T * N + boot), T, N)
    if T > 1:
        assert (d["terminated"] & d["truncated"]).any() and (d["truncated"] & ~d["terminated"]).any()
    check(eng, d, boot=boot, pitch=pitch)
    check(eng, d, gamma=1.0, lam=0.0, boot=boot, pitch=pitch)


@pytest.mark.parametrize("pattern", ["never", "always", "last_only", "both_flags"])
def test_flag_patterns(eng, pattern):
    T, N = 19, 263
    d = VC.random_gae_inputs(np.random.default_rng(3), T, N)
    te, tr = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
    if pattern == "always":
        te[:, ::2] = 1
        tr[:, 1::2] = 1
    elif pattern == "last_only":
        tr[T - 1] = 1
    elif pattern == "both_flags":
        te[::3] = tr[::3] = 1
    d["terminated"], d["truncated"] = te, tr
    check(eng, d, boot=True, pitch=272)
    check(eng, d, boot=False, pitch=272)


def test_bool_flags_are_accepted(eng):
    d = VC.random_gae_inputs(np.random.default_rng(4), 5, 32)
    want = check(eng, d)
    a = {k: torch.as_tensor(v).to(eng.device) for k, v in d.items()}
    res = eng.gae(a["reward"], a["value"], a["terminated"].bool(), a["truncated"].bool(), a["last_value"], 0.99, 0.95,
                  boot_value=a["boot_value"])
    np.testing.assert_array_equal(res["advantage"].cpu().numpy().view(np.int32), want[0].view(np.int32))
    with pytest.raises(ValueError, match="gae 'value'"):
        eng.gae(a["reward"], a["value"].double(), a["terminated"], a["truncated"], a["last_value"], 0.99, 0.95)


def test_masked_out_nan_changes_nothing(eng):
    T, N = 11, 70
    d = VC.random_gae_inputs(np.random.default_rng(5), T, N, p_te=0.2, p_tr=0.2)
    base = check(eng, d, pitch=80)
    te, tr = d["terminated"].astype(bool), d["truncated"].astype(bool)
    p = {k: v.copy() for k, v in d.items()}
    not_cut = ~(tr & ~te)
    assert not_cut.any() and (te | tr)[:-1].any()
    p["boot_value"][not_cut] = np.nan  # a boot_value of a step that is not truncated only is never read
    got = run(eng, p, 0.99, 0.95, True, 80)
    for x, y in zip(base, got):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
    # value[t + 1] after a done step t is masked out of step t; it is still step t + 1's own value, so that one entry
    # (and no other: the walk reaches t + 1 before t, and t cuts the recurrence) becomes NaN
    t, lane = map(int, np.argwhere((te | tr)[:-1])[0])
    p = {k: v.copy() for k, v in d.items()}
    p["value"][t + 1, lane] = np.nan
    got = run(eng, p, 0.99, 0.95, True, 80)
    keep = np.ones((T, N), bool)
    keep[t + 1, lane] = False
    for x, y in zip(base, got):
        np.testing.assert_array_equal(x[keep].view(np.int32), y[keep].view(np.int32))
        assert np.isnan(y[t + 1, lane])
