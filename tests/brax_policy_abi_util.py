"""What the host-side tests of the Brax closed-loop entry points share (test_brax_policy_abi.py, test_brax_episodes_abi.py,
test_brax_stats_abi.py): C structs with fake device pointers -- nothing is enqueued --, the refusal check, fake engines and
templates for the Python-side refusals, and the reader of the sources the table tests parse."""
import os
import re

import torch

import brax_policy_cases as BP
from carl_amd import _lib
from carl_amd.brax_engine import _BRAX_FAMILY, BraxVecEngine, _BraxInfo
from carl_amd.brax_policy import BraxMLPPolicy
from policy_cases import c_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch(n=1000, **kw):
    kw.setdefault("n_ctx_obs", 2)
    kw.setdefault("ctx_obs_feat", (0, 1))
    kw.setdefault("flags", _lib.FLAG_AUTORESET)
    return c_batch(family=_BRAX_FAMILY, n=n, **kw)


def policy(s, **kw):
    """a valid carl_policy_t for batch() and model `s` (2 context inputs, 2 x 64 tanh), kw: the fields to spoil"""
    p = _lib.Policy()
    p.n_ctx, p.n_hidden, p.n_out = 2, 2, s.n_act
    p.n_in = 2 + s.obs_dim
    p.ctx_rows[0], p.ctx_rows[1] = 0, 1
    p.width[0], p.width[1] = 64, 64
    p.activation, p.head, p.n_sets, p.lanes_per_set, p.params = _lib.POLICY_TANH, _lib.POLICY_HEAD_BOX, 1, 1024, 0x2000
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def episodes_out(**kw):
    out = _lib.PolicyEpisodes(0x3000, 0x3000, 0x3000, 0x3000, 0x3000, 0x3000)
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def refused(who, code, msg, want=_lib.ERR_INVALID_ARGUMENT):
    """the call returned `want` (None: any error code) and left the entry point's prefix `who` + msg as the last error"""
    err = _lib.load().carl_last_error()
    assert (code != 0 if want is None else code == want) and err == who + msg, (code, err)


def info(obs_dim, n_act, n_features=8):
    return _BraxInfo(0, obs_dim, n_features, n_act, 0, 0, 1000, -1.0, 1.0)


def ant_policy(rng, widths=(8,), rows=()):
    return BraxMLPPolicy(info(27, 8), list(rows), BP.make_layers(rng, 27 + len(rows), widths, 8), "relu")


def fake_brax_engine(auto_reset=True, n=1024):
    eng = object.__new__(BraxVecEngine)
    eng.b = _lib.Batch()  # (auto_reset is a flag of the batch)
    eng.D, eng.sys, eng.n, eng.auto_reset, eng.device = 27, BP.build_model("ant")[0], n, auto_reset, torch.device("cpu")
    return eng


def source(name, comments=True):
    """the text of carl_amd/csrc/<name>, with or without its // comments"""
    with open(os.path.join(ROOT, "carl_amd", "csrc", name)) as f:
        src = f.read()
    return src if comments else re.sub(r"//[^\n]*", "", src)
