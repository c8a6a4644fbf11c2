"""Every case of tests/context_kernel_cases.py on the device, through the C ABI (`carl_sample_contexts` /
`carl_verify_contexts` with a row stride, which the Python wrapper cannot pass), against the oracle
(oracle/context_sampler.c).  The bars and where they come from: context_kernel_cases.py's docstring."""
import ctypes as C

import numpy as np
import pytest
import torch

import context_kernel_cases as K
from carl_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CASES = K.CASES
IDS = [c.name for c in CASES]


def upload_specs(specs, device):
    return torch.from_numpy(np.frombuffer(bytes(specs), dtype=np.uint8).copy()).to(device)


def sample(case, device, *, n=None, stride=None, offset=None):
    """[F][stride] float32 as the device left it; the table holds CANARY everywhere before the launch"""
    n = case.n if n is None else n
    stride = case.stride if stride is None else stride
    specs = case.specs()
    specs_dev = upload_specs(specs, device)
    table = torch.from_numpy(np.full((case.F, stride), K.CANARY, np.float32)).to(device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().carl_sample_contexts(specs_dev.data_ptr(), specs, case.F, n, stride,
                                                    case.offset if offset is None else offset, C.c_uint64(case.seed),
                                                    table.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return table.cpu().numpy()


def verify(case, table, device):
    """the device's count for a host [F][stride] table; n_bad_out holds garbage before the call"""
    specs = case.specs()
    specs_dev = upload_specs(specs, device)
    t = torch.from_numpy(np.array(table, dtype=np.float32)).to(device)  # a copy: the oracle tables are read-only
    n_bad = torch.full((1,), K.GARBAGE, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().carl_verify_contexts(specs_dev.data_ptr(), specs, case.F, case.n, t.shape[1], t.data_ptr(),
                                                    n_bad.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return int(n_bad.item())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sampled_table_matches_the_oracle(case, device):
    got_full = sample(case, device)
    want_full = K.oracle_table(case)
    assert got_full.shape == want_full.shape == (case.F, case.stride)
    # the padding columns come back bit-identical
    assert np.array_equal(bits(got_full[:, case.n:]), bits(want_full[:, case.n:])), "padding columns written"
    got, want = got_full[:, :case.n], want_full[:, :case.n]
    flips = 0
    for j, sp in enumerate(case.spec_list):
        g, w = got[j], want[j]
        where = f"{case.name} row {j} ({K.branch_of(sp)})"
        if K.is_exact(sp):
            assert np.array_equal(bits(g), bits(w)), where
        elif K.branch_of(sp) == "log":
            rel = np.abs(g.astype(np.float64) - w) / w
            print(f"{where}: worst relative error {rel.max():.3e}, bar {case.log_bar():.3e}")
            assert (g >= np.float32(sp.lower)).all() and (g <= np.float32(sp.upper)).all(), where
            assert rel.max() <= case.log_bar(), where
        else:
            bar = case.normal_bar(j, w)
            err = np.abs(g.astype(np.float64) - w)
            print(f"{where}: worst |got - want| / bar {np.max(err / bar):.3e}")
            miss = err > bar
            if miss.any():  # only where the oracle's own trace shows a candidate on the edge of a bound
                alt = case.normal_alternative(j, w)
                ok = np.abs(g.astype(np.float64) - alt) <= bar  # False where alt is NaN
                assert ok[miss].all(), (where, np.nonzero(miss & ~ok)[0][:8], g[miss & ~ok][:8], w[miss & ~ok][:8])
                flips += int(miss.sum())
    assert flips <= case.flip_cap(), (case.name, flips)
    # a table the device sampled verifies against the specs it was sampled from, on the device
    assert verify(case, got_full, device) == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_verifier_counts_what_the_oracle_counts(case, device):
    specs = case.specs()
    valid = K.oracle_table(case)
    assert verify(case, valid, device) == 0  # also: GARBAGE in n_bad_out is overwritten when nothing is bad
    planted = K.planted_table(case)
    want = O.verify_contexts(specs, planted, case.n)
    assert want > 0 and verify(case, planted, device) == want
    all_bad = np.full_like(valid, np.nan)
    assert O.verify_contexts(specs, all_bad, case.n) == case.F * case.n
    assert verify(case, all_bad, device) == case.F * case.n


def test_one_bad_entry_per_feature_row_of_256(device):
    case = K.BY_NAME["f256"]
    t = K.oracle_table(case).copy()
    for f in range(case.F):
        t[f, f] = np.nan  # a different context in every row: 256 waves' worth of single counts
    t[:, case.n:] = np.nan
    assert O.verify_contexts(case.specs(), t, case.n) == 256 == verify(case, t, device)


def test_shards_at_a_padded_layout_are_slices_of_one_launch(device):
    case = K.BY_NAME["shape-n1003-s1008"]
    o = 2**32 - 150  # the carry into the high counter word falls inside the first shard
    full = sample(case, device, offset=o)
    lo = sample(case, device, n=300, stride=305, offset=o)
    hi = sample(case, device, n=703, stride=720, offset=o + 300)
    assert np.array_equal(bits(full[:, :300]), bits(lo[:, :300]))
    assert np.array_equal(bits(full[:, 300:1003]), bits(hi[:, :703]))
    for part, n in ((lo, 300), (hi, 703)):
        assert (bits(part[:, n:]) == bits(K.CANARY)).all()
