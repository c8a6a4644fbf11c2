"""tests/context_kernel_cases.py held against the oracle on the host: every kind and every branch of the device
sampler has a case that reaches it (by the oracle's trace, not by the case's name), the committed extreme-draw ids
draw what they say, the oracle's own tables verify, no entry of the oracle's trace sits on an accept / reject edge,
and the recorded float32 deviations behind the GPU test's bars are the measured ones."""
import numpy as np
import pytest

import context_kernel_cases as K
from carl_amd import _lib
from oracle import oracle as O

CASES = K.CASES
IDS = [c.name for c in CASES]


def branches_reached(case):
    """from the specs' kinds and, for NORMAL_FLOAT rows, the attempt the oracle's trace takes"""
    got = set()
    for j, sp in enumerate(case.spec_list):
        b = K.branch_of(sp)
        if b != "normal":
            got.add(b)
            continue
        acc = case.trace(j).accepted
        got |= {name for name, hit in (("normal0", acc == 0), ("normal8", (acc >= 8) & (acc < 32)),
                                       ("exhausted", acc == 32)) if hit.any()}
    return got


def test_the_table_spans_the_shapes_strides_and_keys():
    assert {c.n for c in CASES} >= {1, 63, 64, 65, 255, 256, 257, 1003}
    assert {c.F for c in CASES} >= {1, 7, 256}
    assert {c.seed for c in CASES} == {99, 2**32 + 1, 2**64 - 1}
    assert {c.offset for c in CASES} >= {0, 2**32 - 5, 2**62}
    assert all(c.n >= 10 for c in CASES if c.offset == 2**32 - 5)  # the carry happens inside the launch
    kinds = {"dense" if c.stride == c.n else "plus5" if c.stride == c.n + 5 else "r16" if c.stride == K.round_up_16(c.n)
             else "other" for c in CASES}
    assert kinds >= {"dense", "plus5", "r16"}
    f256 = K.BY_NAME["f256"]
    assert {sp.kind for sp in f256.spec_list} == set(range(5)) and {K.branch_of(sp) for sp in f256.spec_list} >= {"log", "linear"}
    assert all(sp.n_choices <= _lib.MAX_CHOICES for c in CASES for sp in c.spec_list)
    assert any(sp.n_choices == _lib.MAX_CHOICES for sp in K.BY_NAME["categorical"].spec_list)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_reaches_the_branches_it_claims(case):
    got = branches_reached(case)
    assert case.reaches and case.reaches <= got, (case.reaches, got)


def test_every_branch_has_a_case():
    claimed = set().union(*(c.reaches for c in CASES))
    assert claimed == set(K.BRANCHES)
    # the redraw cases really spread: every attempt index is taken somewhere, and the window exhausts a few per cent
    acc = K.BY_NAME["normal-window"].trace(1).accepted
    assert set(np.unique(acc)) == set(range(33))
    assert 0.02 < float((acc == 32).mean()) < 0.08
    assert (K.BY_NAME["normal-exhausted"].trace(0).accepted == 32).all()
    assert np.array_equal(K.oracle_table(K.BY_NAME["normal-exhausted"])[:, :K.N_EDGE],
                          np.repeat(np.array([[10.0], [8.0]], np.float32), K.N_EDGE, axis=1))


def test_log_equal_bounds_round_both_ways_in_float32():
    x = np.array([sp.lower for sp in K.BY_NAME["log"].spec_list[:5]], np.float32)
    back = np.exp(np.log(x))
    assert (back < x).any() and (back > x).any(), back - x


def test_extreme_ids_draw_the_extremes():
    for name, cid, word in (("u0", K.EXTREME_U0, 0), ("utop", K.EXTREME_UTOP, 0xFFFFFF)):
        w = O.lane_words(99, cid, 0, 0x40000000)
        assert int(w[0]) >> 8 == word
        assert O.u01(w[0]) == (0.0 if word == 0 else 1.0 - 2.0**-24)
        cases = [c for c in CASES if c.name.startswith(name + "-")]
        assert len(cases) == len(K.EXTREME_SPECS)
        for c in cases:
            assert (c.seed, c.F) == (99, 1) and c.offset + K.EXTREME_AT == cid and K.EXTREME_AT < c.n
            assert c.u(0)[K.EXTREME_AT] == np.float32(0.0 if word == 0 else 1.0 - 2.0**-24)
    zero, top, (best_id, best) = O.scan_u(99, 0, K.EXTREME_UTOP - 1000, 2000)
    assert top == [K.EXTREME_UTOP] and zero == [] and (best_id, best) == (K.EXTREME_UTOP, 0xFFFFFF)
    assert O.scan_u(99, 0, K.EXTREME_U0 - 1000, 2000)[0] == [K.EXTREME_U0]
    # u1 = 1 - 2^-24 is the widest an attempt's |z| gets: sqrt(-2 log 2^-24) = 5.77 (the always-exhausted window is safe)
    t = K.BY_NAME["utop-normal"].trace(0)
    assert t.u1[K.EXTREME_AT, 0] == np.float32(1.0 - 2.0**-24) and abs(np.sqrt(-2 * np.log(1.0 - float(t.u1[K.EXTREME_AT, 0]))) - 5.768) < 1e-3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_table_verifies_and_leaves_the_padding(case):
    t = K.oracle_table(case)
    assert t.shape == (case.F, case.stride)
    assert np.array_equal(t[:, case.n:].view(np.uint32), case.canary_table()[:, case.n:].view(np.uint32))
    assert O.verify_contexts(case.specs(), t, case.n) == 0
    # the accept / reject decision of no entry hangs on the last bits (the GPU test allows flip_cap of them)
    assert K.near_bound_entries(case) == 0 <= case.flip_cap()


def test_oracle_verifier_semantics_on_the_planted_values():
    c = K.BY_NAME["verify-edges"]
    specs = c.specs()
    nan, inf = float("nan"), K.INF
    good = np.array([0.3, 0.5, 2.0, 2.0, 1.0], np.float32)

    def bad(row, value):
        t = np.repeat(good[:, None], 3, axis=1)
        t[row, 1] = value
        return O.verify_contexts(specs, t)

    assert bad(0, 0.3) == 0
    assert [bad(0, v) for v in (inf, -inf, nan)] == [0, 0, 1]           # infinite bounds hold +-inf, nothing holds NaN
    assert [bad(1, v) for v in (-0.0, inf, -inf, nan, K.up(1.0))] == [0, 1, 1, 1, 1]
    assert [bad(2, v) for v in (3.0, K.up(1.0), 2.5, nan, -0.0)] == [0, 1, 1, 1, 1]
    assert [bad(3, v) for v in (2.5, K.up(3.0), nan)] == [0, 1, 1]      # a constant categorical: its range only
    # the planted tables: padding columns never count, whatever they hold
    for case in CASES:
        t = K.planted_table(case)
        assert np.isnan(t[:, case.n:]).all()
        want = O.verify_contexts(case.specs(), t, case.n)
        assert want == O.verify_contexts(case.specs(), np.ascontiguousarray(t[:, :case.n]))
        if case.n >= 16:
            assert want >= case.F  # the NaN of every row, at least


def test_recorded_deviations_are_the_measured_ones():
    d_log = {c.name: K.measure_d_log(c) for c in CASES if c.rows("log")}
    d_z = {c.name: K.measure_d_z(c) for c in CASES if any(c.spec_list[j].sigma > 0 for j in c.rows("normal"))}
    for title, d in (("D_LOG", d_log), ("D_Z", d_z)):
        print(f"{title} = {{")
        for k, v in d.items():
            print(f'    "{k}": {v:.3e},')
        print("}")
    for recorded, measured in ((K.D_LOG, d_log), (K.D_Z, d_z)):
        assert set(recorded) == set(measured)
        for k, v in measured.items():  # to the three digits it is written with
            assert abs(v - recorded[k]) <= 0.005 * recorded[k] + 1e-12, (k, v, recorded[k])
    for c in CASES:
        if c.name in K.D_LOG:
            assert c.log_bar() == max(3e-6, 4 * K.D_LOG[c.name])
