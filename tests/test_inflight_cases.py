"""The shared-rule matrix of tests/inflight_cases.py on the CPU: the streams round-trip through the
oracle, the planted structure survives the coding parameters (counted from the oracle's block
lengths), and the restated rule gives each case the split it is built for.  The GPU half is
tests/test_gpu_inflight.py."""
import functools

import numpy as np

import inflight_cases as I
import oracle as O


@functools.lru_cache(maxsize=None)
def matrix():
    return {c.name.split()[0]: c for c in I.shared_matrix()}


def test_restated_rule_by_hand():
    assert I.shared_solo([10] * 7) == 0                       # under 8 blocks: no solo waves
    assert I.shared_solo([0] * 8 + [5] * 8) == 4              # reference 0: every candidate, up to nbr / 4
    assert I.shared_solo([0] * 14 + [5] * 2) == 2             # ... or the non-empty ones
    assert I.shared_solo([100] * 60 + [130] * 4) == 0         # 1.3 x is not heavier than 1.3 x
    assert I.shared_solo([100] * 60 + [131] * 4) == 4
    assert I.shared_solo([100] * 1100 + [0] * 60 + [200] * 3) == 3    # rank 1024 of 1163, not the lightest
    assert I.shared_solo([100] * 1020 + [0] * 60 + [200] * 3) == 270  # rank 1024 of 1083 is empty: the cap
    assert I.shared_solo([0] * 100 + [7] * 100, waves=12) == 12       # one block per wave


def test_lossless_cases_round_trip():
    m = matrix()
    # (shared_matrix itself asserts that cases 1 to 5 decode to their images)
    np.testing.assert_array_equal(m["1"].want[:, :, :72], 128)
    assert len(np.unique(m["2"].want)) == 256
    np.testing.assert_array_equal(m["9"].want, O.decode(m["9"].cs)[0])


def test_case_1_has_empty_blocks_and_a_reference_of_weight_0():
    w = matrix()["1"].weights
    assert len(w) == 16 and sorted(w)[0] == 0
    assert matrix()["1"].solo == (4, 4) and sum(1 for v in w if v) >= 4


def test_case_2_blocks_lie_within_the_factor():
    w = matrix()["2"].weights
    assert len(w) == 64 and max(w) <= 1.3 * min(w)
    assert matrix()["2"].solo == (0, 0)


def _planted(w):
    s = sorted(w, reverse=True)
    ref = s[min(1024, len(w) - 1)]
    heavy = [v for v in w if v > 1.3 * ref]
    rest = [v for v in w if v <= 1.3 * ref]
    return ref, heavy, rest


def test_cases_3_4_5_planted_blocks():
    m = matrix()
    for k, nbr, planted, solo in (("3", 1089, 5, 5), ("4", 1089, 300, 272), ("5", 1024, 5, 5)):
        w = m[k].weights
        ref, heavy, rest = _planted(w)
        assert len(w) == nbr and len(heavy) == planted and m[k].solo == (solo, solo)
        # the default rule gives plain blocks to solo waves too (a solo wave costs 1 / 2.5 of a lane
        # wave per byte): a planted block is lighter than 2.5 x the lightest plain one
        assert max(heavy) < 2.5 * min(rest)
    assert I.SOLO_WAVES >= 272


def test_case_6_loses_blocks_to_the_layer_limit():
    c = matrix()["6"]
    full = I.oracle_decode(c.cs)
    assert c.layers == 1 and not np.array_equal(full, c.want)
