"""CPU: tests/matching_ref.py -- the restatement of CentralizedWeightedMatching's mapper that the GPU tests
compare against -- pinned to event lists worked by hand from the Java (tests/golden/matching_fixtures.json)."""
import json
from pathlib import Path

import numpy as np
import pytest

import matching_ref as ref

FIX = json.loads((Path(__file__).parent / "golden" / "matching_fixtures.json").read_text())
TYPES = {"ADD": ref.ADD, "REMOVE": ref.REMOVE}
CASES = {c["name"]: c for c in FIX["cases"]}
EXTREMES = [ref.I64_MIN, ref.I64_MAX, -1, 0, 1, 1 << 62, (1 << 62) + 1, -(1 << 62), 3, 7]


def _want(case):
    return [(TYPES[t], s, d, v, i) for t, s, d, v, i in case["events"]]


def test_fixtures_cover_the_cases_the_operator_must_get_right():
    assert set(CASES) >= {"first_edge", "rejected_lighter_edge", "displaces_one_collision", "displaces_two_collisions",
                          "matched_pair_arrives_again", "self_loops", "identical_edge_negative_weight",
                          "long_max_against_two_to_the_62"}


@pytest.mark.parametrize("cls", [ref.Matching, ref.FastMatching])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_hand_derived_events(name, cls):
    case = CASES[name]
    m = cls()
    got = m.edges(*zip(*case["edges"]))
    assert got == _want(case)
    assert m.is_matching()
    assert m.records == len(case["edges"])


def test_java_long_wraps():
    assert ref.java_long(1 << 63) == ref.I64_MIN
    assert ref.java_long(2 * (1 << 62)) == ref.I64_MIN
    assert ref.java_long(2 * ref.I64_MIN) == 0
    assert ref.java_long(ref.I64_MAX + 1) == ref.I64_MIN
    assert ref.java_long(-5) == -5


def _streams():
    rng = np.random.default_rng(0x3A7C)
    n = 3000
    yield "small_ids", rng.integers(0, 60, n), rng.integers(0, 60, n), rng.integers(0, 1 << 16, n)
    yield "ratings", rng.integers(0, 200, n), rng.integers(0, 200, n), 10 * rng.integers(1, 6, n)
    yield "extremes", rng.integers(0, 41, n), rng.integers(0, 41, n), np.array(EXTREMES, dtype=np.int64)[rng.integers(0, 10, n)]


@pytest.mark.parametrize("stream", list(_streams()), ids=lambda s: s[0])
def test_m_is_a_matching_after_every_edge(stream):
    """the invariant the per-vertex state rests on; and the dictionary variant is the literal scan"""
    _, src, dst, val = stream
    lit, fast = ref.Matching(), ref.FastMatching()
    accepted = 0
    for s, d, v in zip(src.tolist(), dst.tolist(), val.tolist()):
        ev = lit.flat_map(s, d, v)
        assert fast.flat_map(s, d, v) == ev
        assert lit.is_matching()
        assert lit.M == fast.M
        if ev:
            accepted += 1
            assert ev[-1] == (ref.ADD, s, d, v) and all(e[0] == ref.REMOVE for e in ev[:-1]) and len(ev) <= 3
    assert 0 < accepted < len(src)
    assert lit.export() == sorted(fast.M) and lit.total_weight() == fast.total_weight()
