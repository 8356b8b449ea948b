"""CPU: the batch-parallel round scheme of gs_matching.hip (tests/matching_rounds_model.py restates it step for
step) yields exactly the sequential mapper's events (tests/matching_ref.py), whole and cut into batches."""
import random

import pytest

import matching_ref as ref
from matching_rounds_model import RoundsModel

EXTREMES = [ref.I64_MIN, ref.I64_MAX, -1, 0, 1, 1 << 62, (1 << 62) + 1, -(1 << 62), 3, 7]


def _streams():
    rng = random.Random(5)
    n = 1500
    yield "extremes", [rng.randrange(41) for _ in range(n)], [rng.randrange(41) for _ in range(n)], \
        [rng.choice(EXTREMES) for _ in range(n)], (n, 7, 1)
    n = 400
    yield "path", list(range(n)), list(range(1, n + 1)), [3 ** (i % 38) for i in range(n)], (n, 64)
    n = 600
    yield "star", [0] * n, list(range(1, n + 1)), list(range(1, n + 1)), (n, 100)
    n = 4000
    skew = lambda: int(2 ** (rng.random() * 10)) - 1      # hubs, as R-MAT has them
    s, d = [skew() for _ in range(n)], [skew() for _ in range(n)]
    yield "hubs_16bit", s, d, [rng.randrange(0x10000) for _ in range(n)], (n, 500, 7)
    yield "hubs_ratings", s, d, [10 * rng.randrange(1, 6) for _ in range(n)], (n, 500)
    ids = [-1, ref.I64_MIN, ref.I64_MAX, 1 << 33, (1 << 40) + 5, 0, 1]
    n = 300
    yield "ids", [rng.choice(ids) for _ in range(n)], [rng.choice(ids) for _ in range(n)], \
        [rng.randrange(-50, 50) for _ in range(n)], (n, 3)


@pytest.mark.parametrize("stream", list(_streams()), ids=lambda s: s[0])
def test_rounds_give_the_sequential_events(stream):
    name, src, dst, val, cuts = stream
    want = ref.FastMatching().edges(src, dst, val)      # pinned to the literal scan by test_matching_ref.py
    assert want
    for cut in cuts:
        for seed in (0, 1):
            m, got = RoundsModel(seed), []
            for a in range(0, len(src), cut):
                got.extend(m.batch(src[a:a + cut], dst[a:a + cut], val[a:a + cut], a))
            assert got == want, (name, cut, seed)
            assert m.rounds <= len(src) + len(range(0, len(src), cut))


def test_path_needs_about_one_round_per_accepted_edge():
    n = 400
    src, dst, val = list(range(n)), list(range(1, n + 1)), [3 ** (i % 38) for i in range(n)]
    m = RoundsModel()
    ev = m.batch(src, dst, val)
    adds = sum(e[0] == ref.ADD for e in ev)
    assert adds > 0.9 * n and 0.9 * adds <= m.rounds <= n
