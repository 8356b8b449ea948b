"""CPU: the edge-by-edge restatement of AssignComponents (tests/assign_ref.py) against records derived by hand,
its fast variant against the literal one, and the reason the library builds the comments' reading: under it a
record that comes back over the feedback edge never emits and never changes the state, while the literal
addToExistingComponent (:136-139) emits the same record again."""
import random

import pytest

import assign_ref as R


def test_builtin_records_by_hand():
    got, ref = R.run(R.BUILTIN, R.AssignLiteral())
    assert got == R.BUILTIN_RECORDS
    assert ref.state() == {v: 1 for v in range(1, 13)}


def test_semantics_table_row_by_row():
    ref = R.AssignLiteral()
    assert ref.edge(7, 5) == [(7, 5), (5, 5)]            # both unknown: (s, m), (t, m)
    assert ref.edge(9, 9) == [(9, 9), (9, 9)]            # a self-loop on an unknown vertex
    assert ref.edge(8, 7) == [(8, 5)]                    # unknown x > c joins
    assert ref.edge(7, 3) == [(5, 3), (7, 3), (8, 3)]    # unknown x < c relabels, x itself not emitted
    assert ref.edge(9, 8) == [(9, 3)]                    # both known: the larger label's vertices
    assert ref.edge(3, 9) == [] and ref.edge(5, 5) == []
    assert ref.edge(-1, 9) == [(3, -1), (5, -1), (7, -1), (8, -1), (9, -1)]   # -1 is an ordinary vertex
    assert ref.state() == {v: -1 for v in (-1, 3, 5, 7, 8, 9)}


@pytest.mark.parametrize("name", ["builtin", "random_v8", "random_v200", "chain_down", "hub_relabelled", "self_loops",
                                  "special_ids", "pairs_zip_backward"])
def test_fast_variant_is_the_literal_one(name):
    edges = R.streams()[name]
    a, ra = R.run(edges, R.AssignLiteral())
    b, rb = R.run(edges, R.AssignFast())
    assert a == b and ra.state() == rb.state()
    assert rb.state() == R.components_of(edges)


def _feedback_streams():
    out = [R.random_edges(random.Random(s).choice([6, 20, 60, 300]), random.Random(s + 1).randrange(5, 160), s)
           for s in range(200)]
    S = R.streams()
    return out + [S[k] for k in ("builtin", "chain_up", "chain_down", "hub_relabelled", "star", "self_loops")]


def test_fed_back_records_emit_nothing_under_the_intended_reading():
    """Every emitted record (v, c) re-enters the mapper as the edge (v, c) at a random later position: it must
    emit nothing, and the true edges' records and the final state must be those of the stream without feedback."""
    for k, edges in enumerate(_feedback_streams()):
        rng = random.Random(1000 + k)
        want, plain = R.run(edges)
        ref, got = R.AssignFast(), []
        queue = []   # (position from which it may arrive, record)
        for i, (s, t) in enumerate(edges):
            rng.shuffle(queue)
            while queue and rng.random() < 0.5:
                v, c = queue.pop()
                assert ref.edge(v, c) == [], (k, i, v, c)
            recs = ref.edge(s, t)
            got += [(v, c, i) for v, c in recs]
            queue += recs
        for v, c in queue:
            assert ref.edge(v, c) == []
        assert got == want and ref.state() == plain.state()


def test_the_literal_mapper_emits_its_fed_back_record_again():
    ref = R.AssignLiteral(literal=True)
    assert ref.edge(1, 2) == [(1, 1), (2, 1)]
    assert ref.edge(1, 3) == [(3, 1)]      # emitted, but 3 is not added to the set (:136-139)
    assert ref.edge(3, 1) == [(3, 1)]      # so its own record, fed back, finds 3 unknown and is emitted again
    assert ref.edge(3, 1) == [(3, 1)]      # ... for ever
    fixed = R.AssignLiteral()
    fixed.edge(1, 2), fixed.edge(1, 3)
    assert fixed.edge(3, 1) == []
