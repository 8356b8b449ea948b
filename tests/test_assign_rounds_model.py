"""CPU: the sequential model of gs_assign.hip's rounds (tests/assign_rounds_model.py) equals the edge-by-edge
restatement (tests/assign_ref.py) record for record and in final state, whatever the batch cut and the order in
which the lanes of a step are visited."""
import pytest

import assign_ref as R
import assign_rounds_model as M

STREAMS = R.streams()
_want = {}


def want(name):
    if name not in _want:
        recs, ref = R.run(STREAMS[name])
        _want[name] = (recs, ref.state())
    return _want[name]


@pytest.mark.parametrize("cut", [None, 1, 7, 64])
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_model_equals_reference(name, cut):
    edges = STREAMS[name]
    recs, state = want(name)
    got, model = M.run(edges, cut, seed=len(edges) + (cut or 0))
    assert got == recs
    assert model.state() == state


def test_rounds_are_few_on_random_streams_and_one_per_edge_on_a_relabelled_hub():
    _, m = M.run(STREAMS["rmat12"])
    assert 1 <= m.rounds <= 40
    _, m = M.run(STREAMS["hub_relabelled"])
    assert m.rounds == 300
    _, m = M.run(STREAMS["chain_up"])
    assert m.rounds == 1
