"""GPU: AssignComponents (gs_assign_*) against the edge-by-edge restatement of tests/assign_ref.py: every record
exact -- (vertex, label, position of its edge in the stream) -- and in order.  The partition lives on the device
across calls, so every stream is cut into batches in several ways and must give the same records."""
import functools

import numpy as np
import pytest
import torch

import assign_ref as R

pytestmark = pytest.mark.gpu
STREAMS = R.streams()
CUTS = [None, 1, 7, 64, 4096]
CASES = [(name, cut) for name in sorted(STREAMS) for cut in CUTS if cut != 1 or name in R.SHORT]


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


@functools.lru_cache(maxsize=None)
def _columns(name):
    e = STREAMS[name]
    s, d = np.array([a for a, _ in e], dtype=np.int64), np.array([b for _, b in e], dtype=np.int64)
    s.setflags(write=False)
    d.setflags(write=False)
    return s, d


@functools.lru_cache(maxsize=None)
def _want(name, upto=None):
    """(records, state as sorted (vertex, label) rows) of the stream's first `upto` edges"""
    recs, ref = R.run(STREAMS[name][:upto])
    return tuple(recs), sorted(ref.state().items())


def _cuts(n, size):
    size = size or max(n, 1)
    return [(a, min(n, a + size)) for a in range(0, n, size)]


def _records(cols, base):
    v, c, e = (_np(x).tolist() for x in cols)
    return [(a, b, i + base) for a, b, i in zip(v, c, e)]


def _feed(state, s, d, cuts, mode="host", room=0):
    out = None
    if mode == "device_out":
        out = (torch.empty(room, dtype=torch.int64, device="cuda"), torch.empty(room, dtype=torch.int64, device="cuda"),
               torch.empty(room, dtype=torch.uint32, device="cuda"))
    got = []
    for a, b in cuts:
        bs, bd = s[a:b], d[a:b]
        if mode != "host":
            bs, bd = torch.from_numpy(np.array(bs)).cuda(), torch.from_numpy(np.array(bd)).cuda()
        cols = state.edges(bs, bd, out=out)
        assert all(isinstance(c, torch.Tensor) and c.is_cuda for c in cols) == (mode != "host")
        lb = state.last_batch()
        assert lb["records"] == len(cols[0]) == state.last_records
        assert lb["rounds"] >= 1 or lb["merging_edges"] == 0      # an edge that merged took a round
        got += _records(cols, a)
    return got


def _rows(state, device=False):
    k, v = state.export(device)
    return list(zip(_np(k).tolist(), _np(v).tolist()))


@pytest.mark.parametrize("mode", ["host", "device", "device_out"])
@pytest.mark.parametrize("name,cut", CASES)
def test_records_are_exact_whatever_the_cut(engine, name, cut, mode):
    s, d = _columns(name)
    want, rows = _want(name)
    cuts = _cuts(len(s), cut)
    per_batch = np.bincount(np.array([p for _, _, p in want], dtype=np.int64) // (cut or len(s)), minlength=len(cuts))
    with engine.assign_components() as st:
        got = _feed(st, s, d, cuts, mode, int(per_batch.max()) + 1)
        assert got == list(want)
        assert _rows(st, device=mode != "host") == rows
        assert st.size() == (len(rows), len({c for _, c in rows}), len(want))
    # replaying the records, the last label of every vertex is the state; a vertex without a record of its own
    # joined as the smaller id that relabelled a component ("not for x itself") and has been its label ever since
    last = {}
    for v, c, _ in got:
        last[v] = c
    assert set(last) <= {v for v, _ in rows}
    assert [(v, last.get(v, v)) for v, _ in rows] == rows


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_state_is_the_window_components_of_the_whole_stream(engine, name):
    s, d = _columns(name)
    k, v = engine.components(s, d)
    with engine.assign_components() as st:
        st.edges(s, d)
        ek, ev = st.export()
        assert np.array_equal(ek, k) and np.array_equal(ev, v)
        assert _rows(st) == sorted(R.components_of(STREAMS[name]).items())


def test_table_grows_several_times(engine):
    s, d = _columns("wide_30000")
    with engine.assign_components() as st:
        _feed(st, s, d, _cuts(len(s), 1000))
        slots, growths = st.capacity()
        assert growths >= 3 and st.size()[0] == 30000 and slots >= 2 * 30000


@pytest.mark.parametrize("name", ["random_v200", "pairs_zip_backward", "rmat12"])
def test_short_capacity_leaves_the_state_alone(engine, pkg, name):
    s, d = _columns(name)
    half = len(s) // 10      # early enough that the rest of the stream still merges components
    want = [r for r in _want(name)[0] if r[2] >= half]
    assert len(want) > 2
    with engine.assign_components() as st:
        _feed(st, s, d, [(0, half)])
        before, size = _rows(st), st.size()
        for cap in (len(want) - 1, 0, 1):
            with pytest.raises(pkg.GsError) as err:
                st.edges(s[half:], d[half:], capacity=cap)
            assert err.value.status == -2 and st.last_records == len(want)     # GS_ECAPACITY, the exact R
            assert _rows(st) == before and st.size() == size
        assert _records(st.edges(s[half:], d[half:], capacity=len(want)), half) == want
        assert _rows(st) == _want(name)[1]


@pytest.mark.parametrize("name", ["random_v2000", "hub_relabelled", "special_ids", "wide_30000"])
@pytest.mark.parametrize("device", [False, True])
def test_export_import_mid_stream_continues_with_the_same_records(engine, name, device):
    s, d = _columns(name)
    half = len(s) // (8 if name == "special_ids" else 2)      # eight ids: they are one component soon
    want = [r for r in _want(name)[0] if r[2] >= half]
    assert want
    with engine.assign_components() as st, engine.assign_components() as st2:
        _feed(st, s, d, _cuts(half, 64))
        k, v = st.export(device)
        assert _rows(st) == _want(name, half)[1]
        st2.load(k, v)
        assert _rows(st2) == _want(name, half)[1] and st2.size()[:2] == st.size()[:2]
        got = _feed(st2, s[half:], d[half:], _cuts(len(s) - half, 64))
        assert [(a, b, p + half) for a, b, p in got] == want
        assert _rows(st2) == _want(name)[1]


def test_import_takes_a_window_components_output(engine):
    s, d = _columns("random_v2000")
    half = len(s) // 2
    k, v = engine.components(s[:half], d[:half])
    with engine.assign_components() as st:
        st.load(k, v)
        got = _records(st.edges(s[half:], d[half:]), half)
        assert got == [r for r in _want("random_v2000")[0] if r[2] >= half]


def test_import_refuses_a_used_state_and_rows_that_break_the_label_rule(engine, pkg):
    good = (np.array([5, 3, 9, 7, -4], dtype=np.int64), np.array([3, 3, 7, 7, -4], dtype=np.int64))
    bad = {"label above its vertex": ([3, 5], [5, 5]),
           "the label's own row carries another label": ([1, 3, 5], [1, 1, 3]),
           "the label has no row": ([3, 5], [3, 2]),
           "a vertex twice": ([3, 5, 5], [3, 3, 3]),
           "a chain of labels at the extremes": ([R.I64_MIN, -1, R.I64_MAX], [R.I64_MIN, R.I64_MIN, -1])}
    with engine.assign_components() as st:
        for why, (k, v) in bad.items():
            with pytest.raises(pkg.GsError) as err:
                st.load(np.array(k, dtype=np.int64), np.array(v, dtype=np.int64))
            assert err.value.status == -1, why     # GS_EINVAL
            assert st.size() == (0, 0, 0) and _rows(st) == []
        st.load(*good)
        assert _rows(st) == sorted(zip(good[0].tolist(), good[1].tolist())) and st.size() == (5, 3, 0)
        with pytest.raises(pkg.GsError) as err:
            st.load(*good)
        assert err.value.status == -1
        assert _records(st.edges(np.array([9, 1]), np.array([5, -4])), 0) == [(7, 3, 0), (9, 3, 0), (1, -4, 1)]
    with engine.assign_components() as st:
        st.edges(np.array([1]), np.array([2]))
        with pytest.raises(pkg.GsError) as err:
            st.load(*good)
        assert err.value.status == -1 and _rows(st) == [(1, 1), (2, 1)]


def test_last_batch_reports_rounds_merging_edges_and_records(engine):
    with engine.assign_components() as st:
        s, d = _columns("hub_relabelled")
        v, _, _ = st.edges(s, d)
        lb = st.last_batch()
        assert lb["rounds"] == 300 and lb["merging_edges"] == 300 and lb["records"] == len(v) == len(_want("hub_relabelled")[0])
        assert lb["live_after"] == {1: 299, 2: 298, 4: 296, 8: 292}
        st.edges(s, d)      # every edge inside one component now
        assert st.last_batch() == {"rounds": 0, "merging_edges": 0, "records": 0, "live_after": {1: 0, 2: 0, 4: 0, 8: 0}}
    with engine.assign_components() as st:
        s, d = _columns("rmat12")
        st.edges(s, d)
        lb = st.last_batch()
        assert 1 <= lb["rounds"] <= 40 and lb["merging_edges"] == st.size()[0] - st.size()[1]
        st.edges(np.array([1 << 50]), np.array([0]))     # one edge that merges: at least one round
        assert st.last_batch()["rounds"] == 1 and st.last_batch()["records"] == 1


def test_iterative_connected_components_on_the_builtin_data(pkg):
    env = pkg.StreamExecutionEnvironment()
    job = pkg.IterativeConnectedComponents(env)
    assert job.getEdgesDataSet() == R.BUILTIN
    want = [(v, c) for v, c, _ in R.BUILTIN_RECORDS]
    assert job.run().collect() == want
    env.setMicroBatch(3)
    assert job.run(R.BUILTIN).collect() == want
    env.setParallelism(2)
    with pytest.raises(ValueError, match="parallelism 1"):
        job.run()
