"""GPU: the JDK HashSet-order simulation of gs_hashset.hip (k_hs_detect, k_hs_jdk_prefix / _order / _group / _write
and the serial k_hs_jdk) held to the independent model of tests/jdk_hashmap_ref.py.

The expected records come from the model and its restatement of GenerateCandidateEdges
(jdk_hashmap_ref.candidate_records), not from the oracle, which shares the kernels' array layout and came from the
same reading of HashMap.  Every set here has tree bins whose hashes have both signs, where the JDK's signed
`(ph = p.hash) > h` decides the tree and with it the iteration order; one set per path of the simulation:
 - 11 and 39 keys: k_hs_jdk_prefix alone (capacity 64), the sign from bit 31 and from bit 63 of the id;
 - j << 24, 200 keys: trees form in the prefix; k > 192, so capacity 512 and the 256 group threads take over a
   table that already holds mixed-sign trees; 300 keys: those trees get new roots in the group phase;
 - j << 20, 3000 keys shuffled: tree bins split, untreeified and re-treeified by the group resizes;
 - 140 complex sets among plain ones in one window (three blocks of k_hs_jdk_prefix);
 - the chunked session, the self-pair term of gs_window_triangles, and the serial kernel in a child process.
Every comparison is exact."""
import os
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest
import torch
from jdk_hashmap_ref import build, candidate_records, hashset_order

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
B63 = 1 << 63
INT64_MIN = -B63


def _set(name):
    if name == "bit31-11":
        return [(j << 6) | ((j & 1) << 31) for j in range(1, 12)]
    if name == "bit63-39":
        return [(j << 6) - ((j & 1) << 63) for j in range(1, 40)]
    if name == "j24-200":
        return [j << 24 for j in range(1, 201)]
    if name == "j24-300":
        return [j << 24 for j in range(1, 301)]
    if name == "j20-3000":
        return [j << 20 for j in range(1, 3001)]
    assert name == "j20-3000-shuffled"
    return np.random.default_rng(20).permutation([j << 20 for j in range(1, 3001)]).tolist()


def _star(hub, ids):
    return np.full(len(ids), hub, dtype=np.int64), np.array(ids, dtype=np.int64)


def _check_window(engine, s, d, want=None):
    wa, wb, wf, flags = want or candidate_records(s, d)
    ga, gb, gf = engine.candidates(*(torch.from_numpy(x).cuda() for x in (s, d)))
    assert engine.last_candidates_jdk_flags == flags
    assert np.array_equal(ga.cpu().numpy(), wa) and np.array_equal(gb.cpu().numpy(), wb)
    assert np.array_equal(gf.cpu().numpy(), wf)


_star_cache = {}


def _star_window(name, hub):
    """(s, d, expected records), built once per window and shared (never modified)."""
    if (name, hub) not in _star_cache:
        s, d = _star(hub, _set(name))
        _star_cache[name, hub] = (s, d, candidate_records(s, d))
    return _star_cache[name, hub]


GROUP_PHASE_FROM = 193   # k_hs_jdk_prefix inserts until the table has 256 bins: the first 193 keys


@pytest.mark.parametrize("name", ["bit31-11", "bit63-39", "j24-200", "j24-300", "j20-3000-shuffled"])
def test_one_vertex_below_all_its_neighbours(engine, name):
    """The vertex's id is below every neighbour's, so the pair records show the whole iteration order.
    In j24-200 the seven keys of the group phase link into trees whose roots stay; j24-300 is there because its
    trees get a new root there (putTreeVal's moveRootToFront in j_put_group), asserted from the model."""
    ids = _set(name)
    hub = INT64_MIN if min(ids) < 0 else 0
    m = build(ids)
    assert m.mixed_sign_compares > 0 and m.flags == 3
    assert m.keys() != hashset_order(ids, signed=False)[0], "the set separates signed from unsigned compares"
    assert m.capacity() == {"bit31-11": 64, "bit63-39": 64, "j24-200": 512, "j24-300": 512,
                            "j20-3000-shuffled": 4096}[name]
    assert any(z >= GROUP_PHASE_FROM for z in m.root_moves_at) == (name in ("j24-300", "j20-3000-shuffled"))
    s, d, want = _star_window(name, hub)
    k = len(ids)
    assert int(want[2].sum()) == k * (k + 1) // 2 - 1      # every pair i <= j but the last element's self pair
    _check_window(engine, s, d, want)


@pytest.mark.parametrize("hub, last_above", [((100 << 24) + 1, True), ((150 << 24) + 1, False)])
def test_vertex_id_inside_the_id_range(engine, hub, last_above):
    """The `> vertexID` filter over an exact order, and the row count when the set's last element is or is not
    above the vertex (its self pair is the one that is never emitted)."""
    ids = _set("j24-200")
    order = hashset_order(ids)[0]
    assert (order[-1] > hub) == last_above
    s, d, want = _star_window("j24-200", hub)
    above = sum(x > hub for x in ids)
    assert int(want[2].sum()) == above * (above + 1) // 2 - int(last_above)
    _check_window(engine, s, d, want)


def _many_sets():
    rng = np.random.default_rng(130)
    V = 280
    s, d = [], []
    for t in range(V):
        k = 11 + (7 * t) % 30                       # 11 .. 40 neighbours
        v = -(t + 1)
        if t % 2 == 0:                              # crowded in bucket 0 up to capacity 64, both hash signs;
            j = np.arange(1, k + 1) + 64 * t        # every fourth vertex takes the sign from bit 63 (those ids
            sign = -B63 if t % 4 == 0 else (1 << 31)   # are below the vertex: the filter drops them)
            ids = [(int(x) << 6) + (sign if x & 1 else 0) for x in j]
        else:
            ids = np.unique(rng.integers(1, 1 << 40, k)).tolist()
        s += [v] * len(ids)
        d += ids
    p = rng.permutation(len(s))
    return np.array(s, dtype=np.int64)[p], np.array(d, dtype=np.int64)[p]


def test_many_complex_sets_in_one_window(engine):
    """140 complex sets (more than two 64-thread blocks of k_hs_jdk_prefix) alternate with plain ones; arrival
    order is shuffled across the vertices."""
    s, d = _many_sets()
    arrivals = {}
    for a, b in zip(s.tolist(), d.tolist()):
        arrivals.setdefault(a, []).append(b)
    models = [build(v) for v in arrivals.values()]
    assert sum(m.flags != 0 for m in models) == 140 > 128
    assert sum(m.mixed_sign_compares > 0 for m in models) == 140
    _check_window(engine, s, d)


@pytest.mark.parametrize("name", ["j24-200", "j20-3000"])
def test_self_pair_term_over_exact_orders(engine, oracle, name):
    """gs_window_triangles over a star with self-loops: the self pair (x, x) of every element of the hub's set but
    the LAST is a candidate, and it closes when x has a self-loop; the hub's own loop puts the hub into its set,
    below the filter.  The set's last element differs between the signed and the unsigned reading (asserted from
    the model); with the loop on one of the two and not the other, the count moves by the reading: it is the
    number of looped neighbours that are not last, from the model.  The oracle's two algorithms must say the same
    (tests/test_jdk_hashmap_ref.py holds the oracle's order to the model)."""
    ids = _set(name)
    arrivals = ids[:len(ids) // 3] + [0] + ids[len(ids) // 3:]        # the hub's set, its own loop in between
    last = hashset_order(arrivals)[0][-1]
    last_unsigned = hashset_order(arrivals, signed=False)[0][-1]
    assert last != last_unsigned and 0 not in (last, last_unsigned)
    counts = []
    for looped_last in (last, last_unsigned):
        looped = [ids[3], ids[len(ids) // 2], looped_last]
        assert len(set(looped)) == 3
        s = np.array([looped[0]] + [0] * len(arrivals) + looped[1:], dtype=np.int64)
        d = np.array([looped[0]] + arrivals + looped[1:], dtype=np.int64)
        want = len(looped) - (last in looped)
        w, ex, has, flags = oracle.window_triangles_ref(s, d)
        assert (flags, ex, w, has) == (3, want, want, True) and (w, ex, has) == oracle.window_triangles_fwd(s, d)
        assert engine.triangles(*(torch.from_numpy(x).cuda() for x in (s, d))) == (ex, w, has)
        assert engine.triangles(s, d) == (ex, w, has)
        counts.append(ex)
    assert counts == [2, 3]


def test_chunked_session_cuts_inside_pair_rows(engine):
    """gs_candidates_begin / _next over the 200-key window, 333 records a chunk (a pair row has up to 200)."""
    s, d, (wa, wb, wf, flags) = _star_window("j24-200", 0)
    total = engine.candidates_begin(torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda())
    assert total == len(wa) and engine.last_candidates_jdk_flags == flags
    parts, at, done = [], 0, False
    while not done:
        a, b, f, first, done = engine.candidates_next(333)
        assert first == at and (len(a) == 333 or done)
        at += len(a)
        parts.append([x.cpu().numpy() for x in (a, b, f)])
    assert at == total
    ga, gb, gf = (np.concatenate([p[i] for p in parts]) for i in range(3))
    assert np.array_equal(ga, wa) and np.array_equal(gb, wb) and np.array_equal(gf, wf)


SERIAL_CHILD = textwrap.dedent("""
    import os, sys
    import numpy as np
    assert os.environ["GS_HS_JDK_SERIAL"] == "1"
    sys.path[:0] = [{root!r}, {tests!r}]
    import __graft_entry__ as ge
    from jdk_hashmap_ref import candidate_records
    pkg = ge.load_package()
    eng = pkg.Engine(0)
    for ids in ([j << 24 for j in range(1, 201)],
                np.random.default_rng(20).permutation([j << 20 for j in range(1, 3001)]).tolist()):
        s, d = np.zeros(len(ids), np.int64), np.array(ids, np.int64)
        wa, wb, wf, flags = candidate_records(s, d)
        ga, gb, gf = eng.candidates(s, d)
        assert eng.last_candidates_jdk_flags == flags == 3
        assert np.array_equal(ga, wa) and np.array_equal(gb, wb) and np.array_equal(gf, wf), len(ids)
    eng.close()
    print("serial kernel: ok")
""")


def test_serial_kernel_in_a_fresh_process():
    """GS_HS_JDK_SERIAL=1 (read once per process) selects k_hs_jdk, one thread per set: the 200-key and the
    3000-key window equal the model there too.  One child process, while this one waits."""
    env = dict(os.environ, GS_HS_JDK_SERIAL="1")
    r = subprocess.run([sys.executable, "-c", SERIAL_CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"))],
                       capture_output=True, text=True, timeout=170, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "serial kernel: ok" in r.stdout
