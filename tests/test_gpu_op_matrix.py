"""GPU: every entry point after every other on one engine (the catalogue: tests/op_matrix.py).

One gs_ctx carries predictions from the previous window and scratch buffers its operators share by convention
("What a ctx carries between calls").  The suite checks each operator at its own edges; this module pins
what makes the shared ctx safe: a call's result depends only on its arguments and on its own state object, never on
what the ctx ran before.  Every call of every sequence is compared with the variant's CPU reference -- integers bit
for bit, float sums through valcheck.assert_values -- and a failure names the pair, the position and the previous call.

The engines are this module's own (not the session fixture), so the verdict is the same alone and inside the suite:
`shared` as created (stage timing on: every read-back through the stream), `lean` with GS_TIMING_OFF, where device
outputs take the asynchronous read-back."""
import numpy as np
import pytest
import torch

import op_matrix as M

pytestmark = pytest.mark.gpu

_DEVICE = {}


def _dev(x):
    """the column on the GPU, uploaded once (a batch is a slice of its variant's column: keyed by the memory it views)"""
    if not isinstance(x, np.ndarray):
        return x
    k = (x.ctypes.data, x.shape, x.dtype.str)
    if k not in _DEVICE:
        _DEVICE[k] = (x, torch.from_numpy(np.array(x)).cuda())
    return _DEVICE[k][1]


PUTS = {"host": M._host, "device": _dev}


@pytest.fixture(scope="module")
def shared(pkg):
    free0 = torch.cuda.mem_get_info()[0]
    eng = pkg.Engine(0)
    yield eng
    torch.cuda.synchronize()
    print(f"\nop matrix: the shared engine holds {(free0 - torch.cuda.mem_get_info()[0]) / 2**20:.0f} MiB at the end")
    eng.close()


@pytest.fixture(scope="module")
def lean(pkg):
    eng = pkg.Engine(0)
    eng.set_timing(pkg._lib.GS_TIMING_OFF)
    yield eng
    eng.close()


# ---- each variant alone reaches the path it is there for ---------------------------------------------------------
def _check_markers(v, run, t):
    m = v.markers
    third = run == 2
    if "path" in m:
        assert t.path == m["path"], (v.name, run, t.path)
    if "sort_passes" in m:
        assert t.sort_passes == m["sort_passes"], (v.name, run, t.sort_passes)
    if "packed_first" in m and run == 0:
        assert t.packed == m["packed_first"] and t.escapes > t.records // 8, (v.name, t.packed, t.escapes)
    if third and "key_bits" in m:   # (a fresh engine's first bucket window predicts all 2048 buckets)
        want = m["key_bits"]() if callable(m["key_bits"]) else m["key_bits"]
        assert t.key_bits == want, (v.name, t.key_bits, want)
    if third and "packed" in m:
        assert t.packed == m["packed"], (v.name, t.packed)
    if third and "speculative_third" in m:
        assert t.speculative == m["speculative_third"], (v.name, t.speculative)


@pytest.mark.parametrize("name", M.NAMES)
def test_solo(pkg, name):
    """A three times on a fresh engine; stage_times() shows the path the variant is in the catalogue for.
    degmax_far carries no speculative marker: its window goes through BkDeg32's histogram first, which rewrites the
    counts a speculation would size its regions from, so the wide policy never speculates on them with a hit; what
    shows the retry is the wide policy's bucket width (2^14 ids) in key_bits."""
    v = M.VARIANTS[name]
    with pkg.Engine(0) as eng:
        for run in range(3):
            M.run_sequence(eng, [name, name] if v.stateful else [name], _dev, label=f"solo {name} run {run}")
            if v.markers:
                _check_markers(v, run, eng.stage_times())


# ---- every ordered pair ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", M.NAMES)
def test_after(shared, a):
    """pair_sequence(A, B) for every B of the catalogue, host columns (staged through the ctx's input and output
    buffers) and device columns (outputs written in place)."""
    ran = 0
    for b in M.NAMES:
        for where, put in PUTS.items():
            M.run_sequence(shared, M.pair_sequence(a, b), put, label=f"pair ({a}, {b}), {where} columns")
        ran += 1
    assert ran == len(M.NAMES) == 40


def test_refused_call_ends_the_candidates_session(pkg):
    """The pair the matrix found: a reduce refused for its direction returned before begin_call, and the
    chunked-candidates session before it went on handing out records, where the header ends it at "any other entry
    point called on the ctx".  (The pair is part of test_after[err_cand_session]; here it runs on a fresh engine.)"""
    with pkg.Engine(0) as eng:
        for put in PUTS.values():
            M.run_sequence(eng, ["err_cand_session", "err_bad_direction"], put)
            M.run_sequence(eng, ["err_cand_session", "err_bad_direction", "err_bad_direction", "err_cand_session"], put)


def test_same_geometry_chain(pkg):
    """The three contents of one bucket geometry, in the order that walks the speculation and packing counters: a hit,
    a miss, eight windows without speculation, a hit again, a window of escapes, sixteen unpacked windows, packed
    again (the values of test_speculative_partition and test_packed_records_escapes: skip = 8, wide = 16)."""
    a, crowded, escapes = "reduce_i64_a", "reduce_i64_crowded", "reduce_i64_escapes"
    steps = ([(a, 0, True), (a, 1, True), (crowded, 2, True)] + [(a, 0, True)] * 8 + [(a, 1, True), (escapes, 1, True)]
             + [(a, 1, False)] * 16 + [(a, 1, True), (a, 1, True)])
    assert [n for n, _, _ in steps] == [a] * 2 + [crowded] + [a] * 9 + [escapes] + [a] * 17 + [a]
    with pkg.Engine(0) as eng:
        for at, (name, spec, packed) in enumerate(steps):
            M.run_sequence(eng, [name], _dev, label=f"chain step {at}")
            t = eng.stage_times()
            assert (t.path, t.speculative, t.packed) == (2, spec, packed), (at, name, t.speculative, t.packed)
            assert (t.escapes > t.records // 8) == (name == escapes), (at, t.escapes)


@pytest.mark.parametrize("e", M.ERRORS)
def test_after_error(shared, lean, e):
    """B, E, B for every non-error B: an API error leaves nothing behind."""
    for b in M.PLAIN:
        M.run_sequence(shared, [b, e, b], M._host, label=f"({b}, {e}, {b}), host columns")
        M.run_sequence(lean, [b, e, b], _dev, label=f"({b}, {e}, {b}), device columns, lean engine")


def test_tiny_tables_then_others(pkg, oracle):
    """The failing triangle call of test_triangle_table_overflow_is_an_error_not_a_hang, exactly as that test makes
    it (the kernels give up by design: GS_EDEVICE, no fault), then every variant that counts no triangles."""
    L = pkg._lib
    s, d = oracle.gen_rmat(14, 200_000, 0x5EED04, no_self_loops=True)
    S, D = (torch.from_numpy(x).cuda() for x in (s, d))
    others = [n for n in M.NAMES if M.VARIANTS[n].group != "triangles"]
    assert len(others) == len(M.NAMES) - 4
    with pkg.Engine(0, flags=L.GS_FLAG_TEST_TINY_TABLES) as eng:
        with pytest.raises(pkg.GsError) as ei:
            eng.triangles(S, D)
        assert ei.value.status == L.GS_EDEVICE and "hash set" in str(ei.value)
        M.run_sequence(eng, others, M._host, label="after the table overflow, host columns")
        with pytest.raises(pkg.GsError) as ei:
            eng.triangles(S, D)
        assert ei.value.status == L.GS_EDEVICE
        M.run_sequence(eng, others, _dev, label="after the table overflow, device columns")


@pytest.mark.parametrize("seed", range(4))
def test_walk(shared, lean, seed):
    eng, where = ((shared, "host"), (shared, "device"), (lean, "host"), (lean, "device"))[seed]
    M.run_sequence(eng, M.walk(seed, 200), PUTS[where], label=f"walk {seed}, {where} columns")


def test_async_readback_then_other_entry_point(pkg):
    """reduce_i64_a into device tensors with the asynchronous output on -- the call returns once the sizes are known,
    the emit kernel may still be writing -- followed at once, with no synchronize, by another entry point; then the
    reduce's tensors are read.  Both results are exact."""
    L = pkg._lib
    v = M.VARIANTS["reduce_i64_a"]
    s, d, val = (_dev(x) for x in v.inputs())
    out = (torch.empty(len(s), dtype=torch.int64, device="cuda"), torch.empty(len(s), dtype=torch.int64, device="cuda"))
    with pkg.Engine(0) as eng:   # torch_stream=True, async_outputs=True: the defaults
        eng.set_timing(L.GS_TIMING_OFF)
        for other in ("tri_b18", "cc_two_phase", "csr_all_f64"):
            how = []
            for _ in range(3):   # (the third window speculates: no host round trip before the read-back)
                for t in out:
                    t.fill_(-1)
                gk, gv = eng.reduce(s, d, val, M.OUT, M.SUM, out=out)
                how.append(eng.last_readback())
            M.run_sequence(eng, [other], _dev, label=f"{other} straight after an asynchronous reduce")
            M.same((gk, gv), v.expected(), where=f"reduce_i64_a before {other}")
            assert how[-1] != L.GS_READBACK_STREAM, how   # the window before `other` took the asynchronous read-back
