"""The catalogue of the cross-operator matrix (not a test module; imports neither torch nor the library).

Every call into the library goes through one gs_ctx, and the ctx carries more than a stream: predictions learned
from the previous window and scratch buffers the operators share by convention ("What a ctx carries
between calls").  The invariant that makes this safe -- a call's result depends only on its arguments and on its own
explicit state object, never on what the ctx ran before -- is what this catalogue is for:

  VARIANTS        name -> Variant: fixed seeded inputs (built lazily, once per process), `expected` computed once on
                  the CPU from the references the suite already trusts, a `precondition` that says in code which
                  state of the ctx the inputs reach, and `first(engine, put, inputs)` [/ `second(token, intervened, inputs)`].
  pair_sequence   [A, B, B, A, A, B]: A->B, B->B, B->A, A->A and A->B again.
  walk            a seeded random walk over the non-error variants.
  run_sequence    runs a sequence of names on one engine and checks every call against `expected`; a failure names
                  the sequence, the position and the previous call.

A variant with a device-resident state (and the candidates session) has two halves: `first` creates the state and
feeds batch 1, `second` feeds batch 2, checks both outputs and the export, and closes.  In a sequence the two halves
take the successive places of the variant's name, so the other variant of a pair runs inside its stream; a state
still open at the end of a sequence is closed by one more `second`.

`engine` is the package's Engine or a ModelEngine (tests/test_op_matrix_ref.py) with the same methods; `put` turns a
numpy column into what the engine is given (the identity: host columns; the GPU tests also pass device tensors).
Two calls the Engine class has no method for -- an output one row short through the C ABI -- go through
reduce_short_then_fetch / components_short, which use the engine's own method of that name when it has one.

Sizes are the smallest that still reach the state each variant is there for; no window has more than 70 000 edges.
"""
from __future__ import annotations

import ctypes
import functools
import importlib
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

import assign_ref
import continuous_ref
import distinct_ref
import matching_ref
import textparse_ref
import trisample_ref
from bipartite_cpu import canonical
from idmaps import DIRECT_BITS, id_span, mask_bits, maps, pin_ends
from valcheck import assert_values

IN, OUT, ALL = 0, 1, 2
SUM, MIN, MAX, COUNT = 0, 1, 2, 3
GS_EINVAL, GS_ECAPACITY, GS_EDEVICE = -1, -2, -3

# thresholds read from the code (tests/test_op_matrix_ref.py asserts the inputs against them)
BK_MAXB = 2048            # gs_bucket.hpp: buckets of 2^S ids
S_LONG, S_NARROW, S_DEGREE = 14, 15, 13   # BkVal 8-byte accumulators / 4-byte and COUNT / BkDeg32
SORT_TILE = 8192          # gs_ops.hpp: records per tile of the window sort
UF_TWO_PHASE = 65536      # gs_cc_common.hpp uf_window: records from which the unions run in two phases
TRI_PARTITIONED_V = 1 << 23   # gs_triangles.hip: partitioned okeys above this many ids
TRI_FUSED_2B = 32         # gs_triangles.hip: the fused unique from 2B > 32
PACK_LIMIT = 0xFFFF       # k_dp_scatter_pack: values in [0, 0xFFFF) travel in 16 bits


def _oracle():
    import __graft_entry__ as ge
    return ge.load_oracle()


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _np(x):
    """a result column as numpy (device tensors come back through .cpu())"""
    if x is None or isinstance(x, (int, bool, str)):
        return x
    if hasattr(x, "cpu"):
        return x.cpu().numpy()
    return np.asarray(x)


def _norm(x):
    if isinstance(x, (tuple, list)):
        return tuple(_norm(y) for y in x)
    if isinstance(x, dict):
        return tuple(sorted((k, int(v)) for k, v in x.items()))
    if isinstance(x, np.generic):
        return x.item()
    return _np(x)


def same(got, want, float_sum=None, where="result"):
    """got == want, item by item: scalars equal, integer arrays bit for bit with the reference's dtype; float_sum =
    (dtype, op): float arrays through valcheck.assert_values, as everywhere else in the suite."""
    got, want = _norm(got), _norm(want)
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == len(want), f"{where}: {len(got) if isinstance(got, tuple) else got!r} items, the reference has {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, float_sum, f"{where}[{i}]")
        return
    if isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray), f"{where}: {type(got).__name__}, the reference is an array"
        assert got.shape == want.shape, f"{where}: {got.shape} rows, the reference has {want.shape}"
        assert got.dtype == want.dtype, f"{where}: dtype {got.dtype}, the reference is {want.dtype}"
        if np.issubdtype(want.dtype, np.floating):
            dtype, op = float_sum if float_sum else (want.dtype, MIN)   # no float_sum: bit for bit
            assert_values(got, want, dtype, op)
        elif not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{where}: {len(bad)} of {len(want)} rows differ, first [{bad[0]}] got {got[bad[0]]!r} "
                                 f"want {want[bad[0]]!r}")
        return
    assert got == want, f"{where}: got {got!r}, want {want!r}"


class Raised(Exception):
    pass


def status_of(fn) -> int:
    """the status of the error fn() raises (GsError and the model's error both carry .status)"""
    try:
        fn()
    except Exception as e:   # noqa: BLE001 -- any error class with a status
        st = getattr(e, "status", None)
        if st is None:
            raise
        return int(st)
    raise Raised("the call returned; an error status was expected")


@dataclass
class Variant:
    name: str
    group: str                      # bucket / sort / csr / triangles / candidates / unionfind / other / state / error
    inputs: Callable[[], tuple]     # lazily built, cached
    expected: Callable[[], object]  # lazily built from the CPU references, cached
    first: Callable                 # (engine, put, inputs) -> result, or (state variants) a token
    precondition: Callable[[], None]
    second: Callable | None = None  # (token, intervened, inputs) -> result
    float_sum: tuple | None = None
    markers: dict = field(default_factory=dict)   # what stage_times() shows when the variant reaches its path
    nontrivial: Callable | None = None            # (expected) -> None, asserts

    @property
    def stateful(self) -> bool:
        return self.second is not None

    @property
    def error(self) -> bool:
        return self.group == "error"


VARIANTS: dict[str, Variant] = {}


def _variant(name, group, inputs, expected, first, precondition, **kw):
    assert name not in VARIANTS
    VARIANTS[name] = Variant(name, group, functools.lru_cache(maxsize=None)(inputs),
                             functools.lru_cache(maxsize=None)(expected), first, precondition, **kw)


def _key_columns(s, d, direction):
    return {IN: (d, d), OUT: (s, s), ALL: (s, d)}[direction]


def _bucket_precondition(get, direction, S, buckets=None):
    def check():
        s, d = get()[:2]
        span = id_span(*_key_columns(s, d, direction))
        nb = (span >> S) + 1
        assert 1 < nb < BK_MAXB, (span, S, nb)
        if buckets is not None:
            assert nb == buckets, (nb, buckets)
    return check


# ---- the bucket path ------------------------------------------------------------------------------------------
N_BK = 40_000


def _uniform(seed, n, span, off=0):
    """n edges over [off, off + span), both ends of the range in both columns"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, span, n).astype(np.int64)
    d = rng.integers(0, span, n).astype(np.int64)
    s[0], s[1], d[0], d[1] = 0, span - 1, span - 1, 0
    return s + off, d + off, rng


def _reduce_variant(name, group, make, direction, op, precondition, markers, float_sum=None, init=None):
    def expected():
        s, d, v = make()
        o = _oracle()
        if init is None:
            return o.window_reduce(s, d, v, direction, op)
        return o.window_fold(s, d, v, direction, op, init)

    def first(engine, put, inp):
        s, d, v = (put(x) for x in inp)
        if init is None:
            return engine.reduce(s, d, v, direction, op)
        return engine.fold(s, d, v, direction, op, init)

    _variant(name, group, make, expected, first, precondition, markers=markers, float_sum=float_sum,
             nontrivial=lambda e: _rows_nontrivial(e, 1000))


def _rows_nontrivial(e, at_least):
    assert len(e[0]) >= at_least and np.all(e[0][1:] > e[0][:-1])
    assert len(np.unique(e[1])) > 1


def _i64_a():
    s, d, rng = _uniform(0xA001, N_BK, 1 << 18)
    return _frozen(s, d, rng.integers(0, PACK_LIMIT, N_BK).astype(np.int64))


def _i64_crowded():
    s, d, rng = _uniform(0xA002, N_BK, 1 << 18)
    # half the records in bucket 0, at positions spread over the whole window: regions sized from _a's counts
    # overflow, regions sized from this window's own counts hold (every XCD slot's tiles see the same mix)
    s[rng.permutation(np.arange(2, N_BK))[:N_BK // 2]] = 12345
    return _frozen(s, d, rng.integers(0, PACK_LIMIT, N_BK).astype(np.int64))


def _i64_escapes():
    s, d, rng = _uniform(0xA003, N_BK, 1 << 18)
    return _frozen(s, d, rng.integers(-(1 << 30), -1, N_BK).astype(np.int64))   # every value escapes: > R / 8


def _packed_values(get, escaping):
    def check():
        v = get()[2]
        esc = int(np.sum((v < 0) | (v >= PACK_LIMIT)))
        assert (esc > len(v) // 8) == escaping and (escaping or esc == 0)
    return check


def _both(*checks):
    def check():
        for c in checks:
            c()
    return check


def _crowded_check():
    s = _i64_crowded()[0]
    assert int(np.sum((s >> S_LONG) == 0)) >= N_BK // 2   # one of 16 buckets holds half the records


_SAME_GEOMETRY = dict(path=2, key_bits=S_LONG + 4, speculative_third=1)
_reduce_variant("reduce_i64_a", "bucket", _i64_a, OUT, SUM,
                _both(_bucket_precondition(_i64_a, OUT, S_LONG, 16), _packed_values(_i64_a, False)),
                dict(_SAME_GEOMETRY, packed=True))
_reduce_variant("reduce_i64_crowded", "bucket", _i64_crowded, OUT, SUM,
                _both(_bucket_precondition(_i64_crowded, OUT, S_LONG, 16), _packed_values(_i64_crowded, False),
                      _crowded_check), dict(_SAME_GEOMETRY, packed=True))
_reduce_variant("reduce_i64_escapes", "bucket", _i64_escapes, OUT, SUM,
                _both(_bucket_precondition(_i64_escapes, OUT, S_LONG, 16), _packed_values(_i64_escapes, True)),
                dict(_SAME_GEOMETRY, packed_first=True, packed=False))


def _f64_all():
    s, d, rng = _uniform(0xA004, N_BK, 1 << 20)
    return _frozen(s, d, (rng.random(N_BK) * 100).astype(np.float64))


_reduce_variant("reduce_f64_all", "bucket", _f64_all, ALL, SUM, _bucket_precondition(_f64_all, ALL, S_LONG, 64),
                dict(path=2, key_bits=S_LONG + 6, speculative_third=1, packed=False), float_sum=(np.float64, SUM))


def _i32_min_in():
    s, d, rng = _uniform(0xA005, N_BK, 1 << 17, -(1 << 40))
    return _frozen(s, d, rng.integers(0, PACK_LIMIT, N_BK).astype(np.int32))


def _base_misses():
    d = _i32_min_in()[1]
    assert int(d.min()) < -(1 << 39)   # nowhere near the base any other variant leaves behind


_reduce_variant("reduce_i32_min_in", "bucket", _i32_min_in, IN, MIN,
                _both(_bucket_precondition(_i32_min_in, IN, S_NARROW, 4), _base_misses),
                dict(path=2, key_bits=S_NARROW + 2, speculative_third=1, packed=True))


def _count_out():
    s, d, rng = _uniform(0xA006, N_BK, 1 << 19)
    return _frozen(s, d, np.zeros(N_BK, np.int64))


_reduce_variant("reduce_count_out", "bucket", _count_out, OUT, COUNT, _bucket_precondition(_count_out, OUT, S_NARROW, 16),
                dict(path=2, key_bits=S_NARROW + 4, speculative_third=1, packed=False))


def _fold_in():
    s, d, rng = _uniform(0xA007, N_BK, 1 << 18)
    return _frozen(s, d, _oracle().gen_values(N_BK, 0xA007, _oracle().DT_I64))


_reduce_variant("fold_i64_in_init", "bucket", _fold_in, IN, SUM, _bucket_precondition(_fold_in, IN, S_LONG, 16),
                dict(path=2, key_bits=S_LONG + 4, speculative_third=1), init=-77)


def _degmax_variant(name, make, direction, precondition, markers):
    def expected():
        s, d = make()
        return _oracle().window_fold_degree_max(s, d, direction)

    def first(engine, put, inp):
        s, d = (put(x) for x in inp)
        return engine.fold_degree_max(s, d, direction)

    _variant(name, "bucket", make, expected, first, precondition, markers=markers,
             nontrivial=lambda e: _rows_nontrivial(e, 1000))


def _degmax_all():
    s, d, _ = _uniform(0xA008, N_BK, 1 << 17)
    return _frozen(s, d)


def _degmax_far():
    s, d, _ = _uniform(0xA009, N_BK, 1 << 17)
    d[::7] += 1 << 40   # keys (OUT: the sources) stay in range; these neighbours leave base + 2^32
    return _frozen(s, d)


def _far_neighbours():
    s, d = _degmax_far()
    assert int(d.max()) - int(s.min()) >= 1 << 32


_degmax_variant("degmax_all", _degmax_all, ALL, _bucket_precondition(_degmax_all, ALL, S_DEGREE, 16),
                dict(path=2, key_bits=S_DEGREE + 4, speculative_third=1))
_degmax_variant("degmax_far", _degmax_far, OUT,
                _both(_bucket_precondition(_degmax_far, OUT, S_DEGREE, 16), _bucket_precondition(_degmax_far, OUT, S_LONG, 8),
                      _far_neighbours), dict(path=2, key_bits=S_LONG + 3))   # BkDeg's 2^14-id buckets: the wide policy answered


# ---- the sort path --------------------------------------------------------------------------------------------
def _sort_precondition(get, direction, S, wide):
    def check():
        s, d = get()[:2]
        ks, kd = _key_columns(s, d, direction)
        assert (id_span(ks, kd) >> S) >= BK_MAXB       # past the bucket path's range
        bits = mask_bits(ks, kd)
        assert bits > 32 if wide else 24 < bits <= 32   # 64-bit keys / 32-bit keys in four passes
    return check


def _i64_wide():
    s, d, rng = _uniform(0xA00A, N_BK, 1 << 40)
    return _frozen(s, d, _oracle().gen_values(N_BK, 0xA00A, _oracle().DT_I64))


def _f32_narrow4():
    s, d, rng = _uniform(0xA00B, N_BK, 1 << 30)
    return _frozen(s, d, (rng.random(N_BK) * 100).astype(np.float32))


_reduce_variant("reduce_i64_wide", "sort", _i64_wide, OUT, SUM, _sort_precondition(_i64_wide, OUT, S_LONG, True),
                dict(path=0, key_bits=40, sort_passes=5))
_reduce_variant("reduce_f32_narrow4", "sort", _f32_narrow4, OUT, SUM, _sort_precondition(_f32_narrow4, OUT, S_NARROW, False),
                dict(path=0, key_bits=30, sort_passes=4), float_sum=(np.float32, SUM))


# ---- CSR: always sort_window(PAY_IDX); the only output that shows a stability error ------------------------------
N_CSR, CSR_HUB = 20_000, 9_000


def _csr_columns(seed, ids, hub_column):
    """20 000 edges over the ids; one vertex holds 9 000 records of `hub_column` at random positions"""
    rng = np.random.default_rng(seed)
    s, d = ids[rng.integers(0, len(ids), N_CSR)], ids[rng.integers(0, len(ids), N_CSR)]
    s[0], d[0] = ids[0], ids[-1]
    hub = ids[len(ids) // 3]
    (s if hub_column == "src" else d)[rng.permutation(np.arange(1, N_CSR))[:CSR_HUB]] = hub
    return s, d, rng, hub


def _csr_variant(name, make, direction, precondition, markers):
    def expected():
        s, d, v = make()[:3]
        return _oracle().window_csr(s, d, v, direction)

    def first(engine, put, inp):
        s, d, v = inp[:3]
        return engine.csr(put(s), put(d), None if v is None else put(v), direction)

    def nontrivial(e):
        assert len(e[0]) > 1 and int(np.max(np.diff(e[1]))) > SORT_TILE

    _variant(name, "csr", make, expected, first, precondition, markers=markers, nontrivial=nontrivial)


def _csr_hub(get, direction, bits=None):
    def check():
        s, d, _, hub = get()
        ks, kd = _key_columns(s, d, direction)
        cols = (ks,) if direction != ALL else (ks, kd)
        assert sum(int(np.sum(c == hub)) for c in cols) > SORT_TILE   # the hub's run crosses sort tiles
        if bits is not None:
            assert bits(mask_bits(ks, kd))
    return check


def _csr_out_i32():
    s, d, rng, hub = _csr_columns(0xC001, np.arange(200, dtype=np.int64), "src")
    return _frozen(s, d, rng.integers(-(1 << 31), 1 << 31, N_CSR).astype(np.int32)) + (int(hub),)


def _csr_all_f64():
    rng = np.random.default_rng(0xC012)
    ids = np.unique(np.concatenate([[0, (1 << 20) - 1], rng.integers(0, 1 << 20, 5000)])).astype(np.int64)
    s, d, rng, hub = _csr_columns(0xC002, ids, "src")
    return _frozen(s, d, rng.standard_normal(N_CSR).astype(np.float64)) + (int(hub),)


def _csr_in_wide():
    ids = np.arange(1 << 12, dtype=np.int64) * ((1 << 51) + 1) - (1 << 62)   # spread over the whole int64 range
    s, d, rng, hub = _csr_columns(0xC003, ids, "dst")
    return _frozen(s, d) + (None, int(hub))


_csr_variant("csr_out_i32", _csr_out_i32, OUT, _csr_hub(_csr_out_i32, OUT, lambda b: b <= 8), dict(path=0, sort_passes=1))
_csr_variant("csr_all_f64", _csr_all_f64, ALL, _csr_hub(_csr_all_f64, ALL, lambda b: b == 20), dict(path=0, key_bits=20))
_csr_variant("csr_in_wide", _csr_in_wide, IN,
             _both(_csr_hub(_csr_in_wide, IN, lambda b: b > 32), lambda: _negative(_csr_in_wide()[1])), dict(path=0))


def _negative(col):
    assert int(col.min()) < 0 < int(col.max())


# ---- triangles ------------------------------------------------------------------------------------------------
def _tri_variant(name, make, loops, precondition, markers):
    def expected():
        s, d = make()
        o = _oracle()
        if loops:
            w, ex, has, _ = o.window_triangles_ref(s, d)
        else:
            w, ex, has = o.window_triangles_fwd(s, d)
        return ex, w, has

    def first(engine, put, inp):
        s, d = (put(x) for x in inp)
        return engine.triangles(s, d)

    def nontrivial(e):
        assert e[0] > 0 and e[2]

    _variant(name, "triangles", make, expected, first, precondition, markers=markers, nontrivial=nontrivial)


def _tri_bits(get, bits, loops=False):
    def check():
        s, d = get()
        assert mask_bits(s, d) == bits
        assert bool(np.any(s == d)) == loops
        if bits <= DIRECT_BITS:
            assert id_span(s, d) < (1 << bits)
    return check


def _tri_b14_loops():
    return _frozen(*pin_ends(*_oracle().gen_rmat(14, 30_000, 0x7B14), 14, at=3))


def _tri_b18():
    return _frozen(*pin_ends(*_oracle().gen_rmat(18, 60_000, 0x7B18, no_self_loops=True), 18))


def _tri_b24():
    s, d = pin_ends(*_oracle().gen_rmat(12, 60_000, 0x7B24, no_self_loops=True), 12)
    f = maps(12)["spread_2p24"]
    return _frozen(f(s), f(d))


def _tri_relabel():
    s, d = pin_ends(*_oracle().gen_rmat(12, 40_000, 0x7B12, no_self_loops=True), 12)
    f = maps(12)["sparse"]
    return _frozen(f(s), f(d))


def _tri_relabel_check():
    s, d = _tri_relabel()
    assert mask_bits(s, d) > DIRECT_BITS and int(s.min()) == -(1 << 61)   # x * 7_919_000_003 - 2^61 from x = 0


def _compact_bits(s, d):
    return max(1, (len(np.unique(np.concatenate([s, d]))) - 1).bit_length())


_variant_tri = [
    ("tri_b14_loops", _tri_b14_loops, True, _both(_tri_bits(_tri_b14_loops, 14, True), lambda: _unfused(14)), dict(path=3, key_bits=14)),
    ("tri_b18", _tri_b18, False, _both(_tri_bits(_tri_b18, 18), lambda: _fused(18)), dict(path=3, key_bits=18)),
    ("tri_b24", _tri_b24, False, _both(_tri_bits(_tri_b24, 24), lambda: _fused(24), lambda: _partitioned(24)), dict(path=3, key_bits=24)),
    ("tri_relabel", _tri_relabel, False, _tri_relabel_check, dict(path=3, key_bits=lambda: _compact_bits(*_tri_relabel()))),
]


def _unfused(B):
    assert 2 * B <= TRI_FUSED_2B


def _fused(B):
    assert 2 * B > TRI_FUSED_2B


def _partitioned(B):
    assert (1 << B) > TRI_PARTITIONED_V


for _args in _variant_tri:
    _tri_variant(*_args)


# ---- candidates -----------------------------------------------------------------------------------------------
def _cand_sparse():
    s, d = pin_ends(*_oracle().gen_rmat(10, 2_000, 0xCA01), 10)
    f = maps(10)["sparse"]
    return _frozen(f(s), f(d))


def _cand_records():
    """GenerateCandidateEdges records of an s10 window: the input of stage 2"""
    s, d = _oracle().gen_rmat(10, 3_000, 0xCA02)
    a, b, f, _ = _oracle().window_candidates(s, d)
    return _frozen(a, b, f)


def _cand_count_graph():
    return _frozen(*_oracle().gen_rmat(11, 4_000, 0xCA03))


def _candidates_first(engine, put, inp):
    s, d = (put(x) for x in inp)
    a, b, f = engine.candidates(s, d)
    return a, b, f, int(engine.last_candidates_jdk_flags)


def _count_candidates_expected():
    w, ex, has, groups = _oracle().count_candidates(*_cand_records())
    return ex, w, has, groups


_variant("candidates_sparse", "candidates", _cand_sparse, lambda: _oracle().window_candidates(*_cand_sparse()),
         _candidates_first, lambda: _sparse_ids(_cand_sparse()), nontrivial=lambda e: _cand_nontrivial(e))
_variant("count_candidates", "candidates", _cand_records, _count_candidates_expected,
         lambda engine, put, inp: engine.count_candidates(*(put(x) for x in inp)),
         lambda: _has_both_kinds(_cand_records()[2]), nontrivial=lambda e: _count_nontrivial(e))
_variant("candidate_count", "candidates", _cand_count_graph, lambda: _oracle().candidate_count(*_cand_count_graph()),
         lambda engine, put, inp: engine.candidate_count(*(put(x) for x in inp)),
         lambda: _sized(_cand_count_graph()[0], 4_000), nontrivial=lambda e: _positive(e, 4_000))


def _sparse_ids(cols):
    s, d = cols
    assert len(s) <= 2_000 and mask_bits(s, d) > 32 and id_span(s, d) >= 1 << 32


def _cand_nontrivial(e):
    assert len(e[0]) > 2_000 and 0 < int(e[2].sum()) < len(e[2])


def _has_both_kinds(f):
    assert 0 < int(f.sum()) < len(f)


def _count_nontrivial(e):
    assert e[0] > 0 and e[2] and e[3] > 0


def _sized(col, n):
    assert len(col) == n


def _positive(e, more_than):
    assert e > more_than


# ---- union-find: ConnectedComponents and BipartitenessCheck ---------------------------------------------------
def _cc_variant(name, make, precondition, markers):
    def expected():
        s, d, prev = make()
        return _oracle().components(s, d, prev)

    def first(engine, put, inp):
        s, d, prev = inp
        return engine.components(put(s), put(d), None if prev is None else tuple(put(x) for x in prev))

    def nontrivial(e):
        assert len(e[0]) > 100 and 1 < len(np.unique(e[1])) < len(e[0])

    _variant(name, "unionfind", make, expected, first, precondition, markers=markers, nontrivial=nontrivial)


def _cc_small():
    return _frozen(*pin_ends(*_oracle().gen_rmat(12, 5_000, 0xCC01), 12)) + (None,)


def _cc_two_phase():
    return _frozen(*pin_ends(*_oracle().gen_rmat(16, 70_000, 0xCC02), 16)) + (None,)


def _cc_relabel_state():
    s, d = pin_ends(*_oracle().gen_rmat(12, 8_000, 0xCC03), 12)
    f = maps(12)["sparse"]
    s, d = f(s), f(d)
    prev = _oracle().components(s[:4_000], d[:4_000])
    return _frozen(s[4_000:].copy(), d[4_000:].copy()) + (_frozen(*prev),)


def _uf_records(get, direct, two_phase, bits=None):
    def check():
        s, d, prev = get()[:3]
        records = len(s) + (len(prev[0]) if prev is not None else 0)
        assert (records >= UF_TWO_PHASE) == two_phase
        cols = (s, d) if prev is None else (np.concatenate([s, prev[0]]), np.concatenate([d, prev[1]]))
        b = mask_bits(*cols)
        assert (b <= DIRECT_BITS) == direct
        if bits is not None:
            assert b == bits
    return check


_cc_variant("cc_small", _cc_small, _uf_records(_cc_small, True, False, 12), dict(path=4, key_bits=12))
_cc_variant("cc_two_phase", _cc_two_phase, _uf_records(_cc_two_phase, True, True, 16), dict(path=4, key_bits=16))
_cc_variant("cc_relabel_state", _cc_relabel_state,
            _both(_uf_records(_cc_relabel_state, False, False), lambda: _has_state(_cc_relabel_state()[2])),
            dict(path=4, key_bits=0))


def _has_state(prev):
    assert prev is not None and len(prev[0]) > 100


def _bip_variant(name, make, precondition, markers, fails=False):
    def expected():
        s, d = make()[:2]
        return canonical(s, d)

    def first(engine, put, inp):
        s, d = inp[:2]
        return engine.bipartite(put(s), put(d))

    def nontrivial(e):
        if fails:
            assert e[0] is False and all(len(x) == 0 for x in e[1:])
        else:
            assert e[0] is True and len(e[1]) > 100 and 0 < int(e[3].sum()) < len(e[3])

    _variant(name, "unionfind", make, expected, first, precondition, markers=markers, nontrivial=nontrivial)


def _bip_graph(K, n, seed):
    """R-MAT made bipartite (2x, 2x + 1): base ids in [0, 2^(K + 1))"""
    s, d = _oracle().gen_rmat(K, n, seed)
    return pin_ends(s * 2, d * 2 + 1, K + 1)


def _bip_two_phase():
    return _frozen(*_bip_graph(15, 70_000, 0xB101)) + (None,)


def _bip_relabel():
    s, d = _bip_graph(11, 5_000, 0xB102)
    f = maps(12)["sparse"]
    return _frozen(f(s), f(d)) + (None,)


def _bip_odd_cycle():
    """one edge between two vertices on the same side of the largest component, at a seeded position"""
    s, d = _bip_graph(11, 5_000, 0xB103)
    _, v, lab, sign = canonical(s, d)
    labels, counts = np.unique(lab, return_counts=True)
    side = v[(lab == labels[np.argmax(counts)]) & (sign == 1)]
    rng = np.random.default_rng(0xB103)
    a, b = rng.choice(side, 2, replace=False)
    at = int(rng.integers(1, len(s) + 1))
    return _frozen(np.insert(s, at, a), np.insert(d, at, b)) + (None,)


_bip_variant("bip_two_phase", _bip_two_phase, _uf_records(_bip_two_phase, True, True, 16), dict(path=5, key_bits=16))
_bip_variant("bip_relabel", _bip_relabel, _uf_records(_bip_relabel, False, False), dict(path=5, key_bits=0))
_bip_variant("bip_odd_cycle", _bip_odd_cycle, _uf_records(_bip_odd_cycle, True, False, 12), dict(path=5, key_bits=12), fails=True)


# ---- others ---------------------------------------------------------------------------------------------------
def _text():
    s, d = _oracle().gen_rmat(14, 3_000, 0x7E01)
    t = np.random.default_rng(0x7E01).integers(-(1 << 62), 1 << 62, 3_000)
    return ("".join(f"{a} {b} {c}\n" for a, b, c in zip(s.tolist(), d.tolist(), t.tolist())).encode(),)


def _text_check():
    text = _text()[0]
    cols, bad = textparse_ref.parse(text)
    assert bad is None and len(cols[0]) == 3_000
    assert int(cols[2].min()) < 0   # signed fields


_variant("parse_text", "other", _text, lambda: _oracle().parse_edges_text(_text()[0]),
         lambda engine, put, inp: engine.parse_edges_text(inp[0], out_device=put is not _host),
         _text_check, nontrivial=lambda e: _sized(e[0], 3_000))


def _host(x):
    return x


NPARTS = 4


def _partials_first(engine, put, inp):
    """two slices through reduce_partials at nparts = 4; every owner merges what the two slices hold for it"""
    s, d, v = inp
    half = len(s) // 2
    slices = []
    for a, b in ((0, half), (half, len(s))):
        k, p, counts = engine.reduce_partials(put(s[a:b]), put(d[a:b]), put(v[a:b]), ALL, SUM, NPARTS)
        assert len(counts) == NPARTS and sum(counts) == len(k), (counts, len(k))
        slices.append((_np(k), _np(p), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)))
    keys, vals = [], []
    for owner in range(NPARTS):
        k = np.concatenate([ks[off[owner]:off[owner + 1]] for ks, _, off in slices])
        p = np.concatenate([ps[off[owner]:off[owner + 1]] for _, ps, off in slices])
        mk, mv = engine.merge_partials(put(k), put(p), SUM)
        mk, mv = _np(mk), _np(mv)
        assert np.all(mk[1:] > mk[:-1]), f"owner {owner}: merged keys not ascending"
        keys.append(mk)
        vals.append(mv)
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    order = np.argsort(keys, kind="stable")
    return keys[order], vals[order]


def _partials_inputs():
    s, d, rng = _uniform(0xD001, N_BK, 1 << 18)
    return _frozen(s, d, _oracle().gen_values(N_BK, 0xD001, _oracle().DT_I64))


_variant("partials_merge", "other", _partials_inputs,
         lambda: _oracle().window_reduce(*_partials_inputs(), ALL, SUM), _partials_first,
         _bucket_precondition(_partials_inputs, ALL, S_LONG, 16), nontrivial=lambda e: _rows_nontrivial(e, 1000))

CHUNK_RECORDS = 10_000


def _chunked_first(engine, put, inp):
    s, d, v = (put(x) for x in inp)
    engine.set_max_window_records(CHUNK_RECORDS)
    try:
        return engine.reduce(s, d, v, ALL, SUM)
    finally:
        engine.set_max_window_records(0)


def _chunked_inputs():
    s, d, rng = _uniform(0xD002, N_BK, 1 << 18)
    return _frozen(s, d, _oracle().gen_values(N_BK, 0xD002, _oracle().DT_I64))


def _chunked_check():
    assert 2 * len(_chunked_inputs()[0]) >= 4 * CHUNK_RECORDS   # several chunks and several merges


_variant("reduce_chunked", "other", _chunked_inputs, lambda: _oracle().window_reduce(*_chunked_inputs(), ALL, SUM),
         _chunked_first, _both(_bucket_precondition(_chunked_inputs, ALL, S_LONG, 16), _chunked_check),
         nontrivial=lambda e: _rows_nontrivial(e, 1000))


# ---- device-resident states: two batches of 4000 edges ----------------------------------------------------------
N_STATE = 4_000


def _columns(rows, dtypes):
    """a list of tuples -> one array per column"""
    return tuple(np.array([r[i] for r in rows], dtype=dt) for i, dt in enumerate(dtypes))


def _state_variant(name, make, expected, create, feed, export, precondition, nontrivial):
    """first: create + batch 1; second: batch 2, the export, close -> (output 1, output 2, export)"""
    def first(engine, put, inp):
        st = create(engine)
        try:
            return {"state": st, "put": put, "out1": _norm(feed(st, put, inp, 0))}
        except BaseException:
            st.close()
            raise

    def second(token, intervened, inp):
        st = token["state"]
        try:
            out2 = _norm(feed(st, token["put"], inp, 1))
            return token["out1"], out2, _norm(export(st))
        finally:
            st.close()

    _variant(name, "state", make, expected, first, precondition, second=second, nontrivial=nontrivial)


def _batch(inp, i):
    return tuple(None if c is None else c[i * N_STATE:(i + 1) * N_STATE] for c in inp)


def _state_edges(seed, V, vals=False):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, V, 2 * N_STATE).astype(np.int64), rng.integers(0, V, 2 * N_STATE).astype(np.int64)
    return _frozen(s, d) + (_frozen(rng.integers(1, 1 << 20, 2 * N_STATE).astype(np.int64)) if vals else ())


def _two_batches(get, columns=2, adds=True):
    def check():
        inp = get()
        assert len(inp) == columns and all(len(c) == 2 * N_STATE for c in inp)
        first, second = (set(np.concatenate([c[a:a + N_STATE] for c in inp[:2]]).tolist()) for a in (0, N_STATE))
        assert first & second   # batch 2 meets the vertices batch 1 left in the state
        assert bool(second - first) == adds   # and brings new ones (the samplers: every vertex is known by then)
    return check


def _cont_inputs():
    return _state_edges(0x5701, 3_000)


def _cont_expected():
    s, d = _cont_inputs()
    ref = continuous_ref.DegreeState()
    outs = [_columns(ref.degrees(*_batch((s, d), i), ALL), (np.int64, np.int64)) for i in range(2)]
    return outs[0], outs[1], _columns(ref.export(), (np.int64, np.int64))


_state_variant("cont_degrees_all", _cont_inputs, _cont_expected, lambda e: e.continuous(),
               lambda st, put, inp, i: st.degrees(*(put(c) for c in _batch(inp, i)), ALL), lambda st: st.export(),
               _two_batches(_cont_inputs), lambda e: _sized(e[1][0], 2 * N_STATE))


def _distinct_inputs():
    return _state_edges(0x5702, 64, vals=True)


def _distinct_expected():
    s, d, v = _distinct_inputs()
    ref = distinct_ref.DistinctState(distinct_ref.KEYED)
    dts = (np.int64, np.int64, np.int64, np.int64)
    outs = [_columns(ref.edges(*_batch((s, d, v), i)), dts) for i in range(2)]
    return outs[0], outs[1], _columns(ref.log, (np.int64, np.int64))


def _distinct_nontrivial(e):
    assert 0 < len(e[1][0]) < len(e[0][0]) < N_STATE   # duplicates inside batch 1, and batch 2 mostly seen before


_state_variant("distinct_keyed", _distinct_inputs, _distinct_expected, lambda e: e.distinct("keyed"),
               lambda st, put, inp, i: st.edges(*(put(c) for c in _batch(inp, i))), lambda st: st.export(),
               _two_batches(_distinct_inputs, 3, adds=False), _distinct_nontrivial)


def _matching_inputs():
    return _state_edges(0x5703, 2_000, vals=True)


def _matching_expected():
    s, d, v = _matching_inputs()
    ref = matching_ref.FastMatching()
    dts = (np.uint8, np.int64, np.int64, np.int64, np.int64)
    outs = [_columns(ref.edges(*_batch((s, d, v), i)), dts) for i in range(2)]
    assert ref.is_matching()
    return outs[0], outs[1], _columns(ref.export(), (np.int64, np.int64, np.int64))


def _matching_nontrivial(e):
    for out in e[:2]:
        assert int(np.sum(out[0] == matching_ref.REMOVE)) > 0 and int(np.sum(out[0] == matching_ref.ADD)) > 0
    assert len(e[2][0]) > 100


_state_variant("matching", _matching_inputs, _matching_expected, lambda e: e.weighted_matching(),
               lambda st, put, inp, i: st.edges(*(put(c) for c in _batch(inp, i))), lambda st: st.export(),
               _two_batches(_matching_inputs, 3), _matching_nontrivial)


def _assign_inputs():
    return _state_edges(0x5704, 6_000)


def _assign_expected():
    s, d = _assign_inputs()
    ref, outs = assign_ref.AssignFast(), []
    for i in range(2):
        rec, ref = assign_ref.run(list(zip(*(c.tolist() for c in _batch((s, d), i)))), ref)
        outs.append(_columns(rec, (np.int64, np.int64, np.uint32)))
    return outs[0], outs[1], _columns(sorted(ref.state().items()), (np.int64, np.int64))


def _assign_nontrivial(e):
    assert len(e[0][0]) > 1_000 and len(e[1][0]) > 1_000 and len(e[1][0]) != len(e[0][0])
    assert len(np.unique(e[2][1])) > 1


_state_variant("assign", _assign_inputs, _assign_expected, lambda e: e.assign_components(),
               lambda st, put, inp, i: st.edges(*(put(c) for c in _batch(inp, i))), lambda st: st.export(),
               _two_batches(_assign_inputs), _assign_nontrivial)

TS_SAMPLES, TS_VERTICES, TS_SEED = 200, 60, 99


def _trisample_inputs():
    return _state_edges(0x5705, TS_VERTICES)


def _trisample_expected():
    s, d = _trisample_inputs()
    ref = trisample_ref.TriangleSamplerRef("broadcast", TS_SAMPLES, TS_VERTICES, seed=TS_SEED)
    outs = [_columns(ref.edges(*_batch((s, d), i)), (np.int64, np.int64)) for i in range(2)]
    return outs[0], outs[1], (len(s), ref.beta_sum(), int(ref.previous), ref.rows())


def _trisample_export(st):
    hdr, rows = st.export()
    return int(hdr["edges_seen"]), int(hdr["beta_sum"]), int(hdr["last_emitted"]), rows


def _trisample_nontrivial(e):
    assert len(e[0][0]) > 10 and len(e[1][0]) > 10 and e[2][1] > 0


_state_variant("trisample_broadcast", _trisample_inputs, _trisample_expected,
               lambda e: e.triangle_sampler("broadcast", TS_SAMPLES, TS_VERTICES, TS_SEED),
               lambda st, put, inp, i: st.edges(*(put(c) for c in _batch(inp, i))), _trisample_export,
               _two_batches(_trisample_inputs, adds=False), _trisample_nontrivial)


# ---- error variants: API errors the library returns by design -----------------------------------------------------
def _lib_of(engine):
    return importlib.import_module(type(engine).__module__.rsplit(".", 1)[0] + "._lib")


def reduce_short_then_fetch(engine, s, d, v, direction, op):
    """gs_window_reduce into device outputs one row short of the window's vertices (found by a sizing call with
    capacity 0), then gs_fetch_last_output -> (status of the short call, the vertices it reported, fetched keys,
    fetched values)"""
    if hasattr(engine, "reduce_short_then_fetch"):
        return engine.reduce_short_then_fetch(s, d, v, direction, op)
    import torch

    L = _lib_of(engine)
    dev = f"cuda:{engine.device}"
    S, D, V = (torch.from_numpy(np.array(_np(x))).to(dev) for x in (s, d, v))
    b = L.GsEdgeBatch(S.data_ptr(), D.data_ptr(), V.data_ptr(), len(S), L.GS_DTYPE_OF[np.dtype(_np(v).dtype)],
                      L.GS_MEM_DEVICE, 0)
    n_out = ctypes.c_uint64(0)

    def call(fn, keys, vals, cap):
        vo = L.GsVertexOut(keys.data_ptr() if cap else None, vals.data_ptr() if cap else None, cap, ctypes.pointer(n_out),
                           L.GS_MEM_DEVICE, 0)
        return fn(vo)

    window = lambda vo: engine._L.gs_window_reduce(engine.ctx, ctypes.byref(b), direction, op, ctypes.byref(vo))
    fetch = lambda vo: engine._L.gs_fetch_last_output(engine.ctx, ctypes.byref(vo))
    tdt = torch.from_numpy(np.empty(0, _np(v).dtype)).dtype
    assert call(window, None, None, 0) == GS_ECAPACITY   # the sizing call
    U = n_out.value
    keys, vals = torch.full((U,), -1, dtype=torch.int64, device=dev), torch.zeros(U, dtype=tdt, device=dev)
    st = call(window, keys, vals, U - 1)
    reported = n_out.value
    n_out.value = 0
    fst = call(fetch, keys, vals, U)
    if fst != 0:
        raise L.GsError(fst, engine._L.gs_last_error(engine.ctx).decode())
    return st, reported, keys[:n_out.value], vals[:n_out.value]


def components_short(engine, s, d, U):
    """gs_window_components into host outputs of U - 1 rows -> (status, the vertices it reported)"""
    if hasattr(engine, "components_short"):
        return engine.components_short(s, d, U)
    L = _lib_of(engine)
    s, d = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(d, np.int64)
    b = L.GsEdgeBatch(s.ctypes.data, d.ctypes.data, None, len(s), L.GS_NONE, L.GS_MEM_HOST, 0)
    keys, labels = np.full(U, -1, np.int64), np.full(U, -1, np.int64)
    n_out = ctypes.c_uint64(0)
    vo = L.GsVertexOut(keys.ctypes.data, labels.ctypes.data, U - 1, ctypes.pointer(n_out), L.GS_MEM_HOST, 0)
    st = engine._L.gs_window_components(engine.ctx, ctypes.byref(b), None, ctypes.byref(vo))
    assert np.all(keys[U - 1:] == -1) and np.all(labels[U - 1:] == -1)   # nothing past the capacity
    return st, n_out.value


def _err_reduce_inputs():
    s, d, rng = _uniform(0xE001, 20_000, 1 << 18)
    return _frozen(s, d, _oracle().gen_values(20_000, 0xE001, _oracle().DT_I64))


def _err_reduce_expected():
    k, v = _oracle().window_reduce(*_err_reduce_inputs(), OUT, SUM)
    return GS_ECAPACITY, len(k), k, v


_variant("err_capacity_reduce", "error", _err_reduce_inputs, _err_reduce_expected,
         lambda engine, put, inp: reduce_short_then_fetch(engine, *inp, OUT, SUM),
         _bucket_precondition(_err_reduce_inputs, OUT, S_LONG, 16), nontrivial=lambda e: _sized(e[2], e[1]))


def _err_cc_inputs():
    return _frozen(*pin_ends(*_oracle().gen_rmat(12, 5_000, 0xE002), 12))


def _err_cc_expected():
    return GS_ECAPACITY, len(_oracle().components(*_err_cc_inputs())[0])


_variant("err_capacity_cc", "error", _err_cc_inputs, _err_cc_expected,
         lambda engine, put, inp: components_short(engine, *inp, _err_cc_expected()[1]),
         lambda: _sized(_err_cc_inputs()[0], 5_000), nontrivial=lambda e: _positive(e[1], 100))

BAD_DIRECTION = 7


def _err_direction_inputs():
    s, d, rng = _uniform(0xE003, 1_000, 1 << 14)
    return _frozen(s, d, np.ones(1_000, np.int64))


_variant("err_bad_direction", "error", _err_direction_inputs, lambda: GS_EINVAL,
         lambda engine, put, inp: status_of(lambda: engine.reduce(*(put(x) for x in inp), BAD_DIRECTION, SUM)),
         lambda: None, nontrivial=lambda e: None)

BAD_RECORD = 1_234


def _err_text_inputs():
    lines = [f"{i} {i + 1} {i * 7}" for i in range(2_000)]
    lines[BAD_RECORD] = "12 x3 5"
    return (("\n".join(lines) + "\n").encode(),)


def _err_text_check():
    cols, bad = textparse_ref.parse(_err_text_inputs()[0])
    assert cols is None and bad == BAD_RECORD


_variant("err_text", "error", _err_text_inputs, lambda: GS_EINVAL,
         lambda engine, put, inp: status_of(lambda: engine.parse_edges_text(inp[0], out_device=put is not _host)),
         _err_text_check, nontrivial=lambda e: None)

CAND_CHUNK = 1_000


def _err_cand_inputs():
    return _frozen(*_oracle().gen_rmat(10, 2_000, 0xE005))


def _err_cand_expected():
    a, b, f, _ = _oracle().window_candidates(*_err_cand_inputs())
    return a, b, f


def _err_cand_first(engine, put, inp):
    want = _err_cand_expected()
    cols = tuple(put(x) for x in inp)
    total = engine.candidates_begin(*cols)
    a, b, f, first, done = engine.candidates_next(CAND_CHUNK)
    same((total, a, b, f, first, done), (len(want[0]),) + tuple(w[:CAND_CHUNK] for w in want) + (0, False), where="chunk 1")
    return {"engine": engine, "cols": cols}   # (the columns stay alive until the session's last candidates_next)


def _err_cand_second(token, intervened, inp):
    """after another entry point call the session is over: EINVAL, never stale records; straight after chunk 1
    (the variant twice in a row) the session goes on with chunk 2"""
    engine = token["engine"]
    if intervened:
        return status_of(lambda: engine.candidates_next(CAND_CHUNK))
    want = _err_cand_expected()
    a, b, f, first, done = engine.candidates_next(CAND_CHUNK)
    same((a, b, f, first, done), tuple(w[CAND_CHUNK:2 * CAND_CHUNK] for w in want) + (CAND_CHUNK, False), where="chunk 2")
    return "continued"


_variant("err_cand_session", "error", _err_cand_inputs, lambda: GS_EINVAL, _err_cand_first,
         lambda: _positive(len(_err_cand_expected()[0]), 2 * CAND_CHUNK), second=_err_cand_second,
         nontrivial=lambda e: None)

NAMES = tuple(VARIANTS)
PLAIN = tuple(n for n in NAMES if not VARIANTS[n].error)
ERRORS = tuple(n for n in NAMES if VARIANTS[n].error)
BUCKET = tuple(n for n in NAMES if VARIANTS[n].group == "bucket")


# ---- sequences ------------------------------------------------------------------------------------------------
def pair_sequence(a: str, b: str) -> list:
    """A->B, B->B, B->A, A->A and A->B again"""
    return [a, b, b, a, a, b]


def ordered_pairs(seq) -> set:
    return set(zip(seq, seq[1:]))


def walk(seed: int, steps: int) -> list:
    """a seeded random walk over all non-error variants"""
    rng = np.random.default_rng(seed)
    return [PLAIN[i] for i in rng.integers(0, len(PLAIN), steps)]


def expand(names) -> list:
    """the calls of a sequence: (name, half), a stateful variant's places alternating between its halves, and one
    closing "second" at the end for each one left open"""
    open_, out = {}, []
    for n in names:
        if VARIANTS[n].stateful:
            half = "second" if open_.get(n) else "first"
            open_[n] = half == "first"
        else:
            half = "first"
        out.append((n, half))
    out.extend((n, "second") for n, is_open in open_.items() if is_open)
    return out


def check_result(v: Variant, half: str, got, intervened=True):
    if v.stateful and half == "first":
        return   # the first half's output is checked with the second's
    if v.name == "err_cand_session" and not intervened:
        assert got == "continued"
        return
    same(got, v.expected(), v.float_sum, v.name)


def run_sequence(engine, names, put=_host, after_each=None, label=None):
    """Run the sequence on `engine`, every call checked against the variant's expected.  A failure (a wrong result or
    an error from the library) is re-raised as an AssertionError naming the sequence, the position and the previous
    call; states still open are closed first."""
    calls = expand(names)
    tokens, prev = {}, None
    try:
        for at, (n, half) in enumerate(calls):
            v = VARIANTS[n]
            try:
                if half == "first":
                    got = v.first(engine, put, v.inputs())
                    if v.stateful:
                        tokens[n] = (got, at)
                    intervened = True
                else:
                    token, since = tokens.pop(n)
                    intervened = at - since > 1
                    got = v.second(token, intervened, v.inputs())
                check_result(v, half, got, intervened)
                if after_each is not None:
                    after_each(at, n, half)
            except Exception as e:   # noqa: BLE001
                where = f"{label or list(names)}: call {at} = {n}.{half} after {prev or 'nothing'}"
                raise AssertionError(f"{where}: {type(e).__name__}: {e}") from e
            prev = f"{n}.{half}"
    finally:
        for token, _ in tokens.values():
            st = token.get("state") if isinstance(token, dict) else None
            if st is not None:
                st.close()
