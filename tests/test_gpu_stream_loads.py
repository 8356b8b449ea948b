"""GPU: the column loads of the speculative scatters and the partition loads of k_bk_accum (ld_stream,
gs_device.hpp: 16- and 8-byte loads, plain or non-temporal) on every path the load code takes.

Windows sit around one scatter tile (8192 records for the packed scatter, 5120 for the unpacked one; under ALL an
edge is two records): two full tiles and a partial one, exactly one tile, one record less, five records.  Columns
are taken as allocated (16-byte aligned: two records per lane and load on full tiles) and with the key or the
value column as a [1:] view of a longer tensor (8-byte aligned, 4-byte for int32 values: the record-by-record
loads).  Buckets 1 .. 6 hold 1, 2, 3, 4, 5 and 7 records, so their accumulate pieces are shorter than one 16-byte
group, pure head / tail, or one group and a tail; buckets 0 and 7 share the rest.  About 1 % of the values are
>= 2^16, 1 % zero and 1 % negative (escapes and presence through both load paths); the five-record windows keep
every value narrow, since more than 1/8 escapes would switch the next window to unpacked records.

Every case runs the window twice on one engine: the second is the speculative window, bit-exact against the
oracle."""
import numpy as np
import pytest
import torch

from test_gpu_bucket import _check, _dev

pytestmark = pytest.mark.gpu

IN, OUT, ALL = 0, 1, 2
SMALL = (1, 2, 3, 4, 5, 7)   # records of buckets 1 .. 6
PACK_TILE, UNPACK_TILE = 8192, 5120

_REF = {}   # windows and references computed once (never modified)


def _once(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _sizes(tile):
    return [2 * tile + 37, tile, tile - 1, 5]


def _window(n, width, direction, seed):
    """n edges: (src, dst, val as int64).  The key column's ids by bucket as the module docstring says; under ALL the
    other column is a key column too and lies in buckets 0 and 7 only, so the small buckets keep their counts."""
    rng = np.random.default_rng(seed)
    counts, left = [], n
    for c in SMALL:
        counts.append(min(c, left))
        left -= counts[-1]
    bucket = np.concatenate([np.repeat(np.arange(1, 7), counts), np.repeat([0, 7], [left // 2, left - left // 2])])
    key = bucket[rng.permutation(n)] * width + rng.integers(0, width, n)
    other = rng.choice([0, 7], n) * width + rng.integers(0, width, n)
    v = rng.integers(1, 1 << 16, n)
    if n > 5:
        v[rng.random(n) < 0.01] = 0
        neg = rng.random(n) < 0.01
        v[neg] = -rng.integers(1, 1 << 20, int(neg.sum()))
        wide = rng.random(n) < 0.01
        v[wide] = rng.integers(1 << 16, 1 << 30, int(wide.sum()))
        v[:3] = (1 << 20, 0, -3)
    else:
        v[0] = 0
    s, d = (other, key) if direction == IN else (key, other)
    return s.astype(np.int64), d.astype(np.int64), v.astype(np.int64)


def _shifted(a):
    """The same values as a [1:] view of a longer device tensor: the data pointer moves by one element."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    big = torch.empty(len(a) + 1, dtype=t.dtype, device="cuda")
    big[1:] = t.cuda()
    view = big[1:]
    assert view.data_ptr() % 16 == t.element_size() % 16 and view.is_contiguous()
    return view


def _run(pkg, oracle, n, width, direction, dtype, op, align, packed):
    s, d, v = _once(("win", n, width, direction), lambda: _window(n, width, direction, 1000 * direction + n % 997))
    val = v.astype(dtype)   # (COUNT ignores it)
    rk, rv = _once(("ref", n, width, direction, np.dtype(dtype).name, op),
                   lambda: oracle.window_reduce(s, d, val, direction, op))
    S, D, V = _dev(s, d, val)
    if align == "key":   # the key column(s): under ALL both columns hold keys
        if direction != IN:
            S = _shifted(s)
        if direction != OUT:
            D = _shifted(d)
    elif align == "val":
        V = _shifted(val)
    with pkg.Engine(0) as e:
        for w in range(2):
            gk, gv = e.reduce(S, D, V, direction, op)
            t = e.stage_times()
            assert t.path == 2 and t.speculative == w and t.packed == packed, (w, t.path, t.speculative, t.packed)
            _check(gk, gv, rk, rv, dtype, op)
            # (Double sums too: the values are integers, so every order of additions gives the same bits)
            assert np.array_equal(gv.cpu().numpy(), rv)


@pytest.mark.parametrize("align", ["aligned", "key", "val"])
@pytest.mark.parametrize("n_tile", range(4), ids=["2t+37", "t", "t-1", "5"])
@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("direction", [IN, OUT, ALL], ids=["in", "out", "all"])
def test_packed_scatter_and_accumulate(pkg, oracle, direction, dtype, n_tile, align):
    """k_sp_scatter_pack and the packed stream of k_bk_accum: integer SUM."""
    n = _sizes(PACK_TILE // (2 if direction == ALL else 1))[n_tile]
    width = 1 << (14 if dtype == np.int64 else 15)   # ids per bucket: 8- and 4-byte accumulators
    _run(pkg, oracle, n, width, direction, dtype, 0, align, True)


@pytest.mark.parametrize("align", ["aligned", "key", "val"])
@pytest.mark.parametrize("n_tile", range(4), ids=["2t+37", "t", "t-1", "5"])
@pytest.mark.parametrize("direction", [IN, OUT, ALL], ids=["in", "out", "all"])
def test_unpacked_scatter_double_sum(pkg, oracle, direction, n_tile, align):
    """k_sp_scatter with an 8-byte payload and the unpacked partition's key / value groups in k_bk_accum."""
    n = _sizes(UNPACK_TILE // (2 if direction == ALL else 1))[n_tile]
    _run(pkg, oracle, n, 1 << 14, direction, np.float64, 0, align, False)


@pytest.mark.parametrize("direction", [IN, OUT, ALL], ids=["in", "out", "all"])
def test_unpacked_scatter_four_byte_values(pkg, oracle, direction):
    """4-byte payloads through k_sp_scatter and the accumulate's 16-byte value groups: int32 values of which a
    quarter are negative escape in the first window, so the following windows store the values in full."""
    n = _sizes(UNPACK_TILE // (2 if direction == ALL else 1))[0]
    s, d, v = _once(("win", n, 1 << 15, direction), lambda: _window(n, 1 << 15, direction, 1000 * direction + n % 997))
    val = np.where(np.arange(n) % 4 == 1, -(v & 0xFFFF) - 1, v).astype(np.int32)
    rk, rv = _once(("ref4", n, direction), lambda: oracle.window_reduce(s, d, val, direction, 0))
    cols = _dev(s, d, val)
    with pkg.Engine(0) as e:
        for w in range(3):
            gk, gv = e.reduce(*cols, direction, 0)
            t = e.stage_times()
            assert t.path == 2 and t.packed == (w == 0), (w, t.path, t.packed)
            _check(gk, gv, rk, rv, np.int32, 0)
        assert t.speculative == 1


@pytest.mark.parametrize("align", ["aligned", "key"])
@pytest.mark.parametrize("n_tile", range(4), ids=["2t+37", "t", "t-1", "5"])
@pytest.mark.parametrize("direction", [IN, OUT, ALL], ids=["in", "out", "all"])
def test_unpacked_scatter_count(pkg, oracle, direction, n_tile, align):
    """k_sp_scatter without a payload: COUNT."""
    n = _sizes(UNPACK_TILE // (2 if direction == ALL else 1))[n_tile]
    _run(pkg, oracle, n, 1 << 15, direction, np.int64, 3, align, False)
