"""The numpy model of gs_slice_reduce / gs_slice_fold_degree_max (a plain module, CPU only).

  window_start      start = ts - ts % size with Java's truncated remainder (oracle.window_start's rule, exact for
                    every int64: Python integers)
  geometry / pack / unpack   the composite key ((start - start_min) / size) << vbits | (vertex - vertex_min),
                    the widths of the two spans (spans taken in unbounded integers, as the engine takes them in
                    unsigned words) and the refusal rule wbits + vbits > 64
  sliced            every window's per-window oracle result, concatenated in window order: what the batched call
                    returns (window_start, row_begin, *row columns)
"""
from dataclasses import dataclass

import numpy as np

DIR_IN, DIR_OUT, DIR_ALL = 0, 1, 2
KEY_BITS = 64


def _trunc_div(t: int, size: int) -> int:
    return t // size if t >= 0 else -((-t) // size)


def window_start(ts, size):
    """int64 array of window starts; ts - ts % size cannot overflow (|start| <= |ts|)."""
    return np.array([_trunc_div(int(t), int(size)) * int(size) for t in np.asarray(ts, dtype=np.int64)], dtype=np.int64)


def key_columns(src, dst, direction):
    """the vertices that key records under `direction` (both columns for ALL)"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    return {DIR_IN: (dst,), DIR_OUT: (src,), DIR_ALL: (src, dst)}[int(direction)]


def expand(src, dst, ts, direction):
    """(key vertex, timestamp) per record in arrival order: ALL gives e at 2i and e.reverse() at 2i + 1, both with
    the edge's timestamp"""
    src, dst, ts = (np.asarray(x, dtype=np.int64) for x in (src, dst, ts))
    if int(direction) == DIR_ALL:
        k = np.empty(2 * len(src), np.int64)
        k[0::2], k[1::2] = src, dst
        return k, np.repeat(ts, 2)
    return (dst if int(direction) == DIR_IN else src), ts


class Refused(Exception):
    """wbits + vbits > 64: the engine returns GS_EUNSUPPORTED and the caller loops over the windows"""


@dataclass(frozen=True)
class Geometry:
    size: int
    start_min: int
    vertex_min: int
    wbits: int
    vbits: int


def geometry(src, dst, ts, size, direction) -> Geometry:
    """Widths of the window span (in windows) and of the vertex span.  The spans are differences of int64 extremes:
    up to 2^64 - 1, so they are taken in Python integers (the engine: unsigned 64-bit words)."""
    cols = key_columns(src, dst, direction)
    vmin = min(int(c.min()) for c in cols)
    vmax = max(int(c.max()) for c in cols)
    st = window_start(ts, size)
    smin, smax = int(st.min()), int(st.max())
    wspan = (smax - smin) // int(size)
    vspan = vmax - vmin
    assert 0 <= wspan < 1 << 64 and 0 <= vspan < 1 << 64
    g = Geometry(int(size), smin, vmin, wspan.bit_length(), vspan.bit_length())
    if g.wbits + g.vbits > KEY_BITS:
        raise Refused(f"{g.wbits} window bits + {g.vbits} vertex bits")
    return g


def pack(g: Geometry, vertex, ts):
    """composite keys (Python integers below 2^64) of records (vertex, ts)"""
    out = []
    for v, t in zip(np.asarray(vertex, dtype=np.int64), np.asarray(ts, dtype=np.int64)):
        w = (_trunc_div(int(t), g.size) * g.size - g.start_min) // g.size
        k = (w << g.vbits) | (int(v) - g.vertex_min)
        assert 0 <= k < 1 << KEY_BITS
        out.append(k)
    return out


def unpack(g: Geometry, keys):
    """(window start, vertex) per composite key"""
    mask = (1 << g.vbits) - 1
    return [(g.start_min + (k >> g.vbits) * g.size, g.vertex_min + (k & mask)) for k in keys]


def sliced(oracle_fn, src, dst, val, ts, size, direction, *args):
    """oracle_fn(src, dst[, val], direction, *args) per window of oracle.split_windows, concatenated:
    (window_start[W], row_begin[W + 1], *row columns).  val None: the oracle function takes no values (the degree
    fold)."""
    import __graft_entry__ as ge
    orc = ge.load_oracle()
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    starts, begin, cols = [], [0], None
    for start, idx in orc.split_windows(ts, size):
        cut = (src[idx], dst[idx]) + (() if val is None else (np.asarray(val)[idx],))
        res = oracle_fn(*cut, direction, *args)
        cols = [[] for _ in res] if cols is None else cols
        for c, r in zip(cols, res):
            c.append(np.array(r))
        starts.append(start)
        begin.append(begin[-1] + len(res[0]))
    rows = tuple(np.concatenate(c) for c in cols) if cols else ()
    return (np.array(starts, dtype=np.int64), np.array(begin, dtype=np.uint64)) + rows
