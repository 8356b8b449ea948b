"""Order-preserving id maps for the window operators' tests (not a test module).

Every window operator measures the id range of its window and picks a code path from it (include/gelly_hip.h;
gs_cc_common.hpp uf_window, gs_triangles.hip tri_geometry, gs_relabel.hip, gs_pairs.hip, gs_hashset.hip).  A
strictly increasing map of the ids changes that path and nothing else: the CPU oracles take any int64, and what
they return on the mapped ids is the reference.

maps(K): the maps over base ids x in [0, 2^K), by name.  A graph used with a map holds base ids 0 and 2^K - 1
(pin_ends), so its geometry is the one the map is named for:

  bits    the width of the XOR mask the library measures (mask_bits), which decides direct / relabel
  span    largest id - smallest id, which decides the packed stage-2 keys and the u32 candidate chunks
  direct  bits <= DIRECT_BITS: union-find and triangles index their tables with id ^ key_xor
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np

DIRECT_BITS = 28   # = CC_DIRECT_BITS (gs_cc_common.hpp) = TRI_MAX_BITS (gs_triangles.hip); tests/test_idmaps_ref.py
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SPARSE_MUL = 7_919_000_003


@dataclass(frozen=True)
class IdMap:
    name: str
    K: int
    f: Callable[[np.ndarray], np.ndarray]   # int64 array of base ids -> int64 array
    bits: int
    span: int

    @property
    def direct(self) -> bool:
        return self.bits <= DIRECT_BITS

    def __call__(self, x):
        x = np.asarray(x, np.int64)
        assert x.size == 0 or (0 <= int(x.min()) and int(x.max()) < (1 << self.K))
        y = self.f(x)
        assert y.dtype == np.int64
        return y


def maps(K: int) -> dict:
    top = (1 << K) - 1
    half = 1 << (K - 1)

    def stride(t):
        return t // top

    def spread(t, off=0):
        return lambda x: x * stride(t) + off

    def ends(last):   # x * stride(2^31) below the last id, the last id -> `last`
        return lambda x: np.where(x == top, np.int64(last), x * stride(1 << 31))

    def sparse(x):
        return x * SPARSE_MUL - (1 << 61)

    def extremes(x):
        return np.where(x == 0, np.int64(I64_MIN), np.where(x == top, np.int64(I64_MAX), sparse(x)))

    s24, s28, s29 = (top * stride((1 << b) - 1) for b in (24, 28, 29))
    rows = [
        ("identity", lambda x: x + 0, K, top),
        ("offset_2p40", lambda x: x + (1 << 40), K, top),
        ("negative_band", lambda x: x - (1 << 62), K, top),
        ("below_2p28", lambda x: x + ((1 << 28) - (1 << K)), K, top),
        ("straddle_2p28", lambda x: x + ((1 << 28) - half), 29, top),
        ("straddle_2p32", lambda x: x + ((1 << 32) - half), 33, top),
        ("straddle_zero", lambda x: x - half, 64, top),
        ("spread_2p24", spread((1 << 24) - 1), 24, s24),
        ("spread_2p24_neg", spread((1 << 24) - 1, -(1 << 62)), 24, s24),
        ("spread_2p28", spread((1 << 28) - 1), 28, s28),
        ("spread_2p29", spread((1 << 29) - 1), 29, s29),
        ("span_2p32m1", ends((1 << 32) - 1), 32, (1 << 32) - 1),
        ("span_2p32", ends(1 << 32), 33, 1 << 32),
        ("sparse", sparse, (top * SPARSE_MUL).bit_length(), top * SPARSE_MUL),
        ("extremes", extremes, 64, (1 << 64) - 1),
    ]
    return {name: IdMap(name, K, f, bits, span) for name, f, bits, span in rows}


NAMES = tuple(maps(10))


def mask_bits(src, dst) -> int:
    """The library's rule: the width of the OR of (id ^ src[0]) over both columns (0: one id only)."""
    s, d = np.asarray(src, np.int64).view(np.uint64), np.asarray(dst, np.int64).view(np.uint64)
    k0 = s[0]
    return int(np.bitwise_or.reduce(s ^ k0) | np.bitwise_or.reduce(d ^ k0)).bit_length()


def id_span(src, dst) -> int:
    lo = min(int(np.min(src)), int(np.min(dst)))
    hi = max(int(np.max(src)), int(np.max(dst)))
    return hi - lo


def pin_ends(src, dst, K: int, lo: int = 0, hi: int | None = None, at: int = 0):
    """Copies of the columns with record `at` = (lo, hi), by default (0, 2^K - 1): the graph spans the whole base
    range, so a map gives it the geometry it is named for."""
    s, d = np.array(src, np.int64), np.array(dst, np.int64)
    s[at], d[at] = lo, (1 << K) - 1 if hi is None else hi
    return s, d
