"""Plain Python restatement of the examples' edge text input, written from the Java rules and not from
oracle/gs_oracle.c, so that the kernel (csrc/gs_text.hip) and the C oracle cannot share a misreading:

    env.readTextFile(path).map(s -> { f = s.split("\\s"); Long.parseLong(f[0]), f[1], f[2] })
    (example/WindowTriangles.java:175-185)

* TextInputFormat (Flink 1.0.3): records are the pieces between '\n'; what follows the last '\n' is a
  record only when it is non-empty; one trailing '\r' is dropped from a record.
* String.split("\\s"): a split at every single char of [ \t\n\x0B\f\r]; trailing empty strings are
  dropped (leading and inner ones stay, and then fail in parseLong).
* Long.parseLong: [+-]?[0-9]+ over the whole field, value in [-2^63, 2^63).  (Only ASCII digits: the
  library's documented limit, include/gelly_hip.h.)
* fields[0..2] are read: fewer than three fields throws (ArrayIndexOutOfBounds), later ones are ignored.

Also here: plan(), which maps a text onto the launch geometry of gs_text.hip, and the record families
that tests/test_textparse_ref.py and tests/test_gpu_text.py share.
"""
from __future__ import annotations

import functools
import itertools
import re
from typing import NamedTuple

import numpy as np

_WS = re.compile(rb"[ \t\n\x0b\f\r]")
_LONG = re.compile(rb"[+-]?[0-9]+")


def records(text: bytes):
    recs = bytes(text).split(b"\n")
    if recs[-1] == b"":
        recs.pop()
    return [r[:-1] if r.endswith(b"\r") else r for r in recs]


def parse_record(rec: bytes):
    """(src, dst, ts) as Python ints, or None where the reference's map throws."""
    fields = _WS.split(rec)
    while fields and fields[-1] == b"":
        fields.pop()
    if len(fields) < 3:
        return None
    out = []
    for f in fields[:3]:
        if not _LONG.fullmatch(f):
            return None
        v = int(f)
        if not -(1 << 63) <= v < (1 << 63):
            return None
        out.append(v)
    return tuple(out)


def parse(text: bytes):
    """((src, dst, ts) int64 arrays, None), or (None, index of the first record that throws)."""
    rows = []
    for i, rec in enumerate(records(text)):
        r = parse_record(rec)
        if r is None:
            return None, i
        rows.append(r)
    a = np.array(rows, dtype=np.int64).reshape(len(rows), 3)
    return (a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()), None


# ---- launch geometry of gelly-streaming_amd/csrc/gs_text.hip ------------------------------------------
# TX_TILE = TX_BLOCK * 16 * TX_VEC = 16384 bytes per k_tx_count / k_tx_starts block;
# TX_BLOCK = 256 records per k_tx_parse block; TX_LDS_WORDS = 4096 words of record text a parse block
# can stage (staged = w1 - w0 <= TX_LDS_WORDS); k_scan_chunks walks the tile counts in 1024-wide chunks.
TILE = 16384
BLOCK_RECORDS = 256
LDS_WORDS = 4096
SCAN_CHUNK = 1024


class Plan(NamedTuple):
    tiles: int                  # k_tx_count / k_tx_starts grid
    tile_newlines: np.ndarray   # newlines of each tile
    scan_chunks: int            # trips of k_scan_chunks' loop (a carry crosses when > 1)
    records: int
    starts: np.ndarray          # byte offset of each record (and of the end after the last newline)
    block_words: np.ndarray     # per parse block, w1 - w0
    block_staged: np.ndarray    # per parse block, whether its text goes through LDS

    def block_of(self, record: int) -> int:
        return record // BLOCK_RECORDS


def plan(text: bytes) -> Plan:
    a = np.frombuffer(bytes(text), np.uint8)
    n = len(a)
    nt = (n + TILE - 1) // TILE
    nlpos = np.flatnonzero(a == 10).astype(np.int64)
    tile_nl = np.bincount(nlpos // TILE, minlength=nt).astype(np.int64)
    nl = len(nlpos)
    nrec = nl + (1 if n and a[-1] != 10 else 0)
    starts = np.concatenate([np.zeros(1, np.int64), nlpos + 1])
    words = []
    for r0 in range(0, nrec, BLOCK_RECORDS):
        rl = min(nrec, r0 + BLOCK_RECORDS)
        span0 = int(starts[r0])
        span1 = int(starts[rl]) if rl <= nl else n
        words.append(((span1 + 3) >> 2) - (span0 >> 2))
    words = np.array(words, dtype=np.int64)
    return Plan(nt, tile_nl, (nt + SCAN_CHUNK - 1) // SCAN_CHUNK, nrec, starts, words, words <= LDS_WORDS)


# ---- record families ----------------------------------------------------------------------------------
ALPHABET = [b"1", b"-", b"+", b" ", b"\t", b"\r", b"x", b"\x0b"]

FIELDS = [b"", b"1", b"-", b"+", b"-1", b"+1", b"1-", b"1x", b"x", b"--1", b"01", b"-0", b"9223372036854775807",
          b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809", b"00000000000000000000001",
          b"18446744073709551616", b"18446744073709551617", b"9223372036854775799", b"92233720368547758070",
          b"\xd9\xa1", b"1\x00", b"\xff"]
SEPARATORS = [b" ", b"\t", b"\x0b", b"\f", b"\r", b"  ", b",", b"\xa0", b"\x1c"]
TAILS = [b"", b" ", b"\r", b" x", b" 1 2", b"\t\t", b"x", b"\r\r", b" \r"]


def alphabet_records():
    """every byte string of length 0..6 over ALPHABET"""
    for n in range(7):
        for t in itertools.product(ALPHABET, repeat=n):
            yield b"".join(t)


def grid_records():
    for a, b, c in itertools.product(FIELDS, repeat=3):
        yield a + b" " + b + b" " + c
    for s0, s1, t, f in itertools.product(SEPARATORS, SEPARATORS, TAILS, FIELDS):
        yield f + s0 + b"-2" + s1 + f + t


def nominal_variants():
    """the record "7 -2 9" with one thing changed at a time"""
    out = []
    for f in FIELDS:
        out += [f + b" -2 9", b"7 " + f + b" 9", b"7 -2 " + f]
    for s in SEPARATORS:
        out += [b"7" + s + b"-2 9", b"7 -2" + s + b"9"]
    for t in TAILS:
        out.append(b"7 -2 9" + t)
    return out


@functools.lru_cache(maxsize=None)
def accepted_family_records():
    """the records of both families that parse, as the middle record of a text would (no '\n' in any;
    a final '\r' is the record's CR)"""
    out = []
    for rec in itertools.chain(alphabet_records(), grid_records()):
        if parse_record(rec[:-1] if rec.endswith(b"\r") else rec) is not None:
            out.append(rec)
    return tuple(out)
