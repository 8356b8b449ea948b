"""CPU: oracle/gs_oracle.c (gso_parse_edges_text), the checker of csrc/gs_text.hip, pinned to the
independent Python restatement of the Java rules in tests/textparse_ref.py: both agree on accept or
reject, on the values and on the index of the first malformed record."""
import ctypes

import numpy as np
import pytest

import textparse_ref as ref
from test_oracle_golden import BAD_RECORDS


def _oracle_middle(oracle):
    """record -> the oracle's verdict on b"5 6 7\\n" + record + b"\\n8 9 10\\n": the middle row, or the index
    of the record it rejects (one library call per record, into reused buffers)"""
    fn = oracle.lib().gso_parse_edges_text
    cols = [np.zeros(4, np.int64) for _ in range(3)]
    ptrs = [c.ctypes.data_as(ctypes.c_void_p) for c in cols]

    def run(rec):
        text = b"5 6 7\n" + rec + b"\n8 9 10\n"
        n = fn(text, len(text), ptrs[0], ptrs[1], ptrs[2], 4)
        if n < 0:
            return -1 - n
        assert n == 3 and [int(c[0]) for c in cols] == [5, 6, 7] and [int(c[2]) for c in cols] == [8, 9, 10]
        return tuple(int(c[1]) for c in cols)
    return run


def _ref_middle(rec):
    text = b"5 6 7\n" + rec + b"\n8 9 10\n"
    cols, bad = ref.parse(text)
    if bad is not None:
        return bad
    assert len(cols[0]) == 3
    return tuple(int(c[1]) for c in cols)


def _compare(oracle, recs):
    run = _oracle_middle(oracle)
    total = accepted = 0
    for rec in recs:
        want = _ref_middle(rec)
        assert run(rec) == want, rec
        total += 1
        accepted += isinstance(want, tuple)
    return total, accepted


def test_every_short_string_over_the_alphabet(oracle):
    total, accepted = _compare(oracle, ref.alphabet_records())
    assert total == sum(8 ** n for n in range(7)) == 299593
    assert accepted == 224      # three fields of "1" with optional signs, single separators, whitespace tail


def test_field_separator_tail_grid(oracle):
    total, accepted = _compare(oracle, ref.grid_records())
    assert total == 24 ** 3 + 9 * 9 * 9 * 24 == 31320
    assert accepted == 2529


def test_reference_on_known_records():
    """the restatement itself, on records whose Java outcome is known by hand"""
    lo, hi = -(1 << 63), (1 << 63) - 1
    assert ref.parse_record(b"1 2 3") == (1, 2, 3)
    assert ref.parse_record(b"-4\t+5\x0b6 extra fields") == (-4, 5, 6)
    assert ref.parse_record(b"%d %d 0" % (hi, lo)) == (hi, lo, 0)
    assert ref.parse_record(b"00000000000000000000001 -0 +0") == (1, 0, 0)
    assert ref.parse_record(b"1 2 3 ") == (1, 2, 3) and ref.parse_record(b"1 2 3\t\t") == (1, 2, 3)
    assert ref.parse_record(b"1\r2\f3") == (1, 2, 3)          # a CR inside a record is a separator like any
    for bad in BAD_RECORDS + [b"1 2 3_0", b"1 2 1_0", b"\xd9\xa1 2 3", b"1 2 3\x00", b"1\xa02 3 4", b" ", b"1 2 \t3"]:
        assert ref.parse_record(bad) is None, bad
    assert ref.records(b"") == [] and ref.records(b"\n") == [b""] and ref.records(b"a\r\nb") == [b"a", b"b"]
    assert ref.records(b"a\r\r\n\r") == [b"a\r", b""]


@pytest.mark.parametrize("text", [b"", b"\n", b"\n\n", b"1 2 3\n\n", b"1 2 3\n" + b"\n" * 100, b"1 2 3", b"1 2 3\r",
                                  b"\r\n", b"1 2 3\n\r"] + [b"1 2 3\n" + b + b"\n4 5 6\n" for b in BAD_RECORDS]
                         + [b"1 2 3\n4 5 6\n" + b for b in BAD_RECORDS])
def test_whole_texts(oracle, text):
    cols, bad = ref.parse(text)
    if bad is None:
        got = oracle.parse_edges_text(text)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, cols))
    else:
        with pytest.raises(ValueError, match=f"record {bad}$"):
            oracle.parse_edges_text(text)


def test_plan_matches_hand_counts():
    """plan() on texts small enough to count by hand"""
    p = ref.plan(b"")
    assert (p.tiles, p.records, p.scan_chunks, len(p.block_words)) == (0, 0, 0, 0)
    p = ref.plan(b"1 2 3\n4 5 6")
    assert (p.tiles, p.records, list(p.tile_newlines), list(p.block_words), list(p.block_staged)) == \
        (1, 2, [1], [3], [True])
    line = b"1 2 3 " + b"z" * 57 + b"\n"                      # 64 bytes
    p = ref.plan(line * 513)
    assert p.tiles == 3 and list(p.tile_newlines) == [256, 256, 1] and p.records == 513
    assert list(p.block_words) == [4096, 4096, 16] and p.block_staged.all()
    p = ref.plan(b"9\n" + line * 512)                          # blocks start at byte 0 and 2 + 255 * 64
    assert list(p.block_words) == [4081, 4097, 17] and list(p.block_staged) == [True, False, True]
    assert ref.plan(b"x" * (ref.TILE * 1024)).scan_chunks == 1 and ref.plan(b"x" * (ref.TILE * 1024 + 1)).scan_chunks == 2
