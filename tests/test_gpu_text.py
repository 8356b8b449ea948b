"""GPU: gs_parse_edges_text (csrc/gs_text.hip) on the paths tests/test_gpu_api.py never reaches: the
unstaged half of k_tx_parse and its 4096-word threshold, k_scan_chunks' carry, tiles without a newline,
unaligned device text, bytes past the end, several malformed records, the capacity protocol.

Expected values come from tests/textparse_ref.py (an independent restatement of the Java rules); the
oracle must agree with it wherever it is asked too.  Every test asserts through textparse_ref.plan()
that its input reaches the path it is named for, so a changed constant in gs_text.hip fails here
instead of quietly losing the coverage."""
import ctypes
import re

import numpy as np
import pytest
import torch

import textparse_ref as ref
from test_oracle_golden import BAD_RECORDS

pytestmark = pytest.mark.gpu

JUNK = b"junk 17 -x 0x1f\t+ "      # what pads a line: fields after the third are ignored


def _pad(line, k):
    """line with k more bytes of ignored fields (k >= 0)"""
    if k == 0:
        return line
    j = b" " + JUNK * ((k - 1) // len(JUNK) + 1)
    return line + j[:k]


def _short_lines(rng, n):
    """n valid records of 5..60 bytes"""
    a = rng.integers(-(1 << 40), 1 << 40, n)
    b = rng.integers(0, 1 << 62, n)
    c = rng.integers(-(1 << 63), (1 << 63) - 1, n)
    a[::3] = rng.integers(0, 100, len(a[::3]))
    b[::4] = rng.integers(0, 10, len(b[::4]))
    c[::5] = rng.integers(-9, 10, len(c[::5]))
    return [b"%d %d %d" % (int(x), int(y), int(z)) for x, y, z in zip(a, b, c)]


def _long_lines(rng, n, lo, hi):
    """n valid records padded to lo..hi bytes"""
    return [_pad(s, int(k) - len(s)) for s, k in zip(_short_lines(rng, n), rng.integers(lo, hi + 1, n))]


def _fill(rng, nbytes, lo=None, hi=None):
    """lines whose bytes, newlines included, add up to exactly nbytes; padded to lo..hi bytes when given"""
    out, left = [], nbytes
    reserve = 2 * (hi or 64) + 2
    while left > reserve:
        batch = _long_lines(rng, 64, lo, hi) if lo else _short_lines(rng, 64)
        for s in batch:
            if left <= reserve:
                break
            out.append(s)
            left -= len(s) + 1
    s = _short_lines(rng, 1)[0]
    out.append(_pad(s, left - 1 - len(s)))
    assert sum(len(x) + 1 for x in out) == nbytes
    return out


def _join(lines, final_newline=True):
    return b"\n".join(lines) + (b"\n" if final_newline else b"")


def _oracle_verdict(oracle, text):
    try:
        return oracle.parse_edges_text(text), None
    except ValueError as e:
        return None, int(re.search(r"record (\d+)$", str(e)).group(1))


def _same(got, want):
    assert len(got) == 3
    for g, w in zip(got, want):
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        assert g.dtype == np.int64 and w.dtype == np.int64 and np.array_equal(g, w)


def _check(engine, text, oracle=None, arg=None, want=None, **kw):
    """The library on `arg` (default: the host bytes) against the reference on `text`; returns the
    reference's (columns, first bad record)."""
    from gelly_streaming_amd import GsError, _lib

    cols, bad = want if want is not None else ref.parse(text)
    if oracle is not None:
        ocols, obad = _oracle_verdict(oracle, text)
        assert obad == bad
        if bad is None:
            _same(ocols, cols)
    if bad is None:
        _same(engine.parse_edges_text(text if arg is None else arg, **kw), cols)
    else:
        with pytest.raises(GsError, match=f"record {bad} ") as e:
            engine.parse_edges_text(text if arg is None else arg, **kw)
        assert e.value.status == _lib.GS_EINVAL
    return cols, bad


def _cuda(text, lead=0):
    """the text on the device, `lead` bytes into its allocation"""
    buf = torch.zeros(lead + len(text), dtype=torch.uint8, device="cuda")
    buf[lead:] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    return buf[lead:]


# ---- rules in bulk --------------------------------------------------------------------------------

def test_accepted_records_in_bulk(engine, oracle):
    """Every record either family accepts, and every accepted one-change variant of "7 -2 9", shuffled
    and repeated over many parse blocks: bit-equal columns."""
    recs = list(ref.accepted_family_records())
    assert len(recs) == 224 + 2529
    recs += [v for v in ref.nominal_variants() if ref.parse_record(v[:-1] if v.endswith(b"\r") else v)]
    rng = np.random.default_rng(0x7E47)
    recs = [recs[i] for i in np.concatenate([rng.permutation(len(recs)) for _ in range(2)])]
    text = _join(recs)
    p = ref.plan(text)
    assert p.records == len(recs) > 5000 and len(p.block_words) >= 20
    cols, bad = _check(engine, text, oracle)
    assert bad is None and {-(1 << 63), (1 << 63) - 1, 0, 7} <= set(cols[0].tolist())
    _check(engine, text[:-1], oracle, want=(cols, None))


def test_whole_grid_fails_at_the_first_bad_record(engine, oracle):
    """The unfiltered grid as one text: thousands of malformed records over a hundred blocks, the
    lowest index is reported.  Then the same with the leading rejects cut off, so that the first bad
    record is not record 0."""
    recs = list(ref.grid_records())
    text = _join(recs)
    assert ref.plan(text).records == len(recs) == 31320
    _, bad = _check(engine, text, oracle)
    assert bad is not None
    ok = [ref.parse_record(r[:-1] if r.endswith(b"\r") else r) is not None for r in recs]
    first_ok = ok.index(True)
    run = ok.index(False, first_ok) - first_ok
    assert run >= 1
    _, bad = _check(engine, _join(recs[first_ok:]), oracle)
    assert bad == run


# ---- rejects, one call each -----------------------------------------------------------------------

def _placement_base():
    """1024 good records: blocks 0, 1 and 3 staged, block 2 (lines of ~100 bytes) unstaged"""
    rng = np.random.default_rng(0xBA5E)
    return _short_lines(rng, 512) + _long_lines(rng, 256, 90, 110) + _short_lines(rng, 256)


PLACEMENTS = [("record 0", 0, True, True), ("last, final newline", 1023, True, True),
              ("last, no final newline", 1023, False, True), ("middle of a staged block", 384, True, True),
              ("inside an unstaged block", 512 + 77, True, False)]


def test_each_reject_alone_in_good_text(engine, oracle):
    base = _placement_base()
    rejects = [v for v in ref.nominal_variants() + BAD_RECORDS
               if ref.parse_record(v[:-1] if v.endswith(b"\r") else v) is None]
    assert len(rejects) > 60
    used = set()
    for i, v in enumerate(rejects):
        for j in range(len(PLACEMENTS)):
            name, at, final_nl, staged = PLACEMENTS[(i + j) % len(PLACEMENTS)]
            text = _join(base[:at] + [v] + base[at + 1:], final_nl)
            want = ref.parse(text)
            if want[1] == at:      # b"" as the last record without a newline is no record: next placement
                break
        assert want[1] == at, v
        p = ref.plan(text)
        assert bool(p.block_staged[p.block_of(at)]) == staged and list(p.block_staged[:2]) == [True, True], (v, name)
        _check(engine, text, oracle, want=want)
        used.add(name)
    assert used == {p[0] for p in PLACEMENTS}


# ---- several bad records --------------------------------------------------------------------------

def test_first_of_several_bad_records_wins(engine, oracle):
    rng = np.random.default_rng(0x5E7)
    good = _short_lines(rng, 256 * 9 + 40)
    spots = {"block0": 200, "middle": 256 * 4 + 3, "last": 256 * 9 + 39}
    for where, want_bad in ((["last", "middle", "block0"], 200), (["last", "middle"], 256 * 4 + 3),
                            (["last"], 256 * 9 + 39), (["block0", "last"], 200)):
        lines = list(good)
        for w in where:
            lines[spots[w]] = b"1 2 x"
        text = _join(lines)
        assert len(ref.plan(text).block_words) == 10
        _, bad = _check(engine, text, oracle)
        assert bad == want_bad
        # the failed call leaves nothing behind: a good text parses on the same engine
        cols, bad = _check(engine, _join(good), oracle)
        assert bad is None and len(cols[0]) == len(good)


# ---- the unstaged path and its threshold ----------------------------------------------------------

def test_every_block_unstaged(engine, oracle):
    rng = np.random.default_rng(0x0A)
    lines = _long_lines(rng, 3000, 90, 115)
    for final_nl in (True, False):
        text = _join(lines, final_nl)
        p = ref.plan(text)
        assert p.records == 3000 and len(p.block_staged) == 12 and not p.block_staged.any()
        assert _check(engine, text, oracle)[1] is None


def test_one_long_line_among_short_ones(engine, oracle):
    rng = np.random.default_rng(0x0B)
    lines = _short_lines(rng, 1000)
    lines[300] = _pad(lines[300], 20 * 1024)
    text = _join(lines)
    p = ref.plan(text)
    assert list(p.block_staged) == [True, False, True, True]
    assert _check(engine, text, oracle)[1] is None
    lines[300] = lines[300][:-1] + b"\x00"       # a bad byte at the far end of the junk changes nothing
    lines[301] = b"1 2"                          # and a short reject right after the long line is found
    text = _join(lines)
    assert list(ref.plan(text).block_staged) == [True, False, True, True]
    assert _check(engine, text, oracle)[1] == 301


def _threshold_text(rng, offset, words):
    """block 0 ends at a byte offset = `offset` (mod 4); block 1 spans exactly `words` words"""
    b0 = _short_lines(rng, 256)
    b0[17] = _pad(b0[17], (offset - sum(len(s) + 1 for s in b0)) % 4)
    span = 4 * words - offset                    # the most bytes that still round up to `words` words
    b1 = _short_lines(rng, 256)
    b1[100] = _pad(b1[100], span - sum(len(s) + 1 for s in b1))
    return _join(b0 + b1 + _short_lines(rng, 10))


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_staging_threshold(engine, oracle, offset):
    rng = np.random.default_rng(0x0C + offset)
    for words, staged in ((ref.LDS_WORDS, True), (ref.LDS_WORDS + 1, False), (ref.LDS_WORDS - 1, True)):
        text = _threshold_text(rng, offset, words)
        p = ref.plan(text)
        assert p.starts[256] % 4 == offset and p.block_words[1] == words
        assert list(p.block_staged) == [True, staged, True]
        assert _check(engine, text, oracle)[1] is None


def test_crlf_and_open_last_record_in_unstaged_blocks(engine, oracle):
    rng = np.random.default_rng(0x0D)
    lines = _long_lines(rng, 700, 90, 115)
    crlf = b"\r\n".join(lines) + b"\r\n"
    for text in (crlf, crlf[:-1], crlf[:-2], crlf[:-2] + b"\r\r"):
        p = ref.plan(text)
        assert p.records == 700 and not p.block_staged.any()
        assert _check(engine, text, oracle)[1] is None
    # a lone CR line is an empty record
    text = crlf + b"\r\n" + crlf
    assert not ref.plan(text).block_staged[700 // ref.BLOCK_RECORDS]
    assert _check(engine, text, oracle)[1] == 700


# ---- tiles and granules ---------------------------------------------------------------------------

def test_lines_longer_than_a_tile(engine, oracle):
    rng = np.random.default_rng(0x1A)
    lines = _short_lines(rng, 600)
    lines[5] = _pad(lines[5], 17 * 1024)
    lines[400] = _pad(lines[400], 40 * 1024)
    lines.append(_pad(b"3 2 1", 17 * 1024))
    for final_nl in (True, False):
        text = _join(lines, final_nl)
        p = ref.plan(text)
        assert (p.tile_newlines == 0).sum() >= 1                # 40 KiB cover a whole tile wherever they start
        s, e = int(p.starts[400]), int(p.starts[401])
        assert (e - 1) // ref.TILE - s // ref.TILE >= 2         # the record crosses two tile edges or more
        assert (int(p.starts[6]) - 1) // ref.TILE > int(p.starts[5]) // ref.TILE
        assert _check(engine, text, oracle)[1] is None


@pytest.mark.parametrize("j", [-1, 0, 1, 15, 16])
def test_newline_next_to_a_tile_edge(engine, oracle, j):
    rng = np.random.default_rng(0x1B + j)
    lines, pos = [], 0
    targets = [ref.TILE * k + j for k in (1, 2, 3)]
    for t in targets:
        for s in _short_lines(rng, 2000):
            if pos + len(s) + 1 + 80 > t:
                break
            lines.append(s)
            pos += len(s) + 1
        s = _short_lines(rng, 1)[0]
        lines.append(_pad(s, t - pos - len(s)))
        pos = t + 1
    lines += _short_lines(rng, 20)
    text = _join(lines)
    a = np.frombuffer(text, np.uint8)
    assert all(a[t] == 10 for t in targets) and ref.plan(text).tiles == 4
    assert _check(engine, text, oracle)[1] is None
    # the record after the edge newline is the bad one
    at = int(np.searchsorted(ref.plan(text).starts, targets[1] + 1))
    assert ref.plan(text).starts[at] == targets[1] + 1
    lines[at] = b"+ 1 2"
    assert _check(engine, _join(lines), oracle)[1] == at


def test_every_length_residue_mod_16(engine, oracle):
    rng = np.random.default_rng(0x1C)
    seen = set()
    for r in range(16):
        for final_nl in (True, False):
            n = 40 * 1024 + 16 + r
            lines = _fill(rng, n + (0 if final_nl else 1))
            text = _join(lines, final_nl)
            assert len(text) == n and len(text) % 16 == r and (text[-1:] == b"\n") == final_nl
            assert _check(engine, text, oracle)[1] is None
            seen.add((len(text) % 16, final_nl))
    assert len(seen) == 32
    # and plain truncation, which may cut a record short: whatever the reference says
    text = _join(_fill(rng, 40 * 1024) + [b"1 2 3", b"12 34 567"])
    assert len(text) % 16 == 0
    verdicts = {_check(engine, text[:len(text) - k], oracle)[1] is None for k in range(16)}
    assert verdicts == {True, False}


@pytest.mark.parametrize("n", [16383, 16384, 16385, 32768])
def test_total_length_at_a_tile_edge(engine, oracle, n):
    rng = np.random.default_rng(n)
    for final_nl in (True, False):
        text = _join(_fill(rng, n + (0 if final_nl else 1)), final_nl)
        assert len(text) == n and ref.plan(text).tiles == (n + ref.TILE - 1) // ref.TILE
        assert _check(engine, text, oracle)[1] is None


# ---- the scan's carry -----------------------------------------------------------------------------

def _segments(rng, segs):
    """[(bytes, dense)]: dense segments are short lines, the others lines of about 4 KiB"""
    lines = []
    for nbytes, dense in segs:
        lines += _fill(rng, nbytes) if dense else _fill(rng, nbytes, 3900, 4300)
    return lines


T = ref.TILE
SCAN_CASES = {
    # exactly 1024 tiles, full to the last byte: the last text without a carry
    "1024": ([(1024 * T, False)], True, 1024, 1),
    # tile 1023 holds ~4 newlines, tile 1024 hundreds: the carry meets a dense first tile
    "1025": ([(1024 * T, False), (5000, True)], False, 1025, 2),
    # dense tiles right before the chunk edge at 1024, sparse after; a third chunk of one tile
    "2049": ([(1021 * T, False), (3 * T, True), (1024 * T, False), (100, True)], True, 2049, 3),
}


@pytest.mark.parametrize("case", list(SCAN_CASES))
def test_scan_carry(engine, oracle, case):
    segs, final_nl, tiles, chunks = SCAN_CASES[case]
    rng = np.random.default_rng(tiles)
    text = _join(_segments(rng, segs), final_nl)
    p = ref.plan(text)
    assert p.tiles == tiles and p.scan_chunks == chunks and len(text) == sum(s[0] for s in segs) - (not final_nl)
    if case == "1025":
        assert p.tile_newlines[1023] <= 5 and p.tile_newlines[1024] >= 100
    if case == "2049":
        assert p.tile_newlines[1021:1024].min() >= 300 and p.tile_newlines[1024] <= 5 and p.tile_newlines[2048] >= 1
    cols, bad = _check(engine, text, oracle)
    assert bad is None and len(cols[0]) == p.records < 20000


# ---- device text placement ------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["staged", "unstaged"])
def test_unaligned_device_text(engine, oracle, kind):
    rng = np.random.default_rng(0x2A)
    lines = _short_lines(rng, 1500) if kind == "staged" else _long_lines(rng, 1500, 90, 115)
    for final_nl in (True, False):
        text = _join(lines, final_nl)
        p = ref.plan(text)
        assert p.block_staged.all() if kind == "staged" else not p.block_staged.any()
        want = _check(engine, text, oracle)
        assert want[1] is None
        for lead in (1, 3, 8, 15):
            dev = _cuda(text, lead)
            assert dev.data_ptr() % 16 == lead and dev.numel() == len(text)
            _check(engine, text, arg=dev, want=want)
    text = _join(lines[:700] + [b"1 2 3.0"] + lines[700:])
    want = _check(engine, text, oracle)
    assert want[1] == 700
    _check(engine, text, arg=_cuda(text, 3), want=want)


@pytest.mark.parametrize("trailer", [b"\n9 9 9\n1 1", b"777\n9 9 9\n1 1"])
def test_bytes_past_the_end_of_aligned_device_text(engine, oracle, trailer):
    rng = np.random.default_rng(0x2B)
    trailer = trailer + b"23456789" * 4
    for r in (1, 7, 15):
        for final_nl in (True, False):
            n = 5 * 1024 + r
            text = _join(_fill(rng, n + (0 if final_nl else 1)), final_nl)
            assert len(text) == n and n % 16 == r
            buf = torch.zeros(16 + n + len(trailer), dtype=torch.uint8, device="cuda")
            buf[16:] = torch.from_numpy(np.frombuffer(text + trailer, np.uint8).copy()).cuda()
            dev = buf[16:16 + n]
            assert dev.data_ptr() % 16 == 0         # read in place: the bytes after it are the trailer's
            want = _check(engine, text, oracle)
            assert want[1] is None
            _check(engine, text, arg=dev, want=want)
            _check(engine, text, arg=dev, want=want, out_device=False)


def test_stale_bytes_in_the_reused_staging_buffer(engine, oracle):
    rng = np.random.default_rng(0x2C)
    big = _join(_fill(rng, 1 << 20))
    assert _check(engine, big, oracle)[1] is None
    small = b"11 22 33\n44 55 66\n-7 +8 9\n12345 6 789"
    assert len(small) == 37
    cols, bad = _check(engine, small, oracle)
    assert bad is None and cols[2].tolist() == [33, 66, 9, 789]


# ---- the ABI's two-phase protocol -------------------------------------------------------------------

def _abi_call(pkg, engine, text, cols, cap, out_mem, dev_text=None):
    lib = pkg.load_library()
    from gelly_streaming_amd import _lib
    n_out, bad = ctypes.c_uint64(123), ctypes.c_uint64(5)
    if dev_text is not None:
        ptr, in_mem = ctypes.c_void_p(dev_text.data_ptr()), _lib.GS_MEM_DEVICE
    else:
        host = np.frombuffer(text, np.uint8)
        ptr, in_mem = (ctypes.c_void_p(host.ctypes.data) if len(text) else None), _lib.GS_MEM_HOST
    ps = [None if c is None else ctypes.c_void_p(c.data_ptr() if hasattr(c, "data_ptr") else c.ctypes.data)
          for c in cols]
    st = lib.gs_parse_edges_text(engine.ctx, ptr, len(text), in_mem, ps[0], ps[1], ps[2], cap, out_mem,
                                 ctypes.byref(n_out), ctypes.byref(bad))
    return st, n_out.value, bad.value


@pytest.mark.parametrize("out", ["device", "host"])
def test_abi_capacity_protocol(pkg, engine, oracle, out):
    from gelly_streaming_amd import _lib
    rng = np.random.default_rng(0x3A)
    out_mem = _lib.GS_MEM_DEVICE if out == "device" else _lib.GS_MEM_HOST
    none = ~0 & 0xFFFFFFFFFFFFFFFF

    def columns(n):
        if out == "device":
            return [torch.full((max(n, 1),), -77, dtype=torch.int64, device="cuda") for _ in range(3)]
        return [np.full(max(n, 1), -77, np.int64) for _ in range(3)]

    for final_nl in (True, False):
        text = _join(_short_lines(rng, 777), final_nl)
        want, bad = ref.parse(text)
        n = len(want[0])
        assert bad is None and n == 777
        for dev_text in (None, _cuda(text)):
            assert _abi_call(pkg, engine, text, [None] * 3, 0, out_mem, dev_text) == (_lib.GS_ECAPACITY, n, none)
            assert b"777 records" in pkg.load_library().gs_last_error(engine.ctx)
            short = columns(n - 1)
            assert _abi_call(pkg, engine, text, short, n - 1, out_mem, dev_text) == (_lib.GS_ECAPACITY, n, none)
            cols = columns(n)
            assert _abi_call(pkg, engine, text, cols, n, out_mem, dev_text) == (_lib.GS_OK, n, none)
            _same(cols, want)
            roomy = columns(n + 5)
            assert _abi_call(pkg, engine, text, roomy, n + 5, out_mem, dev_text) == (_lib.GS_OK, n, none)
            _same([c[:n] for c in roomy], want)
            tail = [c[n:].cpu().numpy() if hasattr(c, "cpu") else c[n:] for c in roomy]
            assert all((t == -77).all() for t in tail)       # nothing is written past the records
    # a malformed record: the count and the index both come back
    text = _join(_short_lines(rng, 300) + [b"1 2"] + _short_lines(rng, 300))
    assert _abi_call(pkg, engine, text, columns(601), 601, out_mem) == (_lib.GS_EINVAL, 601, 300)
    # sizing alone does not look at the records
    assert _abi_call(pkg, engine, text, [None] * 3, 0, out_mem) == (_lib.GS_ECAPACITY, 601, none)
    # no bytes: no records, with or without buffers
    assert _abi_call(pkg, engine, b"", [None] * 3, 0, out_mem) == (_lib.GS_OK, 0, none)
    assert _abi_call(pkg, engine, b"", columns(4), 4, out_mem) == (_lib.GS_OK, 0, none)


# ---- the wrapper's capacity -------------------------------------------------------------------------

def test_wrapper_capacity_never_hides_the_bad_record(engine, oracle):
    from gelly_streaming_amd import GsError
    for text, bad in ((b"1 2 3\n" + b"\n" * 100, 1), (b"\n" * 50, 0), (b"1 2 3\n4 5 6\n" + b"\r\n" * 40, 2),
                      (b"\n", 0), (b"\r", 0)):
        assert ref.parse(text) == (None, bad) and _oracle_verdict(oracle, text) == (None, bad)
        for arg in (text, _cuda(text)):
            for out_device in (True, False):
                with pytest.raises(GsError, match=f"record {bad} "):
                    engine.parse_edges_text(arg, out_device=out_device)
    assert [len(x) for x in engine.parse_edges_text(b"")] == [0, 0, 0]
