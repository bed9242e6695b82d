"""replace_substring (arrow_amd.compute, csrc/string_replace.hip) against pyarrow.compute on the host copy of the same
array: values, validity, null_count and offset 0, exact equality.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus one column of 10^6 rows built from numpy buffers.  Both forms are reached through
compute.STRING_REPLACE_PATH (1 = one lane per row, 2 = one wave per row, 0 = the library chooses); large offsets, a null
row over bytes that hold the pattern, the refused arguments and the int32 overflow go through the C ABI.

The reference is never called with an empty pattern and unlimited replacements: it does not terminate."""
import ctypes as C

import numpy as np
import pytest

from . import string_util
from .string_util import c_buffers, path_set, same, sync

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

LENGTHS = [0, 1, 63, 64, 65, 4097]
ROW_COUNTER, WAVE_COUNTER = b"string_replace_row_launches", b"string_replace_wave_launches"
AUTO, ROWS, WAVES = 0, 1, 2
PATTERNS = {1: "a", 2: "ab", 8: "abcdefgh", 9: "aabaabaac", 17: "0123456789abcdefg"}   # by length; the 9 overlaps itself
LONG = "".join(chr(65 + (i * 7 + i // 26) % 26) for i in range(1025))                   # 1025 bytes: past the LDS cap
ROW_BYTES = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097]
SEED = 0x4E91
KNOB = "STRING_REPLACE_PATH"              # the global of arrow_amd.compute that selects the kernel form


def rng_for(*key):
    return string_util.rng_for(SEED, *key)


def replacements(pattern):
    """Replacements of 0, 1, m and m + 3 bytes."""
    m = len(pattern)
    return ["", "Z", ("xy" * m)[:m], ("<" + pattern + ">>")[: m + 3]]


def triples(patterns=tuple(PATTERNS.values())):
    """(pattern, replacement, max_replacements): every pattern length with every replacement length, the values of
    max_replacements dealt round: None, -1, -5, 0, 1, 2 and more than any row holds."""
    caps = [None, -1, -5, 0, 1, 2, 10**6]
    out = []
    for pattern in patterns:
        for rep in replacements(pattern):
            out.append((pattern, rep, caps[len(out) % len(caps)]))
    return out


def check(amd, host, dev, todo, paths=(ROWS, WAVES)):
    binary = pa.types.is_binary(host.type) or pa.types.is_large_binary(host.type)
    for pattern, rep, cap in todo:
        if binary and isinstance(pattern, str):
            pattern, rep = pattern.encode(), rep.encode()
        want = pc.replace_substring(host, pattern, rep, max_replacements=cap)
        for path in paths:
            with path_set(amd, KNOB, path):
                got = amd.compute.replace_substring(dev, pattern, rep, max_replacements=cap)
            same(got, want, host, (host.type, pattern[:20], rep[:20], cap, path, len(host)))
            assert got.type == dev.type


# ---------------------------------------------------------------- rows
def row_pool(rng):
    """Short rows over a small alphabet with every pattern of PATTERNS planted: alone, at either end, twice, adjacent."""
    rows = ["", "a", "b", "ab", "ba", "aab", "abab", "xyz", "abcdefg", "aabaabaa", "0123456789abcdef"]
    for p in PATTERNS.values():
        rows += [p, p + p, "x" + p, p + "x", "xx" + p + "yy" + p, p[:-1], p[1:], p + p[:-1], "q" * 13 + p + "r" * 20 + p + p]
    for _ in range(30):
        rows.append("".join("abc"[i] for i in rng.integers(0, 3, rng.integers(0, 40))))
    return rows


def column(rng, n, null_p, typ):
    pool = row_pool(rng)
    mask = (rng.random(n) < null_p) if null_p else None
    return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask).cast(typ)


def _grid(amd, n):
    """Both types, both null shares, whole and as slice(7) of n + 7 rows; both forms forced."""
    todo = triples()
    for k, typ in enumerate((pa.string(), pa.binary())):
        for j, null_p in enumerate((0.0, 0.1)):
            arr = column(rng_for("grid", n, typ, null_p), n + 7, null_p, typ)
            dev = amd.Array.from_pyarrow(arr)
            part = todo[2 * k + j::4] if n > 1000 else todo      # the large count: each triple on one type and null share
            check(amd, arr.slice(7), dev.slice(7), part)         # n rows, first offset non-zero, odd validity bit offset
            check(amd, arr.slice(0, n), dev.slice(0, n), part[::3])


def _row_lengths(amd):
    """Rows of every length of ROW_BYTES and of m - 1, m, m + 1: filler, the pattern at the front, at the back, at both,
    and rows that are nothing but matches."""
    for m, p in PATTERNS.items():
        rows = []
        for size in sorted(set(ROW_BYTES + [m - 1, m, m + 1])):
            rows += ["x" * size, (p * (size // m + 1))[:size], ("ba" * size)[:size]]
            if size >= m:
                rows += [p + "x" * (size - m), "x" * (size - m) + p, p * (size // m) + "y" * (size % m)]
            if size >= 2 * m:
                rows.append(p + "-" * (size - 2 * m) + p)
        arr = pa.array(rows, pa.string())
        assert set(ROW_BYTES) <= set(pc.binary_length(arr).to_pylist())
        check(amd, arr, amd.Array.from_pyarrow(arr), [(p, rep, cap) for rep, cap in zip(replacements(p), (None, 2, -1, 1))])


def _long_literals(amd):
    """A pattern and a replacement of 1025 bytes: past the LDS cap, read where they lie."""
    rows = ["", "x", LONG, LONG[:-1], LONG[1:], "x" + LONG, LONG + "x", LONG + LONG, "ab" + LONG + "cd" + LONG + LONG[:700], "ab" * 900]
    arr = pa.array(rows + [None] + rows[::-1], pa.string())
    dev = amd.Array.from_pyarrow(arr)
    check(amd, arr, dev, [(LONG, "", None), (LONG, "Z", 1), (LONG, LONG[::-1], -1), (LONG, "[" + LONG[:1024], 2),
                          ("ab", LONG, None), ("ab", LONG[:1024], 3), (LONG[:1024], "cd", None)])


def _constructed(amd):
    """The greedy rule and the boundaries a match may straddle."""
    rows = ["aaa", "aaaa", "aaaaa", "abababa", "a", "", "aa", "baab", "aabaa"]
    arr = pa.array(rows, pa.string())
    dev = amd.Array.from_pyarrow(arr)
    for path in (ROWS, WAVES):
        with path_set(amd, KNOB, path):
            cp = amd.compute
            assert cp.replace_substring(dev, "aa", "b").to_pyarrow().to_pylist() == ["ba", "bb", "bba", "abababa", "a", "", "b", "bbb", "bbb"]
            assert cp.replace_substring(dev, "aba", "X").to_pyarrow().to_pylist()[3] == "XbX"
            assert cp.replace_substring(dev, "aa", "aaa").to_pyarrow().to_pylist()[1] == "aaaaaa"      # never re-scanned
            assert cp.replace_substring(dev, "aa", "aaa", max_replacements=1).to_pyarrow().to_pylist()[1] == "aaaaa"
    check(amd, arr, dev, [("aa", "b", None), ("aba", "X", None), ("aa", "aaa", None), ("aa", "aaa", 1), ("aa", "", -1), ("a", "aa", 2)])
    # a match at byte 0, one ending at the row's last byte, rows that are nothing but matches
    for p in ("ab", "aabaabaac", "0123456789abcdefg"):
        edge = pa.array([p, p + "tail", "head" + p, p * 2, p * 7, p * 130, p[:-1] + p, p + p[1:]], pa.string())
        check(amd, edge, amd.Array.from_pyarrow(edge), [(p, "", None), (p, "<" + p + ">", None), (p, "#", 3)])
    # two adjacent rows whose concatenation holds the pattern across the row boundary: no match
    split = pa.array(["xxab", "cdxx", "ab", "cd", "abcdefgh012345678"[:9], "abcdefgh012345678"[9:], "abc", "d"], pa.string())
    for p in ("abcd", "bc", "abcdefgh012345678", "cd"):
        check(amd, split, amd.Array.from_pyarrow(split), [(p, "!", None)])
    assert pc.replace_substring(split, "abcdefgh012345678", "!").to_pylist() == split.to_pylist()
    assert pc.replace_substring(split, "abcd", "!").to_pylist()[:4] == split.to_pylist()[:4]
    # binary rows: '\0' and 0xff are ordinary bytes
    raw = pa.array([b"a\x00\xffb", b"\x00\xff\x00\xff", b"\xff\x00", b"\x00" * 20 + b"\xff" * 20, b"", None, b"\x00\xff"], pa.binary())
    check(amd, raw, amd.Array.from_pyarrow(raw), [(b"\x00\xff", b"\xff\x00\x00", -5), (b"\x00", b"", None), (b"\xff\xff", b"\x00", 1),
                                                  (b"\x00\xff", b"\x00\xff\x00\xff", None)])


def _straddles(amd):
    """Matches across an 8-byte word, a 16-byte granule and the 1024-byte tile of the waves form: the rows sweep every
    alignment of the match against the buffer, whatever the buffer's own."""
    for p in ("ab", "aabaabaac", "0123456789abcdefg"):
        m = len(p)
        rows = []
        for pad in range(33):                                    # 3 pads, 2 matches: every position modulo 16 (and 8)
            rows += ["#" * pad, "x" * 5 + p + "y" * 3 + p, p]
        for q in range(1024 - m - 16, 1024 + 17):                # one match at q, one right behind it, around the tile's end
            rows.append("." * q + p + p + "." * (1100 - q - 2 * m))
        arr = pa.array(rows, pa.string())
        offsets = np.frombuffer(arr.buffers()[1], np.int32)[: len(rows) + 1]
        starts = offsets[1:3 * 33:3] + 5                         # where the first match of a short row begins
        assert set(starts % 16) == set(range(16))
        check(amd, arr, amd.Array.from_pyarrow(arr), [(p, "", None), (p, "0123456789abcdefghij", None), (p, "Q" * m, 1)])


def _auto_and_counters(amd):
    """The launch counters rise on the forced form only (one launch in each of the two calls); auto takes rows for short
    rows and waves for long ones, with the same results."""
    from arrow_amd import _lib

    lib = _lib.get_lib()
    short = pa.array(["xxabxx", None, "ab", ""] * 40, pa.string())
    long_ = pa.array([("ab" + "x" * 30) * 128, None, "ab" * 2048, "y" * 4096] * 3, pa.string())
    for arr, auto_counter in ((short, ROW_COUNTER), (long_, WAVE_COUNTER)):
        dev = amd.Array.from_pyarrow(arr)
        want = pc.replace_substring(arr, "ab", "<ab>")
        for path, counter in ((ROWS, ROW_COUNTER), (WAVES, WAVE_COUNTER), (AUTO, auto_counter)):
            before = {c: lib.arx_get_counter(c) for c in (ROW_COUNTER, WAVE_COUNTER)}
            with path_set(amd, KNOB, path):
                got = amd.compute.replace_substring(dev, "ab", "<ab>")
            same(got, want, arr, (path, len(arr)))
            for c in (ROW_COUNTER, WAVE_COUNTER):
                assert lib.arx_get_counter(c) == before[c] + (2 if c == counter else 0), (path, c)
    check(amd, short, amd.Array.from_pyarrow(short), triples(("ab",)), paths=(AUTO,))
    check(amd, long_, amd.Array.from_pyarrow(long_), triples(("ab",)), paths=(AUTO,))


def _all_null_and_all_empty(amd):
    for arr in (pa.array([None] * 70, pa.string()), pa.array([""] * 70, pa.string()), pa.array(["ab"] * 70, pa.binary()),
                pa.array([], pa.string())):
        check(amd, arr, amd.Array.from_pyarrow(arr), [("ab", "", None), ("ab", "xyz", 1)])


def _mirror(amd):
    s = pa.array(["héllo wörld", None, "", "日本日本x"], pa.string())
    ds = amd.Array.from_pyarrow(s)
    cp = amd.compute
    same(cp.call_function("replace_substring", [ds], cp.ReplaceSubstringOptions("ö", "oe")), pc.replace_substring(s, "ö", "oe"), s, "options")
    same(cp.call_function("replace_substring", [ds], cp.ReplaceSubstringOptions("日本", "", max_replacements=1)),
         pc.replace_substring(s, "日本", "", max_replacements=1), s, "max_replacements")
    same(cp.replace_substring(ds, b"l", b"L", max_replacements=-7), pc.replace_substring(s, "l", "L"), s, "bytes literals")
    sliced = cp.replace_substring(ds.slice(1), "日", "x")         # the null count of a slice is not known: lazy
    assert sliced.null_count == 1 and sliced.to_pyarrow().to_pylist() == [None, "", "x本x本x"]
    with pytest.raises(amd.ArrowInvalid, match="Function 'replace_substring' cannot be called without options"):
        cp.call_function("replace_substring", [ds])
    for cap in (None, -1, 0, 2):
        with pytest.raises(amd.ArrowNotImplementedError, match="replace_substring with an empty pattern"):
            cp.replace_substring(ds, "", "x", max_replacements=cap)
    with pytest.raises(amd.ArrowNotImplementedError, match="replace_substring of a scalar"):
        cp.call_function("replace_substring", [amd.Scalar("a", ds.type, True)], cp.ReplaceSubstringOptions("a", "b"))
    with pytest.raises(TypeError, match="pattern must be str or bytes"):
        cp.replace_substring(ds, 3, "x")
    for host in (pa.array([1, 2, 3]), pa.array([True])):
        with pytest.raises(pa.ArrowNotImplementedError) as want_err:
            pc.replace_substring(host, "a", "b")
        with pytest.raises(pa.ArrowNotImplementedError) as got_err:
            cp.replace_substring(amd.Array.from_pyarrow(host), "a", "b")
        assert str(got_err.value) == str(want_err.value)
        assert "has no kernel matching input types" in str(got_err.value)


# ---------------------------------------------------------------- the C ABI directly
def device_bytes(raw):
    from arrow_amd.array import to_device

    return to_device(np.frombuffer(bytes(raw) or b"\0", np.uint8).copy())


def c_replace(amd, arr, owidth, pattern, rep, cap, path, hint=None):
    """arx_replace_substring_offsets + _data on `arr`: (the output rows as bytes, the output offsets); the 0xEE guard
    words after the offsets and after the data survive."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    span, keep, nbytes = c_buffers(arr, owidth)
    n = len(arr)
    ws_bytes = lib.arx_replace_substring_workspace_bytes(n, owidth)
    ws = to_device(np.zeros(ws_bytes, np.uint8))
    out_offsets = to_device(np.full((n + 1) * owidth + 8, 0xEE, np.uint8))
    total = C.c_int64(-1)
    dpat, drep = device_bytes(pattern), device_bytes(rep)
    rc = lib.arx_replace_substring_offsets(C.byref(span), owidth, dpat.data_ptr(), len(pattern), len(rep), cap, nbytes if hint is None else hint,
                                           path, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), C.byref(total), None)
    assert rc == 0, lib.arx_last_error()
    out_data = to_device(np.full(total.value + 8, 0xEE, np.uint8))
    rc = lib.arx_replace_substring_data(C.byref(span), owidth, dpat.data_ptr(), len(pattern), drep.data_ptr() if rep else None, len(rep), cap,
                                        path, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), total.value, out_data.data_ptr(), None)
    assert rc == 0, lib.arx_last_error()
    sync(out_data)
    raw_o, raw_d = out_offsets.cpu().numpy(), out_data.cpu().numpy()
    assert (raw_o[(n + 1) * owidth: (n + 1) * owidth + 8] == 0xEE).all()
    assert (raw_d[total.value: total.value + 8] == 0xEE).all()
    offsets = raw_o[: (n + 1) * owidth].view(np.int32 if owidth == 4 else np.int64).copy()
    assert offsets[0] == 0 and offsets[-1] == total.value and (np.diff(offsets) >= 0).all()
    return [raw_d[offsets[i]: offsets[i + 1]].tobytes() for i in range(n)], offsets


def _large_offsets(amd):
    """large_utf8 / large_binary (offset_width 8) and the same rows with int32 offsets: the reference's rows for both."""
    small = column(rng_for("large"), 1000, 0.1, pa.string())
    a4, a8 = small.slice(5), small.cast(pa.large_string()).slice(5)
    b8 = small.cast(pa.large_binary()).slice(5)
    for pattern, rep, cap in triples(("ab", "aabaabaac")):
        want8 = pc.replace_substring(a8, pattern, rep, max_replacements=cap)
        assert want8.type == pa.large_string()
        assert pc.replace_substring(b8, pattern.encode(), rep.encode(), max_replacements=cap).cast(pa.large_string()).equals(want8)
        want = [b"" if r is None else r for r in want8.cast(pa.large_binary()).to_pylist()]
        for path in (ROWS, WAVES):
            rows8, off8 = c_replace(amd, a8, 8, pattern.encode(), rep.encode(), -1 if cap is None else cap, path)
            rows4, off4 = c_replace(amd, a4, 4, pattern.encode(), rep.encode(), -1 if cap is None else cap, path)
            assert rows8 == want and rows4 == want, (pattern, rep, cap, path)
            assert off8.dtype == np.int64 and off4.dtype == np.int32 and (off8 == off4).all()


def _null_row_spanning_bytes(amd):
    """A null row whose offsets span bytes that hold the pattern: it stays null and holds no bytes."""
    plain = pa.array(["xabx", "ababab", "ab", "b"], pa.string())
    arr = pa.Array.from_buffers(pa.string(), 4, [pa.py_buffer(bytes([0b1101])), plain.buffers()[1], plain.buffers()[2]])
    assert arr.to_pylist()[1] is None
    check(amd, arr, amd.Array.from_pyarrow(arr), [("ab", "ZZZ", None), ("ab", "", 1)])
    for path in (ROWS, WAVES):
        rows, offsets = c_replace(amd, arr, 4, b"ab", b"ZZZ", -1, path)
        assert offsets.tolist() == [0, 5, 5, 8, 9] and rows == [b"xZZZx", b"", b"ZZZ", b"b"]      # no byte of the null row


def _c_abi_contract(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    arr = pa.array(["xabx", "ab"], pa.string())
    span, keep, nbytes = c_buffers(arr, 4)
    ws_bytes = lib.arx_replace_substring_workspace_bytes(2, 4)
    assert ws_bytes == lib.arx_string_slice_workspace_bytes(2, 4)
    ws = to_device(np.zeros(ws_bytes + 8, np.uint8))
    out = to_device(np.full(64, 0xEE, np.uint8))
    data = to_device(np.full(64, 0xEE, np.uint8))
    total = C.c_int64(-1)
    lit = device_bytes(b"abQQ")
    pat_ptr, rep_ptr = lit.data_ptr(), lit.data_ptr() + 2

    def offsets(sp=span, width=4, pat=pat_ptr, m=2, r=2, cap=-1, path=ROWS, w=ws.data_ptr(), wb=ws_bytes, o=out, t=total):
        return lib.arx_replace_substring_offsets(C.byref(sp) if sp is not None else None, width, pat, m, r, cap, nbytes, path, w, wb,
                                                 o.data_ptr() if o is not None else None, C.byref(t) if t is not None else None, None)

    def write(sp=span, width=4, pat=pat_ptr, m=2, rep=rep_ptr, r=2, path=ROWS, w=ws.data_ptr(), wb=ws_bytes, o=out, tb=6, d=data):
        return lib.arx_replace_substring_data(C.byref(sp) if sp is not None else None, width, pat, m, rep, r, -1, path, w, wb,
                                              o.data_ptr() if o is not None else None, tb, d.data_ptr() if d is not None else None, None)

    neg = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, -1, 0)
    no_offsets = _lib.ArxBinarySpan(None, None, keep[2].data_ptr(), 0, 2, 0)
    no_data = _lib.ArxBinarySpan(None, keep[1].data_ptr(), None, 0, 2, 0)
    shared = [({"path": -1}, b"path -1"), ({"path": 3}, b"path 3"), ({"width": 2}, b"offset_width 2"), ({"width": 16}, b"offset_width 16"),
              ({"sp": neg}, b"negative length"), ({"m": 0}, b"pattern_length 0 is not positive"), ({"m": -1}, b"pattern_length -1 is not positive"),
              ({"r": -1}, b"negative replacement_length -1"), ({"pat": None}, b"NULL pattern or replacement"),
              ({"sp": no_offsets}, b"NULL"), ({"wb": ws_bytes - 1}, b"ws of"), ({"w": None}, b"ws of"), ({"w": ws.data_ptr() + 4}, b"ws of")]
    before = [lib.arx_get_counter(c) for c in (ROW_COUNTER, WAVE_COUNTER)]
    for kwargs, text in shared + [({"sp": None}, b"NULL values, out_offsets or out_total_bytes"),
                                  ({"o": None}, b"NULL values, out_offsets or out_total_bytes"),
                                  ({"t": None}, b"NULL values, out_offsets or out_total_bytes")]:
        assert offsets(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    for kwargs, text in shared + [({"sp": None}, b"NULL values"), ({"rep": None}, b"NULL pattern or replacement"),
                                  ({"tb": -1}, b"negative total_bytes -1"), ({"o": None}, b"NULL out_offsets, out_data"),
                                  ({"d": None}, b"NULL out_offsets, out_data"), ({"sp": no_data}, b"NULL out_offsets, out_data")]:
        assert write(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    sync(out)
    assert (out.cpu().numpy() == 0xEE).all() and (data.cpu().numpy() == 0xEE).all() and total.value == -1    # nothing written
    # length 0: success, nothing launched, nothing written but out_offsets[0] and the total
    empty = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, 0, 0)
    for width in (4, 8):
        total.value = -1
        assert offsets(sp=empty, width=width, w=None, wb=0) == 0 and total.value == 0
        assert write(sp=empty, width=width, w=None, wb=0, tb=0) == 0
        sync(out)
        raw = out.cpu().numpy()
        assert (raw[:width] == 0).all() and (raw[width:64] == 0xEE).all() and (data.cpu().numpy() == 0xEE).all()
        out[:64] = 0xEE
    assert write(tb=0) == 0                                      # nothing to write: nothing launched
    assert [lib.arx_get_counter(c) for c in (ROW_COUNTER, WAVE_COUNTER)] == before
    # a NULL replacement of length 0 deletes
    assert offsets(r=0) == 0 and total.value == 2, lib.arx_last_error()
    assert write(rep=None, r=0, tb=2) == 0, lib.arx_last_error()
    sync(data)
    assert out.cpu().numpy()[:12].view(np.int32).tolist() == [0, 2, 2] and data.cpu().numpy()[:3].tolist() == [ord("x"), ord("x"), 0xEE]
    assert [lib.arx_get_counter(c) for c in (ROW_COUNTER, WAVE_COUNTER)] == [before[0] + 2, before[1]]


def _overflow(amd):
    """4097 rows of 1024 x 'a', every byte replaced by 600: 2.5 x 10^9 bytes.  int32 offsets overflow in the scan; int64
    offsets give the total.  The output is never allocated: the data call is not made."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n, size, r = 4097, 1024, 600
    data = to_device(np.full(n * size, ord("a"), np.uint8))
    pat = device_bytes(b"a")
    for width, path in ((4, ROWS), (4, WAVES), (8, ROWS), (8, WAVES)):
        offs = to_device((np.arange(n + 1, dtype=np.int64) * size).astype(np.int32 if width == 4 else np.int64))
        span = _lib.ArxBinarySpan(None, offs.data_ptr(), data.data_ptr(), 0, n, 0)
        ws_bytes = lib.arx_replace_substring_workspace_bytes(n, width)
        ws = to_device(np.zeros(ws_bytes, np.uint8))
        out_offsets = to_device(np.zeros((n + 1) * width, np.uint8))
        total = C.c_int64(-1)
        rc = lib.arx_replace_substring_offsets(C.byref(span), width, pat.data_ptr(), 1, r, -1, n * size, path, ws.data_ptr(), ws_bytes,
                                               out_offsets.data_ptr(), C.byref(total), None)
        if width == 4:
            assert rc == _lib.ARX_INVALID and b"offset overflow while replacing substrings" in lib.arx_last_error(), (path, lib.arx_last_error())
        else:
            assert rc == 0, lib.arx_last_error()
            assert total.value == n * size * r
            sync(out_offsets)
            got = out_offsets.cpu().numpy()[: (n + 1) * 8].view(np.int64)
            assert (got == np.arange(n + 1, dtype=np.int64) * size * r).all()
    # the mirror reports the same overflow as ArrowInvalid
    arr = amd.Array.from_pyarrow(pa.array(["a" * size] * n, pa.string()))
    with pytest.raises(amd.ArrowInvalid, match="offset overflow"):
        amd.compute.replace_substring(arr, "a", "b" * r)


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_string_replace_grid(emu_ctx, n):
    _grid(emu_ctx, n)


@pytest.mark.emu
def test_string_replace_row_lengths(emu_ctx):
    _row_lengths(emu_ctx)


@pytest.mark.emu
def test_string_replace_long_literals(emu_ctx):
    _long_literals(emu_ctx)


@pytest.mark.emu
def test_string_replace_constructed_rows(emu_ctx):
    _constructed(emu_ctx)


@pytest.mark.emu
def test_string_replace_straddles(emu_ctx):
    _straddles(emu_ctx)


@pytest.mark.emu
def test_string_replace_auto_and_counters(emu_ctx):
    _auto_and_counters(emu_ctx)


@pytest.mark.emu
def test_string_replace_all_null_and_all_empty(emu_ctx):
    _all_null_and_all_empty(emu_ctx)


@pytest.mark.emu
def test_string_replace_mirror(emu_ctx):
    _mirror(emu_ctx)


@pytest.mark.emu
def test_string_replace_c_abi_large_offsets(emu_ctx):
    _large_offsets(emu_ctx)


@pytest.mark.emu
def test_string_replace_c_abi_null_row_spanning_bytes(emu_ctx):
    _null_row_spanning_bytes(emu_ctx)


@pytest.mark.emu
def test_string_replace_c_abi_contract(emu_ctx):
    _c_abi_contract(emu_ctx)


@pytest.mark.emu
def test_string_replace_overflow(emu_ctx):
    _overflow(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_gpu_string_replace_grid(gpu_ctx, n):
    _grid(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_string_replace_row_lengths_and_long_literals(gpu_ctx):
    _row_lengths(gpu_ctx)
    _long_literals(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_replace_constructed_rows_and_straddles(gpu_ctx):
    _constructed(gpu_ctx)
    _straddles(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_replace_auto_nulls_and_mirror(gpu_ctx):
    _auto_and_counters(gpu_ctx)
    _all_null_and_all_empty(gpu_ctx)
    _mirror(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_replace_c_abi(gpu_ctx):
    _large_offsets(gpu_ctx)
    _null_row_spanning_bytes(gpu_ctx)
    _c_abi_contract(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_replace_overflow(gpu_ctx):
    _overflow(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_replace_1e6_rows_from_numpy_buffers(gpu_ctx):
    rng = rng_for("1e6")
    n = 1_000_000
    lens = rng.integers(0, 41, n)                                  # mean row size 20
    lens[rng.integers(0, n, 20)] = 30_000                          # a few long rows among the short ones
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    data = rng.integers(97, 123, int(offsets[-1])).astype(np.uint8)
    pattern = b"@#"
    planted = np.flatnonzero((rng.random(n) < 0.36) & (lens >= len(pattern)))      # the pattern in about a third of the rows
    for _ in range(2):                                             # up to two a row; they may overlap or touch
        at = offsets[planted] + rng.integers(0, lens[planted] - len(pattern) + 1)
        for k, byte in enumerate(pattern):
            data[at + k] = byte
        planted = planted[rng.random(len(planted)) < 0.3]
    long_rows = np.flatnonzero(lens == 30_000)
    for row in long_rows:                                          # the long rows hold many
        at = offsets[row] + rng.integers(0, 30_000 - 2, 500)
        data[at], data[at + 1] = pattern[0], pattern[1]
    valid = np.packbits(rng.random(n) >= 0.05, bitorder="little")
    arr = pa.Array.from_buffers(pa.string(), n, [pa.py_buffer(valid.tobytes()), pa.py_buffer(offsets.astype(np.int32).tobytes()),
                                                 pa.py_buffer(data.tobytes())])
    share = pc.sum(pc.match_substring(arr, "@#")).as_py() / n
    assert 0.25 < share < 0.4, share
    check(gpu_ctx, arr.slice(13), gpu_ctx.Array.from_pyarrow(arr).slice(13), [("@#", "<<>>>", None), ("@#", "", 1), ("@#", "#@", -1)])
