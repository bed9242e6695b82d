"""match_substring / starts_with / ends_with (arrow_amd.compute, csrc/match_substring.hip) against pyarrow.compute on the
host copy of the same array: values, validity and null_count, exact equality, no tolerances.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus one column of 10^6 rows built from numpy buffers.  Both kernels are reached through
compute.MATCH_SUBSTRING_PATH (1 = one lane per row, 2 = the lanes walk the bytes); large offsets go through the C ABI,
since the mirror's Array does not carry them."""
import ctypes as C

import numpy as np
import pytest

from . import string_util
from .string_util import c_buffers, path_set

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

OPS = ("match_substring", "starts_with", "ends_with")
OP_CODE = {"match_substring": 0, "starts_with": 1, "ends_with": 2}
LENGTHS = [0, 1, 63, 64, 65, 4097, 100_000]
LDS_CAP = 1024          # kPatternLdsCap of csrc/match_substring.hip
TILE = 4096             # kTileBytes: 256 lanes x 16 bytes
SEED = 0x5B5
KNOB = "MATCH_SUBSTRING_PATH"              # the global of arrow_amd.compute that selects the kernel form


def rng_for(*key):
    return string_util.rng_for(SEED, *key)


def pattern_of(m):
    """A pattern of m bytes without a period, so that rows can hold it exactly once or twice."""
    return bytes((ord("a") + (i * 7 + i // 26) % 26) for i in range(m))


def row_pool(pat):
    m = len(pat)
    rows = [b"", pat, pat + b"z", b"z" + pat, pat + b"-tail of the row", b"the head of the row-" + pat,
            b"mid" + pat + b"dle", pat + b"--" + pat, b"zzzz", b"hello world", b"q" * 40, pat[: m // 2] * 2,
            pat[1:] + pat[:1], b"x\x00y"]
    if m:
        rows += [pat[:-1], pat[:-1] + b"!", b"!" + pat[1:]]
    return rows


def column(rng, pat, n, null_p, typ):
    pool = row_pool(pat)
    mask = (rng.random(n) < null_p) if null_p else None
    return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.binary(), mask=mask).cast(typ)


def check(amd, arr, pat, offset=0, ops=OPS, paths=(1, 2)):
    """Every op on both paths equals the reference (computed once per op) on arr.slice(offset)."""
    host = arr.slice(offset) if offset else arr
    dev = amd.Array.from_pyarrow(arr)
    dev = dev.slice(offset) if offset else dev
    for op in ops:
        want = getattr(pc, op)(host, pat)
        for path in paths:
            with path_set(amd, KNOB, path):
                got = getattr(amd.compute, op)(dev, pat)
            assert got.to_pyarrow().equals(want), (op, path, host.type, offset, len(host), pat[:20])
            assert got.null_count == want.null_count, (op, path)
            assert got.offset == 0


def _grid(amd, n):
    pat = b"abc"
    for typ in (pa.string(), pa.binary()):
        for null_p in (0.0, 0.1):
            arr = column(rng_for("grid", n, typ, null_p), pat, n + 13, null_p, typ)
            check(amd, arr, pat, offset=13)          # n rows, first offset non-zero, odd validity bit offset
            if n <= 4097:
                check(amd, arr.slice(0, n), pat)


def _pattern_lengths(amd, m):
    pat = pattern_of(m)
    n = 700                                           # three workgroups of rows
    for typ, null_p, off in ((pa.binary(), 0.1, 13), (pa.string(), 0.0, 0)):
        check(amd, column(rng_for("m", m, typ), pat, n, null_p, typ), pat, offset=off)


def _special_patterns(amd):
    rng = rng_for("special")
    nul = b"a\x00b"
    check(amd, column(rng, nul, 500, 0.1, pa.binary()), nul, offset=13)
    check(amd, column(rng, nul, 500, 0.0, pa.string()), nul.decode())
    long_pat = b"x" * 5000                            # longer than every row
    arr = column(rng, b"abc", 300, 0.1, pa.string())
    check(amd, arr, long_pat)
    assert not pc.match_substring(arr, long_pat).drop_null().to_pylist().count(True)
    check(amd, pa.array(["", None, ""], pa.string()), b"a")      # no referenced byte at all
    check(amd, pa.array(["", None, "abc"], pa.string()), b"")    # the empty pattern: every valid row


def rows_with_matches_at(starts, pat, total):
    """Rows of '.' whose concatenated bytes hold `pat` at each byte position of `starts` (one match per row)."""
    rows, pos = [], 0
    for s in starts:
        assert s >= pos
        rows.append(b"." * (s - pos) + pat + b"..")
        pos = s + len(pat) + 2
    rows.append(b"." * max(0, total - pos))
    return rows


def _bytes_path_cases(amd):
    # the pattern spans two adjacent rows: no match for either; then with empty rows and a null row in between
    check(amd, pa.array(["xxab", "cxx"], pa.string()), "abc")
    check(amd, pa.array(["xxab", "", None, "", "cxx", "abc"], pa.string()), "abc")
    # matches that straddle a lane's 16-byte boundary and a tile boundary (the buffers are 64-byte aligned, so byte
    # position = address modulo the tile), a 3-byte and a 20-byte pattern (the verify crosses the boundary too)
    for pat in (b"abc", pattern_of(20)):
        m = len(pat)
        starts = [16 - 2, 192 - (m - 1), TILE - 1, 2 * TILE - m + 1, 3 * TILE - m // 2, 3 * TILE + 16 * 255 + 15 - 1]
        rows = rows_with_matches_at(sorted(starts), pat, 5 * TILE)
        arr = pa.array(rows, pa.binary())
        assert pc.match_substring(arr, pat).to_pylist() == [True] * (len(rows) - 1) + [False]
        check(amd, arr, pat)
    # a match ending on the last referenced byte and one starting on the first; the neighbours outside the slice hold
    # bytes that would complete a match across the slice's ends
    arr = pa.array(["junkab", "abcxx", "yy", "zzabc", "abc"], pa.string())
    check(amd, arr.slice(1, 3), "abc")
    arr = pa.array(["xab", "cde", "fga", "bc"], pa.string())
    check(amd, arr.slice(1, 2), "abc")
    assert pc.match_substring(arr.slice(1, 2), "abc").to_pylist() == [False, False]
    # runs of empty rows resolve to the one non-empty row that owns the byte; more rows in one tile than offsets are staged
    check(amd, pa.array(([b""] * 2500 + [b"abc", b"", b"ab", b"", b"c"]) * 3 + [b"", b"xabc", b""], pa.binary()), b"abc")
    # every position a hit
    check(amd, pa.array([b"a" * k for k in list(range(0, 70)) + [5000, 1, 0, 33]], pa.binary()), b"a")
    check(amd, pa.array([b"a" * k for k in (100, 0, 4096, 17)], pa.binary()), b"a" * 9)


def _one_long_row(amd):
    rng = rng_for("long")
    pat = b"needle"
    rows = [bytes(r) for r in np.split(rng.integers(97, 101, 16 * 1000, dtype=np.uint8), 1000)]
    long_hit = bytes(rng.integers(97, 101, 200_000, dtype=np.uint8)) + pat
    long_miss = bytes(rng.integers(97, 101, 200_000, dtype=np.uint8))
    rows[500] = long_hit
    rows[123] = rows[123] + pat
    arr = pa.array(rows, pa.binary())
    check(amd, arr, pat, ops=("match_substring", "ends_with"))
    rows[500] = long_miss
    check(amd, pa.array(rows, pa.binary()), pat, ops=("match_substring",))


# ---------------------------------------------------------------- the C ABI directly
def c_match(amd, arr, owidth, op, pat, path, hint=None):
    """arx_match_substring on `arr`: the raw output bits as a bool array of len(arr)."""
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    span, keep, nbytes = c_buffers(arr, owidth)
    n = len(arr)
    dpat = to_device(np.frombuffer(pat, dtype=np.uint8) if pat else np.zeros(0, np.uint8))
    out = to_device(np.full(((n + 63) // 64) * 8 + 8, 0xEE, np.uint8))
    rc = lib.arx_match_substring(C.byref(span), owidth, OP_CODE[op], dpat.data_ptr(), len(pat), nbytes if hint is None else hint,
                                 path, out.data_ptr(), None)
    assert rc == 0, lib.arx_last_error()
    if out.is_cuda:
        torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[((n + 63) // 64) * 8:((n + 63) // 64) * 8 + 8] == 0xEE).all()      # nothing past the last word
    return np.unpackbits(raw, bitorder="little")[:n].astype(bool)


def _null_row_holding_the_pattern(amd):
    plain = pa.array(["xabcx", "abc", "q", "abc"], pa.string())
    valid = pa.py_buffer(bytes([0b1101]))
    arr = pa.Array.from_buffers(pa.string(), 4, [valid, plain.buffers()[1], plain.buffers()[2]])
    assert arr.to_pylist() == ["xabcx", None, "q", "abc"]
    check(amd, arr, "abc")
    for op in OPS:
        for path in (1, 2):
            bits = c_match(amd, arr, 4, op, b"abc", path)
            assert bits.tolist() == [op == "match_substring", False, False, True], (op, path)


def _large_offsets(amd):
    rng = rng_for("large")
    for pat in (b"abc", pattern_of(17), b""):
        small = column(rng, pat, 3000, 0.1, pa.string())
        for small_t, large_t in ((pa.string(), pa.large_string()), (pa.binary(), pa.large_binary())):
            a4 = small.cast(small_t).slice(5)
            a8 = small.cast(large_t).slice(5)
            for op in OPS:
                want = getattr(pc, op)(a8, pat)
                assert want.equals(getattr(pc, op)(a4, pat))
                want_bits = np.array(want.fill_null(False).to_pylist())
                for path in (1, 2):
                    assert (c_match(amd, a8, 8, op, pat, path) == want_bits).all(), (op, path, large_t)
                    assert (c_match(amd, a4, 4, op, pat, path) == want_bits).all(), (op, path, small_t)


def _invalid_arguments(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    arr = pa.array(["abc", "b"], pa.string())
    span, keep, nbytes = c_buffers(arr, 4)
    dpat = to_device(np.frombuffer(b"b", dtype=np.uint8))
    out = to_device(np.full(16, 0xEE, np.uint8))

    def call(sp=span, width=4, op=0, m=1, path=1, o=out):
        return lib.arx_match_substring(C.byref(sp) if sp is not None else None, width, op, dpat.data_ptr(), m, nbytes, path,
                                       o.data_ptr() if o is not None else None, None)

    for kwargs, text in (({"op": 3}, b"op 3"), ({"op": -1}, b"op -1"), ({"path": 3}, b"path 3"), ({"width": 2}, b"offset_width 2"),
                         ({"m": -1}, b"negative length"), ({"sp": None}, b"NULL values or out_bits"),
                         ({"o": None}, b"NULL values or out_bits")):
        assert call(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    neg = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, -1, 0)
    assert call(sp=neg) == _lib.ARX_INVALID and b"negative length" in lib.arx_last_error()
    # length 0 succeeds and writes nothing
    empty = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, 0, 0)
    rows0, bytes0 = lib.arx_get_counter(b"match_substring_row_launches"), lib.arx_get_counter(b"match_substring_byte_launches")
    for path in (0, 1, 2):
        assert call(sp=empty, path=path) == 0
    assert (out.cpu().numpy()[:16] == 0xEE).all()
    assert lib.arx_get_counter(b"match_substring_row_launches") == rows0
    assert lib.arx_get_counter(b"match_substring_byte_launches") == bytes0
    assert call() == 0


def _counters(amd):
    from arrow_amd import _lib

    lib = _lib.get_lib()
    count = lambda: (lib.arx_get_counter(b"match_substring_row_launches"), lib.arx_get_counter(b"match_substring_byte_launches"))  # noqa: E731
    rng = rng_for("counters")
    short = amd.Array.from_pyarrow(pa.array([bytes(r) for r in np.split(rng.integers(97, 100, 16 * 2000, dtype=np.uint8), 2000)]))
    wide = amd.Array.from_pyarrow(pa.array([bytes(r) for r in np.split(rng.integers(97, 100, 4096 * 64, dtype=np.uint8), 64)]))
    r0, b0 = count()
    with path_set(amd, KNOB, 1):
        for op in OPS:
            getattr(amd.compute, op)(short, "ab")
    assert count() == (r0 + 3, b0)
    with path_set(amd, KNOB, 2):              # starts_with / ends_with and the empty pattern always take rows
        for op in OPS:
            getattr(amd.compute, op)(short, "ab")
        amd.compute.match_substring(short, "")
    assert count() == (r0 + 6, b0 + 1)
    # auto: rows for a 16-byte-mean column, bytes for a 4 KiB-mean column
    with path_set(amd, KNOB, 0):
        got_short = amd.compute.match_substring(short, "abcab")
        assert count() == (r0 + 7, b0 + 1)
        got_wide = amd.compute.match_substring(wide, "abcabcab")
        assert count() == (r0 + 7, b0 + 2)
        amd.compute.starts_with(wide, "a")
        assert count() == (r0 + 8, b0 + 2)
    assert got_short.to_pyarrow().equals(pc.match_substring(short.to_pyarrow(), "abcab"))
    assert got_wide.to_pyarrow().equals(pc.match_substring(wide.to_pyarrow(), "abcabcab"))


def _mirror(amd):
    arr = pa.array(["héllo", "hello", None, "", "llo"], pa.string())
    d = amd.Array.from_pyarrow(arr)
    for op in OPS:
        for pat in ("llo", "é", ""):
            want = getattr(pc, op)(arr, pat)
            assert getattr(amd.compute, op)(d, pat).to_pyarrow().equals(want), (op, pat)
            assert getattr(amd.compute, op)(d, pat.encode("utf-8")).to_pyarrow().equals(want), (op, pat)
            got = amd.compute.call_function(op, [d], amd.compute.MatchSubstringOptions(pat))
            assert got.to_pyarrow().equals(want), (op, pat)
        with pytest.raises(amd.ArrowNotImplementedError, match="ignore_case"):
            getattr(amd.compute, op)(d, "llo", ignore_case=True)
        ints = pa.array([1, 2, 3])
        with pytest.raises(pa.ArrowNotImplementedError) as want_err:
            getattr(pc, op)(ints, "1")
        with pytest.raises(pa.ArrowNotImplementedError) as got_err:
            getattr(amd.compute, op)(amd.Array.from_pyarrow(ints), "1")
        assert str(got_err.value) == str(want_err.value)
        assert "has no kernel matching input types" in str(got_err.value)
    no_nulls = amd.compute.match_substring(amd.Array.from_pyarrow(pa.array(["a", "b"])), "a")
    assert no_nulls.validity is None and no_nulls.null_count == 0
    sliced = amd.compute.match_substring(d.slice(1), "llo")             # the null count of a slice is not known: lazy
    assert sliced.null_count == 1 and sliced.to_pylist() == [True, None, False, True]


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_match_substring_grid(emu_ctx, n):
    _grid(emu_ctx, n)


@pytest.mark.emu
@pytest.mark.parametrize("m", [0, 1, 7, 8, 9, 16, 17, 300, LDS_CAP, LDS_CAP + 1])
def test_match_substring_pattern_lengths(emu_ctx, m):
    _pattern_lengths(emu_ctx, m)


@pytest.mark.emu
def test_match_substring_nul_bytes_long_and_empty_patterns(emu_ctx):
    _special_patterns(emu_ctx)


@pytest.mark.emu
def test_match_substring_bytes_path_boundaries(emu_ctx):
    _bytes_path_cases(emu_ctx)


@pytest.mark.emu
def test_match_substring_one_long_row_among_short_ones(emu_ctx):
    _one_long_row(emu_ctx)


@pytest.mark.emu
def test_match_substring_null_row_holding_the_pattern(emu_ctx):
    _null_row_holding_the_pattern(emu_ctx)


@pytest.mark.emu
def test_match_substring_c_abi_large_offsets(emu_ctx):
    _large_offsets(emu_ctx)


@pytest.mark.emu
def test_match_substring_c_abi_invalid_arguments_and_length_zero(emu_ctx):
    _invalid_arguments(emu_ctx)


@pytest.mark.emu
def test_match_substring_counters_and_auto_path(emu_ctx):
    _counters(emu_ctx)


@pytest.mark.emu
def test_match_substring_mirror(emu_ctx):
    _mirror(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
def test_gpu_match_substring_grid(gpu_ctx):
    for n in LENGTHS:
        _grid(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_match_substring_patterns(gpu_ctx):
    for m in (0, 1, 7, 8, 9, 16, 17, 300, LDS_CAP, LDS_CAP + 1):
        _pattern_lengths(gpu_ctx, m)
    _special_patterns(gpu_ctx)


@pytest.mark.gpu
def test_gpu_match_substring_bytes_path_cases(gpu_ctx):
    _bytes_path_cases(gpu_ctx)
    _one_long_row(gpu_ctx)
    _null_row_holding_the_pattern(gpu_ctx)


@pytest.mark.gpu
def test_gpu_match_substring_c_abi(gpu_ctx):
    _large_offsets(gpu_ctx)
    _invalid_arguments(gpu_ctx)


@pytest.mark.gpu
def test_gpu_match_substring_counters_and_mirror(gpu_ctx):
    _counters(gpu_ctx)
    _mirror(gpu_ctx)


@pytest.mark.gpu
def test_gpu_match_substring_1e6_rows_from_numpy_buffers(gpu_ctx):
    rng = rng_for("1e6")
    n = 1_000_000
    lengths = rng.integers(0, 33, n)
    lengths[rng.integers(0, n, 20)] = 50_000                      # a few long rows among the short ones
    offsets = np.zeros(n + 1, np.int32)
    np.cumsum(lengths, out=offsets[1:])
    data = rng.integers(97, 100, int(offsets[-1]), dtype=np.uint8)   # 'a' .. 'c': "abca" is frequent, 12 bytes of it rare
    valid = np.packbits(rng.random(n) >= 0.05, bitorder="little")
    arr = pa.Array.from_buffers(pa.binary(), n, [pa.py_buffer(valid.tobytes()), pa.py_buffer(offsets.tobytes()),
                                                 pa.py_buffer(data.tobytes())])
    check(gpu_ctx, arr, b"abca", offset=13)
    check(gpu_ctx, arr, b"abcabcabcabc", ops=("match_substring",))
