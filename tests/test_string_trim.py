"""The twelve trim functions {ascii,utf8}_{,l,r}trim{,_whitespace} (arrow_amd.compute, csrc/string_trim.hip) against
pyarrow.compute on the host copy of the same array: values, validity, null_count and offset 0, exact equality.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus one column of 10^6 rows built from numpy buffers.  Large offsets and invalid UTF-8 go through the C ABI,
since the mirror's Array carries neither.

One known departure from the reference: where its walk meets an invalid UTF-8 sequence it raises "Invalid UTF8 sequence in
input"; the device stops trimming there and returns the row.  Those rows are checked against rule_trim below, the unit
rule of csrc/string_trim.hip restated, and test_reference_trim_of_invalid_utf8_still_raises notices a pyarrow that no
longer raises."""
import ctypes as C

import numpy as np
import pytest

from . import string_util
from .string_util import c_buffers, same, sync

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

LENGTHS = [0, 1, 63, 64, 65, 4097]
LEFT, RIGHT, BOTH = 1, 2, 3
ASCII_WS, UTF8_WS, BYTE_SET, CODEPOINT_SET = 0, 1, 2, 3
SIDES = {"trim": BOTH, "ltrim": LEFT, "rtrim": RIGHT}
WHITESPACE_TRIMS = [f"{enc}_{side}_whitespace" for enc in ("ascii", "utf8") for side in SIDES]
CHARACTER_TRIMS = [f"{enc}_{side}" for enc in ("ascii", "utf8") for side in SIDES]
COUNTER = b"string_trim_launches"
RUNS = (0, 1, 15, 16, 17, 33)
MIXED = "xé 　😀"                                             # 1-, 2-, 1-, 3- and 4-byte characters
WS = {9, 10, 11, 12, 13, 0x1C, 0x1D, 0x1E, 0x1F, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F,
      0x3000}
ASCII_WS_BYTES = {9, 10, 11, 12, 13, 32}
SEED = 0x7219


def rng_for(*key):
    return string_util.rng_for(SEED, *key)


# ---------------------------------------------------------------- the unit rule of csrc/string_trim.hip
def cont(x):
    return (x & 0xC0) == 0x80


def value(u):
    """The value of a unit: only when its length is the one its lead declares and the value is not below that length's
    minimum."""
    n = 1 if u[0] < 0x80 else 2 if u[0] >> 5 == 6 else 3 if u[0] >> 4 == 14 else 4 if u[0] >> 3 == 30 else 0
    if n == 0 or n != len(u):
        return None
    v = u[0] if n == 1 else u[0] & (0xFF >> (n + 1))
    for x in u[1:]:
        v = (v << 6) | (x & 0x3F)
    return v if v >= (0, 0, 0x80, 0x800, 0x10000)[n] else None


def front_unit(b, p, e):
    if cont(b[p]):
        return p + 1, None
    q = p + 1
    while q < e and q - p < 4 and cont(b[q]):
        q += 1
    return q, value(b[p:q])


def back_unit(b, p, e):
    q, k = e - 1, 0
    while q > p and k < 3 and cont(b[q]):
        q, k = q - 1, k + 1
    if cont(b[q]):
        return e - 1, None
    return q, value(b[q:e])


def rule_trim(b, inset, sides):
    """Trimming advances over a unit only if it has a value and that value is in the set; left first, then right."""
    p, e = 0, len(b)
    while sides & LEFT and p < e:
        q, v = front_unit(b, p, e)
        if v is None or not inset(v):
            break
        p = q
    while sides & RIGHT and e > p:
        q, v = back_unit(b, p, e)
        if v is None or not inset(v):
            break
        e = q
    return b[p:e]


def byte_trim(b, members, sides):
    p, e = 0, len(b)
    while sides & LEFT and p < e and b[p] in members:
        p += 1
    while sides & RIGHT and e > p and b[e - 1] in members:
        e -= 1
    return b[p:e]


# ---------------------------------------------------------------- rows
def row_pool():
    ws = " \t\n\r\x0b\x0c"
    rows = ["", "x", "abc", "héllo wörld", "a b", "\x00", "\x7f", " \x00 ", "\x7f ", "xax", "éaé", "😀a😀", "　a　", "xé 　😀z😀　 éx"]
    for k in RUNS:                                           # trimmable runs at either end, or at both
        run = (ws * 6)[:k]
        rows += [run + "payload", "payload" + run, run + "p" + run, " " * k + "é日😀" + " " * k, "x" * k + "q" + "x" * k]
    rows += [(ws * 900)[:k] for k in (1, 16, 17, 5000)]     # all-trimmable rows (and "" above)
    rows += ["　" * 6, " \u0085　a　\u0085 ", "      ", "\x1c\x1d\x1e\x1f|\x1f\x1e"]
    rows += ["\u200bx\u200b", "\u180e a \u180e", " \u0084a\u0084 ", "\u0086", "\u2027 a \u2027", " \u200b ", "\u3000\u3001\u3000"]   # near misses
    return rows


def column(rng, n, null_p, pool=None):
    pool = pool or row_pool()
    mask = (rng.random(n) < null_p) if null_p else None
    return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask)


def calls(characters=(MIXED,)):
    """(function, arguments): the six whitespace trims, and the six trims under every `characters`."""
    return [(name, ()) for name in WHITESPACE_TRIMS] + [(name, (c,)) for name in CHARACTER_TRIMS for c in characters]


def check(amd, host, dev, todo):
    for name, args in todo:
        want = getattr(pc, name)(host, *args)
        got = getattr(amd.compute, name)(dev, *args)
        same(got, want, host, (name, args, len(host)))


def _grid(amd, n):
    """Both null shares, whole and as slice(7) of n + 7 rows, all twelve functions."""
    for null_p in (0.0, 0.1):
        arr = column(rng_for("grid", n, null_p), n + 7, null_p)
        dev = amd.Array.from_pyarrow(arr)
        check(amd, arr.slice(7), dev.slice(7), calls())      # n rows, first offset non-zero, odd validity bit offset
        check(amd, arr.slice(0, n), dev.slice(0, n), calls())


def _granule_edges(amd):
    """Payloads that begin and end on each of the 16 byte positions of a granule, behind and before runs of every length:
    the fillers sweep every alignment, whatever the buffer's own."""
    rows = []
    for pad in range(17):
        for k in RUNS:
            rows += ["#" * pad, " " * k + "payload" + "\t" * k, "　" * (k // 3) + "é" + " " * (k // 3), "x" * k + "日" + "x" * (k + 1)]
    for k in range(17):                                      # multi-byte whitespace across a granule boundary
        rows += ["#" * k, "　 \u0085pay\u0085 　", "#" * k + "　", "\u0085" * 9 + "z" + " " * 6]
    arr = pa.array(rows, pa.string())
    offsets = np.frombuffer(arr.buffers()[1], np.int32)[: len(rows) + 1]
    lens = np.array(pc.binary_length(pc.ascii_ltrim_whitespace(arr)).to_pylist())
    begins = offsets[1:] - lens                              # where the payload of a left-trimmed row begins
    ends = offsets[:-1] + np.array(pc.binary_length(pc.ascii_rtrim_whitespace(arr)).to_pylist())
    assert set(begins % 16) == set(range(16)) and set(ends % 16) == set(range(16))
    check(amd, arr, amd.Array.from_pyarrow(arr), calls())


def _characters(amd):
    arr = column(rng_for("characters"), 300, 0.1)
    dev = amd.Array.from_pyarrow(arr)
    check(amd, arr, dev, calls(("", "x", "xx", MIXED, " \t", "　😀")))
    many = "".join(chr(c) for c in list(range(0x20, 0x40)) + list(range(0xE0, 0xF0)) + list(range(0x3000, 0x3010)) + [0x1F600])
    assert len(set(many)) == 65
    check(amd, arr, dev, [(name, (many[:64],)) for name in CHARACTER_TRIMS])           # exactly 64 distinct codepoints
    check(amd, arr, dev, [(name, (many[:64] + many[:5],)) for name in CHARACTER_TRIMS])   # duplicates do not count
    for name in CHARACTER_TRIMS:
        if name.startswith("utf8"):
            with pytest.raises(amd.ArrowNotImplementedError, match=f"{name} with 65 distinct"):
                getattr(amd.compute, name)(dev, many)
        else:
            check(amd, arr, dev, [(name, (many,))])          # a byte set has no such bound
    assert amd.compute.ascii_trim(amd.Array.from_pyarrow(pa.array(["éaé"])), "xÃ").to_pyarrow().cast(pa.binary()).to_pylist() \
        == [b"\xa9a\xc3\xa9"]
    for bad in (b"\xff", b"\xc3", b"\xe2\x80"):
        with pytest.raises(pa.ArrowInvalid) as want_err:
            pc.utf8_trim(arr, bad)
        with pytest.raises(amd.ArrowInvalid) as got_err:
            amd.compute.utf8_trim(dev, bad)
        assert str(got_err.value) == str(want_err.value) == "Invalid UTF8 sequence in input"


def _null_row_spanning_bytes(amd):
    plain = pa.array(["  ab  ", "   ", " q", "abc "], pa.string())
    arr = pa.Array.from_buffers(pa.string(), 4, [pa.py_buffer(bytes([0b1101])), plain.buffers()[1], plain.buffers()[2]])
    assert arr.to_pylist()[1] is None
    check(amd, arr, amd.Array.from_pyarrow(arr), calls())
    for kind in (ASCII_WS, UTF8_WS):
        rows, offsets = c_trim(amd, arr, 4, BOTH, kind)
        assert offsets.tolist() == [0, 2, 2, 3, 6] and rows == [b"ab", b"", b"q", b"abc"]      # no byte of the null row


def _all_null_and_all_empty(amd):
    spaces = pa.array(["  ", " ", "   "])
    for arr in (pa.array([None] * 70, pa.string()), pa.array([""] * 70, pa.string()), pa.array(["  \t"] * 70, pa.string()),
                pa.Array.from_buffers(pa.string(), 3, [pa.py_buffer(bytes([0])), spaces.buffers()[1], spaces.buffers()[2]])):
        check(amd, arr, amd.Array.from_pyarrow(arr), calls())
        rows, offsets = c_trim(amd, arr, 4, BOTH, UTF8_WS)
        assert int(offsets[-1]) == 0 and not any(rows)


def _mirror(amd):
    s = pa.array([" héllo ", None, "", "x日本x"], pa.string())
    ds = amd.Array.from_pyarrow(s)
    cp = amd.compute
    same(cp.call_function("utf8_trim_whitespace", [ds]), pc.utf8_trim_whitespace(s), s, "utf8_trim_whitespace")
    same(cp.call_function("ascii_rtrim", [ds], cp.TrimOptions(" ")), pc.ascii_rtrim(s, " "), s, "ascii_rtrim")
    same(cp.call_function("utf8_ltrim", [ds], cp.TrimOptions(characters="x ")), pc.utf8_ltrim(s, "x "), s, "utf8_ltrim")
    sliced = cp.utf8_trim(ds.slice(1), "x")                  # the null count of a slice is not known: lazy
    assert sliced.null_count == 1 and sliced.to_pyarrow().to_pylist() == [None, "", "日本"]
    with pytest.raises(amd.ArrowInvalid, match="Function 'ascii_trim' cannot be called without options"):
        cp.call_function("ascii_trim", [ds])
    with pytest.raises(amd.ArrowNotImplementedError, match="utf8_trim_whitespace of a scalar"):
        cp.call_function("utf8_trim_whitespace", [amd.Scalar(" a ", ds.type, True)])
    b, ints = s.cast(pa.binary()), pa.array([1, 2, 3])
    for name, args in calls(("x",)):
        for host in (b, ints):
            with pytest.raises(pa.ArrowNotImplementedError) as want_err:
                getattr(pc, name)(host, *args)
            with pytest.raises(pa.ArrowNotImplementedError) as got_err:
                getattr(cp, name)(amd.Array.from_pyarrow(host), *args)
            assert str(got_err.value) == str(want_err.value)
            assert "has no kernel matching input types" in str(got_err.value)


# ---------------------------------------------------------------- the C ABI directly
def host_set(kind, members):
    """(the host `set` of arx_string_trim_offsets, its length, what keeps it alive)"""
    if kind == BYTE_SET:
        buf = (C.c_uint8 * max(len(members), 1))(*members)
    elif kind == CODEPOINT_SET:
        buf = (C.c_uint32 * max(len(members), 1))(*members)
    else:
        return None, 0, None
    return C.cast(buf, C.c_void_p), len(members), buf


def c_trim(amd, arr, owidth, sides, kind, members=()):
    """arx_string_trim_offsets + arx_string_slice_data on `arr`: (the output rows as bytes, the output offsets); the 0xEE
    guard words after the offsets and after the data survive."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    span, keep, nbytes = c_buffers(arr, owidth)
    n = len(arr)
    ws_bytes = lib.arx_string_slice_workspace_bytes(n, owidth)
    ws = to_device(np.zeros(ws_bytes, np.uint8))
    out_offsets = to_device(np.full((n + 1) * owidth + 8, 0xEE, np.uint8))
    total = C.c_int64(-1)
    set_ptr, set_length, alive = host_set(kind, members)
    rc = lib.arx_string_trim_offsets(C.byref(span), owidth, sides, kind, set_ptr, set_length, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(),
                                     C.byref(total), None)
    assert rc == 0, lib.arx_last_error()
    out_data = to_device(np.full(total.value + 8, 0xEE, np.uint8))
    rc = lib.arx_string_slice_data(C.byref(span), owidth, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), total.value,
                                   out_data.data_ptr(), None)
    assert rc == 0, lib.arx_last_error()
    sync(out_data)
    raw_o, raw_d = out_offsets.cpu().numpy(), out_data.cpu().numpy()
    assert (raw_o[(n + 1) * owidth: (n + 1) * owidth + 8] == 0xEE).all()
    assert (raw_d[total.value: total.value + 8] == 0xEE).all()
    offsets = raw_o[: (n + 1) * owidth].view(np.int32 if owidth == 4 else np.int64).copy()
    assert offsets[0] == 0 and offsets[-1] == total.value and (np.diff(offsets) >= 0).all()
    return [raw_d[offsets[i]: offsets[i + 1]].tobytes() for i in range(n)], offsets


def c_cases():
    """(name, arguments, sides, set kind, the set's members) of all twelve functions under MIXED."""
    out = []
    for side, sides in SIDES.items():
        out += [(f"ascii_{side}_whitespace", (), sides, ASCII_WS, ()), (f"utf8_{side}_whitespace", (), sides, UTF8_WS, ()),
                (f"ascii_{side}", (MIXED,), sides, BYTE_SET, tuple(MIXED.encode())),
                (f"utf8_{side}", (MIXED,), sides, CODEPOINT_SET, tuple(ord(c) for c in MIXED))]
    return out


def _large_offsets(amd):
    small = column(rng_for("large"), 1000, 0.1)
    a4, a8 = small.slice(5), small.cast(pa.large_string()).slice(5)
    for name, args, sides, kind, members in c_cases():
        want = [b"" if r is None else r for r in getattr(pc, name)(a4, *args).cast(pa.binary()).to_pylist()]
        rows8, off8 = c_trim(amd, a8, 8, sides, kind, members)
        rows4, off4 = c_trim(amd, a4, 4, sides, kind, members)
        assert rows8 == want and rows4 == want, name
        assert off8.dtype == np.int64 and off4.dtype == np.int32 and (off8 == off4).all()


def _invalid_utf8(amd):
    rows = [b" \xff a ", b"\xe2\x80", b"\x80 a \x80", b" \xc0\xa0x", b"\xf0\x9f\x98", b"  \x80\x80\x80\x80", b" \xe3\x80\x80 \xe3\x80",
            b"\xe3\x80\x80\x80 ", b"x\xc3\xa9\xa9x", b"\xc3", b"", b" ok\xc3\xa9 "]
    arr = pa.array(rows + rows[::-1], pa.binary())
    rows = arr.to_pylist()
    members = {ord(c) for c in MIXED}
    for sides in (LEFT, RIGHT, BOTH):
        for kind, inset, given in ((UTF8_WS, WS.__contains__, ()), (CODEPOINT_SET, members.__contains__, tuple(members))):
            got, offsets = c_trim(amd, arr, 4, sides, kind, given)
            assert got == [rule_trim(b, inset, sides) for b in rows], (sides, kind)
            assert all(g in b for g, b in zip(got, rows))                  # every output row is a sub-range of its row
        for kind, bytes_in, given in ((ASCII_WS, ASCII_WS_BYTES, ()), (BYTE_SET, {0x80, 0x20, 0xFF}, (0x80, 0x20, 0xFF, 0x80))):
            got, offsets = c_trim(amd, arr, 4, sides, kind, given)
            assert got == [byte_trim(b, bytes_in, sides) for b in rows], (sides, kind)
    # on valid UTF-8 the rule is the reference
    valid = column(rng_for("rule"), 400, 0.0)
    for name, args, sides, kind, given in c_cases():
        if kind in (UTF8_WS, CODEPOINT_SET):
            inset = WS.__contains__ if kind == UTF8_WS else set(given).__contains__
            assert [rule_trim(s.encode(), inset, sides).decode() for s in valid.to_pylist()] == getattr(pc, name)(valid, *args).to_pylist(), name


def _c_abi_contract(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    arr = pa.array([" héllo ", "b "], pa.string())
    span, keep, nbytes = c_buffers(arr, 4)
    ws_bytes = lib.arx_string_slice_workspace_bytes(2, 4)
    ws = to_device(np.zeros(ws_bytes + 8, np.uint8))
    out = to_device(np.full(64, 0xEE, np.uint8))
    total = C.c_int64(-1)
    x = (C.c_uint8 * 1)(ord("x"))
    many = (C.c_uint32 * 65)(*range(0x100, 0x141))

    def offsets(sp=span, width=4, sides=BOTH, kind=ASCII_WS, members=None, count=0, w=ws.data_ptr(), wb=ws_bytes, o=out, t=total):
        return lib.arx_string_trim_offsets(C.byref(sp) if sp is not None else None, width, sides, kind,
                                           C.cast(members, C.c_void_p) if members is not None else None, count, w, wb,
                                           o.data_ptr() if o is not None else None, C.byref(t) if t is not None else None, None)

    neg = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, -1, 0)
    no_offsets = _lib.ArxBinarySpan(None, None, keep[2].data_ptr(), 0, 2, 0)
    cases = [({"sides": 0}, b"sides 0"), ({"sides": 4}, b"sides 4"), ({"kind": -1}, b"set_kind -1"), ({"kind": 4}, b"set_kind 4"),
             ({"width": 2}, b"offset_width 2"), ({"width": 16}, b"offset_width 16"), ({"sp": neg}, b"negative length"),
             ({"sp": None}, b"NULL values, out_offsets or out_total_bytes"), ({"o": None}, b"NULL values, out_offsets or out_total_bytes"),
             ({"t": None}, b"NULL values, out_offsets or out_total_bytes"), ({"sp": no_offsets}, b"NULL offsets"),
             ({"wb": ws_bytes - 1}, b"ws of"), ({"w": None}, b"ws of"), ({"w": ws.data_ptr() + 4}, b"ws of"),
             ({"kind": BYTE_SET, "members": x, "count": -1}, b"negative set_length"),
             ({"kind": CODEPOINT_SET, "members": None, "count": 1}, b"NULL set"), ({"kind": BYTE_SET, "members": None, "count": 3}, b"NULL set")]
    before = lib.arx_get_counter(COUNTER)
    for kwargs, text in cases:
        assert offsets(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    assert offsets(kind=CODEPOINT_SET, members=many, count=65) == _lib.ARX_NOT_IMPLEMENTED
    assert b"64 distinct codepoints" in lib.arx_last_error()
    sync(out)
    assert (out.cpu().numpy()[:64] == 0xEE).all() and total.value == -1      # a refused call writes nothing
    # length 0: success, nothing launched, nothing written but out_offsets[0] and the total
    empty = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, 0, 0)
    for width in (4, 8):
        total.value = -1
        assert offsets(sp=empty, width=width, kind=UTF8_WS, w=None, wb=0) == 0 and total.value == 0
        sync(out)
        raw = out.cpu().numpy()
        assert (raw[:width] == 0).all() and (raw[width:64] == 0xEE).all()
        out[:64] = 0xEE
    assert lib.arx_get_counter(COUNTER) == before
    # one launch a call with length > 0, whatever the sides and the set; a NULL set of length 0 trims nothing
    for i, (kwargs, want) in enumerate([({}, [0, 6, 7]), ({"sides": LEFT, "kind": UTF8_WS}, [0, 7, 9]),
                                        ({"kind": BYTE_SET, "members": None, "count": 0}, [0, 8, 10]),
                                        ({"sides": RIGHT, "kind": CODEPOINT_SET, "members": many, "count": 64}, [0, 8, 10])]):
        assert offsets(**kwargs) == 0, lib.arx_last_error()
        assert lib.arx_get_counter(COUNTER) == before + i + 1
        sync(out)
        raw = out.cpu().numpy()
        assert raw[:12].view(np.int32).tolist() == want and total.value == want[-1] and (raw[12:64] == 0xEE).all(), kwargs


def test_reference_trim_of_invalid_utf8_still_raises():
    arr = pa.array([b" \xff"], pa.binary()).cast(pa.string(), safe=False)
    with pytest.raises(pa.ArrowInvalid, match="Invalid UTF8 sequence in input"):
        pc.utf8_trim_whitespace(arr)
    assert pc.ascii_trim_whitespace(arr).cast(pa.binary()).to_pylist() == [b"\xff"]


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_string_trim_grid(emu_ctx, n):
    _grid(emu_ctx, n)


@pytest.mark.emu
def test_string_trim_granule_edges(emu_ctx):
    _granule_edges(emu_ctx)


@pytest.mark.emu
def test_string_trim_characters(emu_ctx):
    _characters(emu_ctx)


@pytest.mark.emu
def test_string_trim_null_row_spanning_bytes(emu_ctx):
    _null_row_spanning_bytes(emu_ctx)


@pytest.mark.emu
def test_string_trim_all_null_and_all_empty(emu_ctx):
    _all_null_and_all_empty(emu_ctx)


@pytest.mark.emu
def test_string_trim_mirror(emu_ctx):
    _mirror(emu_ctx)


@pytest.mark.emu
def test_string_trim_c_abi_large_offsets(emu_ctx):
    _large_offsets(emu_ctx)


@pytest.mark.emu
def test_string_trim_c_abi_invalid_utf8(emu_ctx):
    _invalid_utf8(emu_ctx)


@pytest.mark.emu
def test_string_trim_c_abi_contract(emu_ctx):
    _c_abi_contract(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_gpu_string_trim_grid(gpu_ctx, n):
    _grid(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_string_trim_granule_edges_and_characters(gpu_ctx):
    _granule_edges(gpu_ctx)
    _characters(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_trim_null_rows_and_mirror(gpu_ctx):
    _null_row_spanning_bytes(gpu_ctx)
    _all_null_and_all_empty(gpu_ctx)
    _mirror(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_trim_c_abi(gpu_ctx):
    _large_offsets(gpu_ctx)
    _invalid_utf8(gpu_ctx)
    _c_abi_contract(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_trim_1e6_rows_from_numpy_buffers(gpu_ctx):
    rng = rng_for("1e6")
    n = 1_000_000
    lens = rng.integers(0, 33, n)                                  # mean row size 16
    lens[rng.integers(0, n, 20)] = 30_000                          # a few long rows among the short ones
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    data = rng.integers(97, 123, int(offsets[-1])).astype(np.uint8)
    row_of = np.repeat(np.arange(n), lens)
    at = np.arange(len(data)) - offsets[row_of]                    # a byte's position in its row, and from its row's end
    from_end = lens[row_of] - 1 - at
    lead, tail = rng.integers(0, 6, n), rng.integers(0, 6, n)      # runs of spaces / tabs / x at either end
    pad = np.array([32, 9, 120], np.uint8)[rng.integers(0, 3, len(data))]
    inside = (at < lead[row_of]) | (from_end < tail[row_of])
    data[inside] = pad[inside]
    all_ws = rng.random(n) < 0.02                                  # all-whitespace rows, the long ones among them
    data[all_ws[row_of]] = 32
    valid = np.packbits(rng.random(n) >= 0.05, bitorder="little")
    arr = pa.Array.from_buffers(pa.string(), n, [pa.py_buffer(valid.tobytes()), pa.py_buffer(offsets.astype(np.int32).tobytes()),
                                                 pa.py_buffer(data.tobytes())])
    check(gpu_ctx, arr.slice(13), gpu_ctx.Array.from_pyarrow(arr).slice(13), calls(("x \t",)))
