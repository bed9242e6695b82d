"""binary_length / utf8_length / binary_slice / utf8_slice_codeunits (arrow_amd.compute, csrc/string_slice.hip) against
pyarrow.compute on the host copy of the same array: values, validity, null_count and offset 0, exact equality.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus one column of 10^6 rows built from numpy buffers.  Both forms of the codepoint walk are reached through
compute.STRING_SLICE_PATH (1 = one lane per row, 2 = one wave per row); large offsets and invalid UTF-8 go through the C
ABI, since the mirror's Array carries neither.

One known departure from the reference: pc.binary_slice(arr, start >= 0, stop=None) overflows its size estimate
("Negative buffer resize") from two rows on; those cases are checked against Python's b[start:] instead, and
test_reference_binary_slice_without_stop_still_raises notices a pyarrow that no longer does."""
import ctypes as C

import numpy as np
import pytest

from . import string_util
from .string_util import c_buffers, path_set, same, sync

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

LENGTHS = [0, 1, 63, 64, 65, 4097]
STARTS = [0, 1, 2, 5, 100, -1, -3, -100]
STOPS = [None, 0, 1, 3, 100, -1, -2, -100]
BYTES, CODEPOINTS = 0, 1
NO_STOP = 2**63 - 1
ROW_COUNTER, WAVE_COUNTER = b"string_slice_row_launches", b"string_slice_wave_launches"
SEED = 0x51CE
KNOB = "STRING_SLICE_PATH"              # the global of arrow_amd.compute that selects the kernel form


def rng_for(*key):
    return string_util.rng_for(SEED, *key)


def row_pool():
    rows = ["x" * k for k in (0, 1, 15, 16, 17, 31, 32, 33, 255)]
    rows += ["é" * 9, "ü" * 8, "日" * 6, "本語" * 5, "😀" * 4, "😀🙂" * 5]                 # 2-, 3- and 4-byte characters
    rows += ["héllo wörld", "日本語テキスト", "aé日😀" * 3, "a" * 14 + "é" + "z" * 3, "ab" * 7 + "日" + "c", "q" * 13 + "😀" + "r" * 20]
    return rows


def column(rng, n, null_p, typ, pool=None):
    pool = pool or row_pool()
    mask = (rng.random(n) < null_p) if null_p else None
    return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask).cast(typ)


def want_slice(host, start, stop):
    """The reference's slice of `host`; Python's b[start:] where the reference overflows (module docstring)."""
    if pa.types.is_binary(host.type) and stop is None and start >= 0:
        return pa.array([None if b is None else b[start:] for b in host.to_pylist()], host.type)
    fn = pc.binary_slice if pa.types.is_binary(host.type) else pc.utf8_slice_codeunits
    return fn(host, start, stop)


def check_lengths(amd, host, dev, paths=(1, 2)):
    same(amd.compute.binary_length(dev), pc.binary_length(host), host, ("binary_length", host.type, len(host)))
    if pa.types.is_string(host.type):
        want = pc.utf8_length(host)
        for path in paths:
            with path_set(amd, KNOB, path):
                same(amd.compute.utf8_length(dev), want, host, ("utf8_length", path, len(host)))


def check_slices(amd, host, dev, bounds, paths=(1, 2)):
    utf8 = pa.types.is_string(host.type)
    for start, stop in bounds:
        want = want_slice(host, start, stop)
        for path in (paths if utf8 else (0,)):
            with path_set(amd, KNOB, path):
                got = (amd.compute.utf8_slice_codeunits if utf8 else amd.compute.binary_slice)(dev, start, stop)
            same(got, want, host, (host.type, start, stop, path, len(host)))


def variants(amd, n):
    """(host, device) for both types, both null shares, whole and as slice(13) of n + 13 rows."""
    for typ in (pa.string(), pa.binary()):
        for null_p in (0.0, 0.1):
            arr = column(rng_for("grid", n, typ, null_p), n + 13, null_p, typ)
            dev = amd.Array.from_pyarrow(arr)
            yield arr.slice(13), dev.slice(13)          # n rows, first offset non-zero, odd validity bit offset
            yield arr.slice(0, n), dev.slice(0, n)


def _grid_lengths(amd, n):
    for host, dev in variants(amd, n):
        check_lengths(amd, host, dev)


def _grid_slices(amd, n, starts=STARTS, stops=STOPS):
    for host, dev in variants(amd, n):
        check_slices(amd, host, dev, [(a, b) for a in starts for b in stops])


def _python_slicing(amd):
    """Bounds of either sign, empty and inverted ranges: Python's s[start:stop], and the reference's answer too."""
    rows = ["héllo wörld", "日本語テキスト", "", "a", "x" * 40]
    arr = pa.array(rows, pa.string())
    dev = amd.Array.from_pyarrow(arr)
    for start, stop in ((0, 2), (1, None), (-3, None), (-3, -1), (2, 1), (-100, 3), (3, 100), (0, 0), (-1, -3), (5, -2)):
        for path in (1, 2):
            with path_set(amd, KNOB, path):
                got = amd.compute.utf8_slice_codeunits(dev, start, stop).to_pylist()
            assert got == [s[start:stop] for s in rows], (start, stop, path)
        assert pc.utf8_slice_codeunits(arr, start, stop).to_pylist() == [s[start:stop] for s in rows]


def _straddles(amd):
    """A multi-byte character across a 16-byte granule boundary and across the 64 x 16 bytes a wave takes a step: the pad
    sweeps every alignment, whatever the buffer's own."""
    rows = []
    for k in range(17):
        rows += ["a" * k + "é" + "z", "a" * k + "😀日" + "z" * 20, "a" * (1008 + k) + "日" + "z" * 5, "é" * 505 + "a" * k + "😀" * 3]
    arr = pa.array(rows, pa.string())
    dev = amd.Array.from_pyarrow(arr)
    check_lengths(amd, arr, dev)
    bounds = [(k, k + 2) for k in range(0, 19)] + [(-3, None), (-7, -1), (1007, 1030), (500, 520), (-30, -1), (1, -1)]
    check_slices(amd, arr, dev, bounds)


def long_rows_column(typ=None):
    rng = rng_for("long")
    pool = ["abcdefghijklmnop", "é" * 8, "日本語テキ" + "x", "😀" * 4]
    rows = [pool[i] for i in rng.integers(0, len(pool), 300)]
    rows[41] = ("aé日😀" * 500)[:2000]                       # 5000 bytes
    rows[200] = "héllo wörld, 日本語テキスト! ab" * 5000         # 200 000 bytes
    assert len(rows[41].encode()) == 5000 and len(rows[200].encode()) == 200_000
    mask = np.zeros(300, bool)
    mask[[7, 150]] = True
    return pa.array(rows, pa.string(), mask=mask).cast(typ or pa.string())


def _long_rows(amd):
    for typ in (pa.string(), pa.binary()):
        arr = long_rows_column(typ)
        dev = amd.Array.from_pyarrow(arr)
        check_lengths(amd, arr, dev, paths=(0, 1, 2))
        bounds = [(0, 2), (1, None), (-3, None), (5, -2), (100, 3000), (3000, 150_000), (-150_000, -10), (-4000, 4500), (64, 65)]
        check_slices(amd, arr.slice(13), dev.slice(13), bounds, paths=(0, 1, 2))


def _null_row_spanning_bytes(amd):
    plain = pa.array(["xabcx", "abc", "q", "abc"], pa.string())
    valid = pa.py_buffer(bytes([0b1101]))
    for typ in (pa.string(), pa.binary()):
        arr = pa.Array.from_buffers(typ, 4, [valid, plain.buffers()[1], plain.buffers()[2]])
        assert arr.to_pylist()[1] is None
        dev = amd.Array.from_pyarrow(arr)
        check_lengths(amd, arr, dev)
        check_slices(amd, arr, dev, [(0, None), (0, 2), (-2, None), (1, -1)])
        unit = CODEPOINTS if typ == pa.string() else BYTES
        for path in (1, 2):
            assert c_length(amd, arr, 4, unit, path).tolist() == [5, 0, 1, 3]
            rows, offsets = c_slice(amd, arr, 4, unit, 0, NO_STOP, path)
            assert offsets.tolist() == [0, 5, 5, 6, 9] and rows == [b"xabcx", b"", b"q", b"abc"]      # no byte of the null row


def _all_null_and_all_empty(amd):
    for typ in (pa.string(), pa.binary()):
        for arr in (pa.array([None] * 70, typ), pa.array(["" if typ == pa.string() else b""] * 70, typ),
                    pa.Array.from_buffers(typ, 3, [pa.py_buffer(bytes([0])), pa.array(["ab", "c", "def"]).buffers()[1],
                                                   pa.array(["ab", "c", "def"]).buffers()[2]])):
            dev = amd.Array.from_pyarrow(arr)
            check_lengths(amd, arr, dev)
            check_slices(amd, arr, dev, [(0, None), (0, 2), (-1, None), (1, 3)])
            unit = CODEPOINTS if typ == pa.string() else BYTES
            for path in (1, 2):
                rows, offsets = c_slice(amd, arr, 4, unit, 0, NO_STOP, path)
                assert int(offsets[-1]) == 0 and not any(rows)


def _steps(amd):
    s = pa.array(["abcdef", None, "xy"], pa.string())
    for host, dev_fn, ref_fn, name in ((s, amd.compute.utf8_slice_codeunits, pc.utf8_slice_codeunits, "utf8_slice_codeunits"),
                                       (s.cast(pa.binary()), amd.compute.binary_slice, pc.binary_slice, "binary_slice")):
        dev = amd.Array.from_pyarrow(host)
        with pytest.raises(pa.ArrowInvalid) as want_err:
            ref_fn(host, 0, 4, 0)
        with pytest.raises(amd.ArrowInvalid) as got_err:
            dev_fn(dev, 0, 4, 0)
        assert str(got_err.value) == str(want_err.value) == "Slice step cannot be zero"
        for step in (2, -1):
            with pytest.raises(amd.ArrowNotImplementedError, match=f"{name} with step={step}"):
                dev_fn(dev, 0, 4, step)


def _mirror(amd):
    s = pa.array(["héllo", None, "", "日本"], pa.string())
    b = s.cast(pa.binary())
    ds, db = amd.Array.from_pyarrow(s), amd.Array.from_pyarrow(b)
    cp = amd.compute
    same(cp.call_function("utf8_length", [ds]), pc.utf8_length(s), s, "utf8_length")
    same(cp.call_function("binary_length", [db]), pc.binary_length(b), b, "binary_length")
    same(cp.call_function("utf8_slice_codeunits", [ds], cp.SliceOptions(1, 3)), pc.utf8_slice_codeunits(s, 1, 3), s, "utf8 slice")
    same(cp.call_function("binary_slice", [db], cp.SliceOptions(start=-2, stop=None)), pc.binary_slice(b, -2), b, "binary slice")
    sliced = cp.utf8_length(ds.slice(1))                    # the null count of a slice is not known: lazy
    assert sliced.null_count == 1 and sliced.to_pyarrow().to_pylist() == [None, 0, 2]
    ints = pa.array([1, 2, 3])
    for name, host, dev, args in (("binary_length", ints, amd.Array.from_pyarrow(ints), ()), ("utf8_length", b, db, ()),
                                  ("binary_slice", s, ds, (0, 2)), ("utf8_slice_codeunits", b, db, (0, 2))):
        with pytest.raises(pa.ArrowNotImplementedError) as want_err:
            getattr(pc, name)(host, *args)
        with pytest.raises(pa.ArrowNotImplementedError) as got_err:
            getattr(cp, name)(dev, *args)
        assert str(got_err.value) == str(want_err.value)
        assert "has no kernel matching input types" in str(got_err.value)


# ---------------------------------------------------------------- the C ABI directly
def c_length(amd, arr, owidth, unit, path, hint=None):
    """arx_string_length on `arr`: the raw lengths; the 0xEE guard word after them survives."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    span, keep, nbytes = c_buffers(arr, owidth)
    n = len(arr)
    out = to_device(np.full(n * owidth + 8, 0xEE, np.uint8))
    rc = lib.arx_string_length(C.byref(span), owidth, unit, nbytes if hint is None else hint, path, out.data_ptr(), None)
    assert rc == 0, lib.arx_last_error()
    sync(out)
    raw = out.cpu().numpy()
    assert (raw[n * owidth: n * owidth + 8] == 0xEE).all()
    return raw[: n * owidth].view(np.int32 if owidth == 4 else np.int64).copy()


def c_slice(amd, arr, owidth, unit, start, stop, path, hint=None):
    """arx_string_slice_offsets + arx_string_slice_data on `arr`: (the output rows as bytes, the output offsets); the 0xEE
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
    rc = lib.arx_string_slice_offsets(C.byref(span), owidth, unit, start, stop, nbytes if hint is None else hint, path, ws.data_ptr(),
                                      ws_bytes, out_offsets.data_ptr(), C.byref(total), None)
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


def _large_offsets(amd):
    rng = rng_for("large")
    small = column(rng, 1000, 0.1, pa.string())
    for small_t, large_t, unit in ((pa.string(), pa.large_string(), CODEPOINTS), (pa.binary(), pa.large_binary(), BYTES),
                                   (pa.string(), pa.large_string(), BYTES)):
        a4, a8 = small.cast(small_t).slice(5), small.cast(large_t).slice(5)
        want_len = (pc.utf8_length if unit == CODEPOINTS else pc.binary_length)(a4)
        assert (pc.utf8_length if unit == CODEPOINTS else pc.binary_length)(a8).type == pa.int64()
        want_len = np.array(want_len.fill_null(0).to_pylist())
        for path in (1, 2):
            l8, l4 = c_length(amd, a8, 8, unit, path), c_length(amd, a4, 4, unit, path)
            assert l8.dtype == np.int64 and l4.dtype == np.int32
            assert (l8 == want_len).all() and (l4 == want_len).all(), (unit, path)
            for start, stop in ((0, 2), (1, 2**31), (-3, NO_STOP), (5, -2), (-100, 3), (2, 1)):
                fn = pc.utf8_slice_codeunits if unit == CODEPOINTS else pc.binary_slice
                host = a4 if unit == CODEPOINTS else a4.cast(pa.binary())
                want = [b"" if r is None else (r.encode() if isinstance(r, str) else r)
                        for r in fn(host, start, None if stop == NO_STOP else stop).to_pylist()]
                rows8, off8 = c_slice(amd, a8, 8, unit, start, stop, path)
                rows4, off4 = c_slice(amd, a4, 4, unit, start, stop, path)
                assert rows8 == want and rows4 == want, (unit, path, start, stop)
                assert off8.dtype == np.int64 and (off8 == off4).all()


def leads(b):
    return [i for i, x in enumerate(b) if (x & 0xC0) != 0x80]


def position(b, k):
    """The position rule of csrc/string_slice.hip: codepoint k >= 0 begins at the (k + 1)-th byte that is no continuation
    byte, or at the row's end; k < 0 at the |k|-th such byte counted backwards, or at the row's start."""
    at = leads(b)
    if k >= 0:
        return at[k] if k < len(at) else len(b)
    return at[len(at) + k] if -k <= len(at) else 0


def rule_slice(b, start, stop):
    end = len(b) if stop is None else position(b, stop)
    return b[min(position(b, start), end): end]


def _invalid_utf8(amd):
    rows = [b"\x80\x80\x80", b"\xff\xfeab\x80\x80c", b"\xc3", b"", b"ok\xc3\xa9", b"\xa9\xa9\xc3\xa9\xa9z" * 9]
    arr = pa.array(rows + rows[::-1], pa.binary())
    rows = arr.to_pylist()
    for path in (1, 2):
        assert c_length(amd, arr, 4, CODEPOINTS, path).tolist() == [len(leads(b)) for b in rows], path
        for start in (0, 1, 2, 5, -1, -3, -100):
            for stop in (None, 0, 1, 3, 100, -1, -2):
                got, offsets = c_slice(amd, arr, 4, CODEPOINTS, start, NO_STOP if stop is None else stop, path)
                assert got == [rule_slice(b, start, stop) for b in rows], (path, start, stop)
                assert all(g in b for g, b in zip(got, rows))              # every output row is a sub-range of its row


def _c_abi_contract(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    arr = pa.array(["héllo", "b"], pa.string())
    span, keep, nbytes = c_buffers(arr, 4)
    ws_bytes = lib.arx_string_slice_workspace_bytes(2, 4)
    assert ws_bytes >= lib.arx_binary_take_workspace_bytes(2) and lib.arx_string_slice_workspace_bytes(2, 8) > ws_bytes
    ws = to_device(np.zeros(ws_bytes, np.uint8))
    out = to_device(np.full(64, 0xEE, np.uint8))
    out_bytes = to_device(np.full(64, 0xEE, np.uint8))
    total = C.c_int64(-1)

    def length(sp=span, width=4, unit=1, path=1, o=out):
        return lib.arx_string_length(C.byref(sp) if sp is not None else None, width, unit, nbytes, path,
                                     o.data_ptr() if o is not None else None, None)

    def offsets(sp=span, width=4, unit=1, path=1, w=ws, wb=ws_bytes, o=out, t=total):
        return lib.arx_string_slice_offsets(C.byref(sp) if sp is not None else None, width, unit, 0, 2, nbytes, path,
                                            w.data_ptr() if w is not None else None, wb, o.data_ptr() if o is not None else None,
                                            C.byref(t) if t is not None else None, None)

    def data(sp=span, width=4, w=ws, wb=ws_bytes, o=out, tb=4, d=out_bytes):
        return lib.arx_string_slice_data(C.byref(sp) if sp is not None else None, width, w.data_ptr() if w is not None else None, wb,
                                         o.data_ptr() if o is not None else None, tb, d.data_ptr() if d is not None else None, None)

    neg = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, -1, 0)
    cases = [(length, {"unit": 2}, b"unit 2"), (length, {"unit": -1}, b"unit -1"), (length, {"path": 3}, b"path 3"),
             (length, {"width": 2}, b"offset_width 2"), (length, {"sp": neg}, b"negative length"),
             (length, {"sp": None}, b"NULL values or out_lengths"), (length, {"o": None}, b"NULL values or out_lengths"),
             (offsets, {"unit": 2}, b"unit 2"), (offsets, {"path": -1}, b"path -1"), (offsets, {"width": 16}, b"offset_width 16"),
             (offsets, {"sp": neg}, b"negative length"), (offsets, {"sp": None}, b"NULL values, out_offsets or out_total_bytes"),
             (offsets, {"o": None}, b"NULL values, out_offsets or out_total_bytes"),
             (offsets, {"t": None}, b"NULL values, out_offsets or out_total_bytes"), (offsets, {"wb": ws_bytes - 1}, b"ws of"),
             (offsets, {"w": None}, b"ws of"), (data, {"width": 3}, b"offset_width 3"), (data, {"sp": neg}, b"negative length"),
             (data, {"sp": None}, b"NULL values"), (data, {"tb": -1}, b"negative total_bytes"), (data, {"wb": 8}, b"ws of"),
             (data, {"d": None}, b"NULL out_offsets, out_data or data")]
    for fn, kwargs, text in cases:
        assert fn(**kwargs) == _lib.ARX_INVALID, (fn.__name__, kwargs)
        assert text in lib.arx_last_error(), (fn.__name__, kwargs, lib.arx_last_error())
    sync(out)
    assert (out.cpu().numpy()[:64] == 0xEE).all()                       # a refused call writes nothing
    # length 0: success, nothing launched, nothing written but out_offsets[0]
    empty = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, 0, 0)
    before = (lib.arx_get_counter(ROW_COUNTER), lib.arx_get_counter(WAVE_COUNTER))
    for path in (0, 1, 2):
        for unit in (0, 1):
            assert length(sp=empty, unit=unit, path=path) == 0
            assert data(sp=empty, tb=0) == 0
    sync(out)
    assert (out.cpu().numpy()[:64] == 0xEE).all()
    for width in (4, 8):
        total.value = -1
        assert offsets(sp=empty, width=width, path=2) == 0 and total.value == 0
        sync(out)
        raw = out.cpu().numpy()
        assert (raw[:width] == 0).all() and (raw[width:64] == 0xEE).all()
        out[:64] = 0xEE
    assert (lib.arx_get_counter(ROW_COUNTER), lib.arx_get_counter(WAVE_COUNTER)) == before
    assert length() == 0 and offsets() == 0 and total.value == 4 and data() == 0
    sync(out)
    assert out_bytes.cpu().numpy()[:8].tobytes() == "hé".encode() + b"b" + b"\xee" * 4 and (out_bytes.cpu().numpy()[8:64] == 0xEE).all()


def _counters(amd):
    from arrow_amd import _lib

    lib = _lib.get_lib()
    count = lambda: (lib.arx_get_counter(ROW_COUNTER), lib.arx_get_counter(WAVE_COUNTER))  # noqa: E731
    rng = rng_for("counters")
    short_h = pa.array([bytes(r).decode() for r in np.split(rng.integers(97, 100, 16 * 500, dtype=np.uint8), 500)])
    wide_h = pa.array([bytes(r).decode() for r in np.split(rng.integers(97, 100, 4096 * 16, dtype=np.uint8), 16)])
    short, wide = amd.Array.from_pyarrow(short_h), amd.Array.from_pyarrow(wide_h)
    r0, w0 = count()
    with path_set(amd, KNOB, 0):
        got = amd.compute.utf8_length(short)
        assert count() == (r0 + 1, w0)
        same(got, pc.utf8_length(short_h), short_h, "auto short length")
        got = amd.compute.utf8_slice_codeunits(short, -3, None)
        assert count() == (r0 + 2, w0)
        same(got, pc.utf8_slice_codeunits(short_h, -3), short_h, "auto short slice")
        got = amd.compute.utf8_length(wide)
        assert count() == (r0 + 2, w0 + 1)
        same(got, pc.utf8_length(wide_h), wide_h, "auto wide length")
        got = amd.compute.utf8_slice_codeunits(wide, 5, -2)
        assert count() == (r0 + 2, w0 + 2)
        same(got, pc.utf8_slice_codeunits(wide_h, 5, -2), wide_h, "auto wide slice")
    for path in (0, 1, 2):                                   # byte units walk no codepoints
        with path_set(amd, KNOB, path):
            amd.compute.binary_length(wide)
            amd.compute.binary_length(short)
            amd.compute.binary_slice(amd.Array.from_pyarrow(wide_h.cast(pa.binary())), 1, 7)
    assert count() == (r0 + 2, w0 + 2)
    with path_set(amd, KNOB, 2):
        amd.compute.utf8_length(short)
    with path_set(amd, KNOB, 1):
        amd.compute.utf8_slice_codeunits(wide, 0, 2)
    assert count() == (r0 + 3, w0 + 3)


def test_reference_binary_slice_without_stop_still_raises():
    arr = pa.array([b"hello"] * 100, pa.binary())
    with pytest.raises(pa.ArrowInvalid, match="Negative buffer resize"):
        pc.binary_slice(arr, 1)
    assert pc.binary_slice(arr, 1, 2**31).to_pylist() == [b"ello"] * 100
    assert pc.binary_slice(arr, -3).to_pylist() == [b"llo"] * 100


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_string_length_grid(emu_ctx, n):
    _grid_lengths(emu_ctx, n)


@pytest.mark.emu
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("n", LENGTHS[:-1])
def test_string_slice_grid(emu_ctx, n, start):
    _grid_slices(emu_ctx, n, [start])


# (the emulator switches fibers at every wave collective: the largest row count takes one case per pair of bounds)
@pytest.mark.emu
@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("start", STARTS)
def test_string_slice_grid_4097_rows(emu_ctx, start, stop):
    _grid_slices(emu_ctx, LENGTHS[-1], [start], [stop])


@pytest.mark.emu
def test_string_slice_is_python_slicing(emu_ctx):
    _python_slicing(emu_ctx)


@pytest.mark.emu
def test_string_slice_characters_across_granule_and_wave_step_boundaries(emu_ctx):
    _straddles(emu_ctx)


@pytest.mark.emu
def test_string_slice_long_rows_among_short_ones(emu_ctx):
    _long_rows(emu_ctx)


@pytest.mark.emu
def test_string_slice_null_row_spanning_bytes(emu_ctx):
    _null_row_spanning_bytes(emu_ctx)


@pytest.mark.emu
def test_string_slice_all_null_and_all_empty(emu_ctx):
    _all_null_and_all_empty(emu_ctx)


@pytest.mark.emu
def test_string_slice_steps(emu_ctx):
    _steps(emu_ctx)


@pytest.mark.emu
def test_string_slice_mirror(emu_ctx):
    _mirror(emu_ctx)


@pytest.mark.emu
def test_string_slice_c_abi_large_offsets(emu_ctx):
    _large_offsets(emu_ctx)


@pytest.mark.emu
def test_string_slice_c_abi_invalid_utf8(emu_ctx):
    _invalid_utf8(emu_ctx)


@pytest.mark.emu
def test_string_slice_c_abi_contract(emu_ctx):
    _c_abi_contract(emu_ctx)


@pytest.mark.emu
def test_string_slice_counters_and_auto_path(emu_ctx):
    _counters(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
def test_gpu_string_length_grid(gpu_ctx):
    for n in LENGTHS:
        _grid_lengths(gpu_ctx, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_gpu_string_slice_grid(gpu_ctx, n):
    _grid_slices(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_string_slice_boundaries_and_long_rows(gpu_ctx):
    _python_slicing(gpu_ctx)
    _straddles(gpu_ctx)
    _long_rows(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_slice_null_rows_steps_and_mirror(gpu_ctx):
    _null_row_spanning_bytes(gpu_ctx)
    _all_null_and_all_empty(gpu_ctx)
    _steps(gpu_ctx)
    _mirror(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_slice_c_abi(gpu_ctx):
    _large_offsets(gpu_ctx)
    _invalid_utf8(gpu_ctx)
    _c_abi_contract(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_slice_counters(gpu_ctx):
    _counters(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_slice_1e6_rows_from_numpy_buffers(gpu_ctx):
    rng = rng_for("1e6")
    n = 1_000_000
    chars = rng.integers(0, 33, n)
    chars[rng.integers(0, n, 20)] = 30_000                        # a few long rows among the short ones
    char_offsets = np.zeros(n + 1, np.int64)
    np.cumsum(chars, out=char_offsets[1:])
    width = rng.integers(1, 3, int(char_offsets[-1]))              # 'a' .. 'z' or U+00E9 (c3 a9)
    at = np.zeros(len(width) + 1, np.int64)
    np.cumsum(width, out=at[1:])
    data = np.empty(int(at[-1]), np.uint8)
    data[at[:-1]] = np.where(width == 1, rng.integers(97, 123, len(width)), 0xC3)
    data[at[:-1][width == 2] + 1] = 0xA9
    offsets = at[char_offsets].astype(np.int32)
    valid = np.packbits(rng.random(n) >= 0.05, bitorder="little")
    for typ in (pa.string(), pa.binary()):
        arr = pa.Array.from_buffers(typ, n, [pa.py_buffer(valid.tobytes()), pa.py_buffer(offsets.tobytes()), pa.py_buffer(data.tobytes())])
        host, dev = arr.slice(13), gpu_ctx.Array.from_pyarrow(arr).slice(13)
        check_lengths(gpu_ctx, host, dev, paths=(0, 1, 2))
        check_slices(gpu_ctx, host, dev, [(0, 2), (-3, None), (5, -2), (3, 20_000)], paths=(0, 1, 2))
