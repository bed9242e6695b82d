"""Date / time field extraction (arrow_amd.compute.year .. nanosecond, arx_temporal_component, csrc/temporal.hip) against
pyarrow.compute on the host copies of the same arrays: values by `equals`, null_count, result offset 0, result type int64
and no validity buffer when the input has none — exact equality, no tolerances.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus one column of 10^6 rows built from numpy buffers per input type.  The known answers are explicit integers
per type (day numbers and in-unit offsets), not values that went through `datetime`."""
import ctypes as C

import numpy as np
import pytest

from . import util as U

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

# rows one wave takes at a time (csrc/temporal.hip): 64 lanes x 2 rows x kTemporalSteps
ROWS_PER_WAVE = (512,)
LENGTHS = [0, 1, 63, 64, 65] + [r + d for r in ROWS_PER_WAVE for d in (-1, 1)] + [4097, 100_000]
OFFSET = 13

CALENDAR = ["year", "quarter", "month", "day", "day_of_week", "day_of_year", "iso_year", "iso_week"]
TIME_OF_DAY = ["hour", "minute", "second", "millisecond", "microsecond", "nanosecond"]
COMPONENT = {name: i for i, name in enumerate(CALENDAR[:4] + ["day_of_week", "day_of_year", "iso_year", "iso_week"] + TIME_OF_DAY)}
# name -> (type, ARX_TIME_*, units per second or None for the two date types)
TYPES = {"date32": (pa.date32(), 0, None), "date64": (pa.date64(), 1, None),
         "timestamp[s]": (pa.timestamp("s"), 2, 1), "timestamp[ms]": (pa.timestamp("ms"), 3, 10**3),
         "timestamp[us]": (pa.timestamp("us"), 4, 10**6), "timestamp[ns]": (pa.timestamp("ns"), 5, 10**9),
         "time32[s]": (pa.time32("s"), 6, 1), "time32[ms]": (pa.time32("ms"), 7, 10**3),
         "time64[us]": (pa.time64("us"), 8, 10**6), "time64[ns]": (pa.time64("ns"), 9, 10**9)}
CALENDAR_TYPES = ["date32", "date64", "timestamp[s]", "timestamp[ms]", "timestamp[us]", "timestamp[ns]"]
TIME_TYPES = ["timestamp[s]", "timestamp[ms]", "timestamp[us]", "timestamp[ns]", "time32[s]", "time32[ms]", "time64[us]", "time64[ns]"]
PAIRS = [(f, t) for f in CALENDAR for t in CALENDAR_TYPES] + [(f, t) for f in TIME_OF_DAY for t in TIME_TYPES]
DAY_MIN, DAY_MAX = -719162, 2932896          # 0001-01-01 .. 9999-12-31


def rng_for(*key):
    return U.rng_for(0x7E3, *key)


def physical(t):
    return (np.int32, pa.int32()) if t.bit_width == 32 else (np.int64, pa.int64())


def typed(values, t, mask=None):
    """The integers `values` as a column of type t (nulls where mask is True; the integers stay underneath)."""
    dt, pt = physical(t)
    return pa.array(np.asarray(values, dtype=dt), pt, mask=mask).view(t)


def random_values(rng, name, n):
    """Random in-range instants of a type, as its physical integers."""
    t, _, per_second = TYPES[name]
    if name.startswith("time"):
        if name == "timestamp[ns]":
            return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)       # the whole range: years 1677 .. 2262
        if name.startswith("timestamp"):
            days = rng.integers(DAY_MIN, DAY_MAX, n, dtype=np.int64, endpoint=True)
            return days * (86400 * per_second) + rng.integers(0, 86400 * per_second, n, dtype=np.int64)
        return rng.integers(0, 86400 * per_second, n, dtype=np.int64)                      # time32 / time64: within one day
    days = rng.integers(DAY_MIN, DAY_MAX, n, dtype=np.int64, endpoint=True)
    return days if name == "date32" else days * 86_400_000


def column(rng, name, n, null_p):
    mask = (rng.random(n) < null_p) if null_p else None
    return typed(random_values(rng, name, n), TYPES[name][0], mask)


def sliced(rng, name, n, null_p):
    return column(rng, name, n + OFFSET + 3, null_p).slice(OFFSET, n)


def check(amd, fn, arr, what=(), want=None, **options):
    want = getattr(pc, fn)(arr, **options) if want is None else want
    src = amd.Array.from_pyarrow(arr)
    known = not callable(src._null_count) and src._null_count >= 0
    got = getattr(amd.compute, fn)(src, **options)
    assert got.type.name == "int64" and want.type == pa.int64(), (fn, what)
    assert got.offset == 0 and got.length == len(want), (fn, what)
    if known and arr.null_count:
        assert not callable(got._null_count), (fn, what)          # the input's count, without a read-back
    assert got.to_pyarrow().equals(want), (fn, what, str(arr.type), len(want))
    assert got.null_count == want.null_count, (fn, what, got.null_count, want.null_count)
    if arr.buffers()[0] is None:
        assert got.validity is None, (fn, what)
    return got


def _grid(amd, n):
    for nulls in (0.0, 0.1):
        columns = {name: sliced(rng_for("grid", n, name, nulls), name, n, nulls) for name in TYPES}
        for fn, name in PAIRS:
            check(amd, fn, columns[name], ("grid", n, name, nulls))


# ---------------------------------------------------------------- known answers
# (day number since 1970-01-01, what it is)
KNOWN_DAYS = [(0, "1970-01-01"), (-1, "1969-12-31"), (-719468, "0000-03-01"), (-719162, "0001-01-01"), (2932896, "9999-12-31"),
              (-25509, "1900-02-28"), (-25508, "1900-03-01"), (11016, "2000-02-29"), (47540, "2100-02-28"), (47541, "2100-03-01"),
              (12783, "2004-12-31"), (12784, "2005-01-01"), (14242, "2008-12-29"), (14612, "2010-01-03"), (18627, "2020-12-31"),
              (-12687428, "-32767-01-01"), (11248737, "32767-12-31")]
LAST_SECOND = 86399                        # 23:59:59


def known_values(name):
    """The known instants in the unit of a type: each day at 00:00:00 and at 23:59:59.999..., and -1; with the day
    number of each (None for the time types)."""
    _, _, per_second = TYPES[name]
    if name == "date32":
        return [d for d, _ in KNOWN_DAYS], [d for d, _ in KNOWN_DAYS]
    if name == "date64":
        return [d * 86_400_000 for d, _ in KNOWN_DAYS] + [-1], [d for d, _ in KNOWN_DAYS] + [-1]
    if name.startswith("timestamp"):
        per_day = 86400 * per_second
        days = [d for d, _ in KNOWN_DAYS if abs(d * per_day) < 2**63 - per_day]
        return ([d * per_day for d in days] + [d * per_day + LAST_SECOND * per_second + (per_second - 1) for d in days] + [-1],
                days + days + [-1])
    values = [0, LAST_SECOND * per_second + (per_second - 1), 12 * 3600 * per_second]
    return values, [None] * len(values)


def reference_known(fn, arr, days):
    """The reference's answer for the known instants — but for iso_week of -32767-01-01, a Saturday of ISO year -32768,
    a year beyond the reference's 16-bit field: it answers -3419452 there (its iso_year is right: -32768).  That year
    starts on a Thursday (as 2032 does, the same year modulo 400), so it has 53 weeks and the day lies in the last."""
    want = getattr(pc, fn)(arr)
    if fn != "iso_week" or -12687428 not in days:
        return want
    fixed = [53 if d == -12687428 and w is not None else w for w, d in zip(want.to_pylist(), days)]
    return pa.array(fixed, pa.int64())


def _known_answers(amd):
    for name, (t, _, _) in TYPES.items():
        values, days = known_values(name)
        plain = typed(values, t)
        valid = np.arange(len(values) + 2) % 5 != 1
        around = typed([7] + values + [7], t, mask=~valid).slice(1, len(values))      # a validity bitmap around them
        for fn, tname in PAIRS:
            if tname == name:
                check(amd, fn, plain, ("known", name), want=reference_known(fn, plain, days))
                check(amd, fn, around, ("known under a bitmap", name), want=reference_known(fn, around, days))
    run = lambda fn, arr: getattr(amd.compute, fn)(amd.Array.from_pyarrow(arr)).to_pyarrow().to_pylist()  # noqa: E731
    # before the epoch every division floors
    for unit in ("s", "ms", "us", "ns"):
        ts = typed([-1], pa.timestamp(unit))
        assert [run(f, ts) for f in ("year", "month", "day", "hour", "minute", "second")] == [[1969], [12], [31], [23], [59], [59]]
    ms = typed([-1], pa.timestamp("ms"))
    assert run("millisecond", ms) == [999] and run("microsecond", ms) == [0]
    ns = typed([-1], pa.timestamp("ns"))
    assert [run(f, ns) for f in ("millisecond", "microsecond", "nanosecond")] == [[999], [999], [999]]
    d = typed([-1, -719468, 12784, 14242, -12687428, 11248737], pa.date32())
    assert run("day_of_week", d)[0] == 2                                     # 1969-12-31, a Wednesday
    assert [run(f, d)[1] for f in ("year", "month", "day", "day_of_year", "iso_week")] == [0, 3, 1, 61, 9]
    assert (run("iso_year", d)[2], run("iso_week", d)[2]) == (2004, 53)        # 2005-01-01
    assert (run("iso_year", d)[3], run("iso_week", d)[3]) == (2009, 1)         # 2008-12-29
    assert run("year", d)[4:] == [-32767, 32767] and run("quarter", d)[4:] == [1, 4]
    last = typed([LAST_SECOND * 10**9 + 999_999_999], pa.time64("ns"))
    assert [run(f, last) for f in TIME_OF_DAY] == [[23], [59], [59], [999], [999], [999]]


def _garbage_under_nulls(amd):
    n = 700
    for name, (t, _, _) in TYPES.items():
        rng = rng_for("garbage", name)
        dt, _ = physical(t)
        info = np.iinfo(dt)
        values = random_values(rng, name, n).astype(dt)
        valid = rng.random(n) >= 0.3
        junk = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        junk[::3] = info.min
        junk[1::3] = info.max
        values[~valid] = junk[~valid]
        arr = pa.Array.from_buffers(t, n, [pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()), pa.py_buffer(values.tobytes())])
        assert arr.null_count == int((~valid).sum())
        for fn, tname in PAIRS:
            if tname == name:
                got = check(amd, fn, arr, ("garbage", name))
                data = got.data.cpu().numpy()[: n * 8].view(np.int64)
                assert (data[~valid] == 0).all(), (fn, name)                       # a null result slot: zero


def _day_of_week_options(amd):
    rng = rng_for("dow")
    for name in ("date32", "timestamp[us]"):
        arr = sliced(rng, name, 1000, 0.1)
        for week_start in range(1, 8):
            for count_from_zero in (True, False):
                check(amd, "day_of_week", arr, (name, week_start, count_from_zero), count_from_zero=count_from_zero, week_start=week_start)
        for bad in (0, 8):
            text = f"week_start must follow ISO convention \\(Monday=1, Sunday=7\\). Got week_start={bad}"
            with pytest.raises(pa.ArrowInvalid, match=text):
                pc.day_of_week(arr, week_start=bad)
            with pytest.raises(amd.ArrowInvalid, match=text):
                amd.compute.day_of_week(amd.Array.from_pyarrow(arr), week_start=bad)


def _mirror_and_refusals(amd):
    rng = rng_for("mirror")
    arr = column(rng, "timestamp[us]", 500, 0.1)
    d = amd.Array.from_pyarrow(arr)
    names = amd.compute.get_function_registry().get_function_names()
    for fn in CALENDAR + TIME_OF_DAY:
        assert fn in names
        assert amd.compute.call_function(fn, [d]).to_pyarrow().equals(getattr(pc, fn)(arr)), fn
    opts = amd.compute.DayOfWeekOptions(count_from_zero=False, week_start=7)
    assert amd.compute.call_function("day_of_week", [d], opts).to_pyarrow().equals(pc.day_of_week(arr, count_from_zero=False, week_start=7))
    # a slice does not know its null count: the result's is counted on first use, and right
    sl = amd.compute.year(d.slice(3))
    want = pc.year(arr.slice(3))
    assert sl.null_count == want.null_count and sl.to_pyarrow().equals(want)
    plain = amd.compute.month(amd.Array.from_pyarrow(column(rng, "date32", 300, 0.0)))
    assert plain.validity is None and plain.null_count == 0
    # ---- refusals: the reference's kernel lists, and time zones
    for fn, name in (("year", "time32[s]"), ("hour", "date64"), ("hour", "date32"), ("iso_week", "time64[ns]"), ("nanosecond", "date32")):
        host = column(rng, name, 10, 0.0)
        with pytest.raises(pa.ArrowNotImplementedError, match="has no kernel matching input types") as ref:
            getattr(pc, fn)(host)
        with pytest.raises(amd.ArrowNotImplementedError, match="has no kernel matching input types") as err:
            getattr(amd.compute, fn)(amd.Array.from_pyarrow(host))
        assert str(err.value) == f"Function '{fn}' has no kernel matching input types ({host.type})"
        assert str(err.value) in str(ref.value)
    ints = amd.Array.from_pyarrow(pa.array([1, 2, 3], pa.int64()))
    with pytest.raises(amd.ArrowNotImplementedError, match="has no kernel matching input types"):
        amd.compute.year(ints)
    zoned = typed([0, 1, 2], pa.timestamp("us")).cast(pa.timestamp("us", tz="UTC"))
    for fn in ("year", "hour", "day_of_week"):
        with pytest.raises(amd.ArrowNotImplementedError, match=rf"{fn} of timestamp\[us, tz=UTC\]"):
            getattr(amd.compute, fn)(amd.Array.from_pyarrow(zoned))


# ---------------------------------------------------------------- the C ABI directly
def c_operand(arr):
    """(ArxSpan, kept device buffers) of a host pyarrow array: its buffers uploaded as they are, offset and all."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    vb, db = arr.buffers()[:2]
    w = arr.type.bit_width // 8
    end = arr.offset + len(arr)
    keep = [to_device(np.frombuffer(vb, dtype=np.uint8)[: (end + 7) // 8]) if vb is not None else None,
            to_device(np.frombuffer(db, dtype=np.uint8)[: end * w])]
    return _lib.ArxSpan(keep[0].data_ptr() if keep[0] is not None else None, keep[1].data_ptr(), arr.offset, len(arr),
                        arr.null_count if vb is not None else 0), keep


def c_temporal(fn, name, arr, week_start=1, count_from_zero=1, with_validity=True, pad=64):
    """arx_temporal_component on a host pyarrow array: (rc, raw data bytes, raw validity bytes | None); both output
    buffers are filled with 0xEE first and carry `pad` bytes after what the call may write."""
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n = len(arr)
    words = (n + 63) // 64
    span, keep = c_operand(arr)
    out = to_device(np.full(n * 8 + pad, 0xEE, np.uint8))
    valid = to_device(np.full(words * 8 + pad, 0xEE, np.uint8)) if with_validity else None
    rc = lib.arx_temporal_component(COMPONENT[fn], TYPES[name][1], C.byref(span), n, week_start, count_from_zero, out.data_ptr(),
                                    valid.data_ptr() if with_validity else None, None)
    if out.is_cuda:
        torch.cuda.synchronize()
    return rc, out.cpu().numpy()[: n * 8 + pad], (valid.cpu().numpy()[: words * 8 + pad] if with_validity else None)


def _c_abi(amd):
    from arrow_amd import _lib

    lib = _lib.get_lib()
    for fn, name in (("year", "date32"), ("day_of_year", "timestamp[us]"), ("iso_week", "date64"), ("day_of_week", "timestamp[s]"),
                     ("minute", "time32[ms]"), ("nanosecond", "timestamp[ns]"), ("millisecond", "time64[us]")):
        for n in (1, 64, 65, 127, 129, 511, 513, 1001):
            for null_p in (0.1, 0.0):
                rng = rng_for("c abi", fn, name, n, null_p)
                arr = sliced(rng, name, n, null_p)
                what = (fn, name, n, null_p)
                want = getattr(pc, fn)(arr)
                words = (n + 63) // 64
                rc, data, valid = c_temporal(fn, name, arr)
                assert rc == 0, (what, lib.arx_last_error())
                assert (data[n * 8:] == 0xEE).all(), what                      # nothing past length * 8
                assert (valid[words * 8:] == 0xEE).all(), what                 # nothing past the last validity word
                if arr.buffers()[0] is None:
                    # no input bitmap: the words are all ones below length (padding bits zero) when a buffer is given ...
                    vbits = np.unpackbits(valid[: words * 8], bitorder="little")
                    assert vbits[:n].all() and not vbits[n:].any(), what
                    # ... and the call takes none
                    rc2, data2, _ = c_temporal(fn, name, arr, with_validity=False)
                    assert rc2 == 0 and (data2 == data).all(), what
                else:
                    vbits = np.unpackbits(valid[: words * 8], bitorder="little")
                    assert not vbits[n:].any(), what                           # padding bits of the last word: zero
                    rc2, data2, _ = c_temporal(fn, name, arr, with_validity=False)
                    assert rc2 == _lib.ARX_INVALID and b"NULL out_validity" in lib.arx_last_error(), what
                    assert (data2 == 0xEE).all(), what
                got = pa.Array.from_buffers(pa.int64(), n, [pa.py_buffer(valid[: words * 8].tobytes()), pa.py_buffer(data[: n * 8].tobytes())])
                assert got.equals(want) and got.null_count == want.null_count, what
                assert not data[: n * 8].view(np.int64)[~vbits[:n].astype(bool)].any(), what      # null slots: zero


def _invalid_arguments(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n = 100
    rng = rng_for("invalid")
    spans, keep = {}, []
    for name in ("date32", "timestamp[us]", "time32[s]", "time64[ns]"):
        spans[name], bufs = c_operand(column(rng, name, n, 0.1))
        keep.append(bufs)
    spans["plain"], bufs = c_operand(column(rng, "timestamp[us]", n, 0.0))
    keep.append(bufs)
    out = to_device(np.full(n * 8 + 64, 0xEE, np.uint8))
    valid = to_device(np.full(16 + 64, 0xEE, np.uint8))
    counters = (b"temporal_civil_launches", b"temporal_iso_launches", b"temporal_weekday_launches", b"temporal_time_launches")
    count = lambda: tuple(lib.arx_get_counter(c) for c in counters)  # noqa: E731
    before = count()

    def call(fn="year", name="timestamp[us]", span="timestamp[us]", length=n, week_start=1, o=out, v=valid, component=None, in_type=None):
        return lib.arx_temporal_component(COMPONENT[fn] if component is None else component, TYPES[name][1] if in_type is None else in_type,
                                          C.byref(spans[span]) if span is not None else None, length, week_start, 1,
                                          o.data_ptr() if o is not None else None, v.data_ptr() if v is not None else None, None)

    for kwargs, text in (({"fn": "year", "name": "time32[s]", "span": "time32[s]"}, b"no kernel for component"),
                         ({"fn": "iso_week", "name": "time64[ns]", "span": "time64[ns]"}, b"no kernel for component"),
                         ({"fn": "hour", "name": "date32", "span": "date32"}, b"no kernel for component"),
                         ({"fn": "second", "name": "date64"}, b"no kernel for component"),
                         ({"component": 14}, b"no kernel for component"), ({"component": -1}, b"no kernel for component"),
                         ({"in_type": 10}, b"no kernel for component"), ({"in_type": -1}, b"no kernel for component"),
                         ({"week_start": 0}, b"Got week_start=0"), ({"week_start": 8}, b"Got week_start=8"),
                         ({"fn": "day_of_week", "week_start": 8}, b"week_start must follow ISO convention (Monday=1, Sunday=7). Got week_start=8"),
                         ({"length": -1}, b"negative length"), ({"span": None}, b"NULL values"), ({"o": None}, b"NULL out_data"),
                         ({"v": None}, b"NULL out_validity")):
        assert call(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    untouched = lambda: (out.cpu().numpy()[: n * 8 + 64] == 0xEE).all() and (valid.cpu().numpy()[: 16 + 64] == 0xEE).all()  # noqa: E731
    assert untouched() and count() == before
    # length 0 succeeds, launches nothing and writes nothing
    spans["empty"] = _lib.ArxSpan(spans["timestamp[us]"].validity, spans["timestamp[us]"].data, 0, 0, 0)
    for fn in ("year", "iso_year", "day_of_week", "hour"):
        assert call(fn=fn, span="empty", length=0) == 0
        assert call(fn=fn, span="empty", length=0, o=None, v=None) == 0
    assert untouched() and count() == before
    # the counter names the kernel: one input of each decomposition group
    assert call(fn="month") == 0 and count() == (before[0] + 1, before[1], before[2], before[3])
    assert call(fn="iso_week") == 0 and count() == (before[0] + 1, before[1] + 1, before[2], before[3])
    assert call(fn="day_of_week", week_start=7) == 0 and count() == (before[0] + 1, before[1] + 1, before[2] + 1, before[3])
    assert call(fn="second") == 0 and count() == (before[0] + 1, before[1] + 1, before[2] + 1, before[3] + 1)
    assert call(fn="day", name="date32", span="date32") == 0 and count()[0] == before[0] + 2
    assert call(fn="hour", name="time64[ns]", span="time64[ns]") == 0 and count()[3] == before[3] + 2
    # no input bitmap: no output bitmap is asked for, and none is written
    valid[:] = 0xEE
    assert call(span="plain", v=None) == 0 and count()[0] == before[0] + 3
    assert (valid.cpu().numpy()[: 16 + 64] == 0xEE).all()


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_temporal_grid(emu_ctx, n):
    _grid(emu_ctx, n)


@pytest.mark.emu
def test_temporal_known_answers(emu_ctx):
    _known_answers(emu_ctx)


@pytest.mark.emu
def test_temporal_garbage_under_nulls(emu_ctx):
    _garbage_under_nulls(emu_ctx)


@pytest.mark.emu
def test_temporal_day_of_week_options(emu_ctx):
    _day_of_week_options(emu_ctx)


@pytest.mark.emu
def test_temporal_mirror_and_refusals(emu_ctx):
    _mirror_and_refusals(emu_ctx)


@pytest.mark.emu
def test_temporal_c_abi_written_bytes(emu_ctx):
    _c_abi(emu_ctx)


@pytest.mark.emu
def test_temporal_c_abi_invalid_arguments_length_zero_and_counters(emu_ctx):
    _invalid_arguments(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
def test_gpu_temporal_grid(gpu_ctx):
    for n in LENGTHS:
        _grid(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_temporal_known_answers_and_garbage(gpu_ctx):
    _known_answers(gpu_ctx)
    _garbage_under_nulls(gpu_ctx)


@pytest.mark.gpu
def test_gpu_temporal_options_mirror_and_refusals(gpu_ctx):
    _day_of_week_options(gpu_ctx)
    _mirror_and_refusals(gpu_ctx)


@pytest.mark.gpu
def test_gpu_temporal_c_abi(gpu_ctx):
    _c_abi(gpu_ctx)
    _invalid_arguments(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TYPES))
def test_gpu_temporal_1e6_rows_from_numpy_buffers(gpu_ctx, name):
    rng = rng_for("1e6", name)
    n = 1_000_000
    t = TYPES[name][0]
    total = n + OFFSET
    valid = np.packbits(rng.random(total) >= 0.05, bitorder="little")
    data = random_values(rng, name, total).astype(physical(t)[0])
    arr = pa.Array.from_buffers(t, total, [pa.py_buffer(valid.tobytes()), pa.py_buffer(data.tobytes())]).slice(OFFSET)
    for fn in (("year", "iso_week") if name in CALENDAR_TYPES else ()) + (("hour", "millisecond") if name in TIME_TYPES else ()):
        check(gpu_ctx, fn, arr, ("1e6", name))
