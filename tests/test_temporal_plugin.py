"""pc.year .. pc.nanosecond through the Arrow registration shim (plugin/temporal.inc) on device-resident arrays.

The script runs in a fresh interpreter, like tests/test_if_else_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the CPU
tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  Every function on every input type of
its list: the device-resident call must equal the same call on the host copy (at slice 0 and at slice 7), leave its
result in HBM (without a bitmap when the input has none) and raise the shim's GPU counter of that function by exactly
one; host arrays keep the reference's kernels and results, zoned timestamps included where the reference can do them;
day_of_week carries its options on both paths; a zoned timestamp on the device and a device array under the guarded
temporal siblings (is_leap_year, strftime, floor_temporal, ...) are refused with a Status; the guarded siblings' host
results are what they were before registration; an Acero plan table_source_rocm -> project(year, month) ->
aggregate_rocm equals the host plan."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TEMPORAL_SCRIPT = textwrap.dedent(r'''
    import ctypes, os, sys, faulthandler
    faulthandler.enable()
    import numpy as np
    import pyarrow as pa, pyarrow.compute as pc, pyarrow.acero as acero
    sys.path.insert(0, ROOT)
    SC = lambda x: max(64, int(x * float(os.environ.get("ARROW_AMD_TEST_SCALE", "1"))))
    if os.environ.get("ARROW_AMD_PLUGIN_EMULATED") == "1":
        from tests.emu.build_plugin_emu import build_plugin
    else:
        from arrow_amd.plugin_build import build_plugin
    path = build_plugin()
    rng = np.random.default_rng(43)
    n = SC(100_000)
    CALENDAR = ["year", "quarter", "month", "day", "day_of_week", "day_of_year", "iso_year", "iso_week"]
    TIME_OF_DAY = ["hour", "minute", "second", "millisecond", "microsecond", "nanosecond"]
    DAY_MIN, DAY_MAX = -719162, 2932896          # 0001-01-01 .. 9999-12-31
    def column(t, null_p=0.1):
        mask = (rng.random(n) < null_p) if null_p else None
        if pa.types.is_time(t):
            per_second = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}[t.unit]
            values = rng.integers(0, 86400 * per_second, n, dtype=np.int64)
        elif t == pa.timestamp("ns"):
            values = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
        else:
            days = rng.integers(DAY_MIN, DAY_MAX, n, dtype=np.int64, endpoint=True)
            per_day = 1 if t == pa.date32() else 86_400_000 if t == pa.date64() else 86400 * {"s": 1, "ms": 10**3, "us": 10**6}[t.unit]
            values = days * per_day + (rng.integers(0, per_day, n, dtype=np.int64) if pa.types.is_timestamp(t) else 0)
        if t.bit_width == 32:
            return pa.array(values.astype(np.int32), pa.int32(), mask=mask).view(t)
        return pa.array(values, pa.int64(), mask=mask).view(t)
    CALENDAR_TYPES = [pa.date32(), pa.date64(), pa.timestamp("s"), pa.timestamp("ms"), pa.timestamp("us"), pa.timestamp("ns")]
    TIME_TYPES = CALENDAR_TYPES[2:] + [pa.time32("s"), pa.time32("ms"), pa.time64("us"), pa.time64("ns")]
    columns = {str(t): column(t) for t in CALENDAR_TYPES + TIME_TYPES[4:]}
    plain = {str(t): column(t, 0.0) for t in (pa.date32(), pa.timestamp("us"), pa.time64("ns"))}
    pairs = [(f, str(t)) for f in CALENDAR for t in CALENDAR_TYPES] + [(f, str(t)) for f in TIME_OF_DAY for t in TIME_TYPES]
    want = {(f, t, sl): getattr(pc, f)(columns[t].slice(sl)) for f, t in pairs for sl in (0, 7)}
    want_plain = {(f, t): getattr(pc, f)(plain[t]) for f, t in pairs if t in plain}
    dow_options = [dict(count_from_zero=False, week_start=7), dict(count_from_zero=True, week_start=3), dict(count_from_zero=False, week_start=1)]
    want_dow = [pc.day_of_week(columns["timestamp[us]"], **o) for o in dow_options]
    # the guarded siblings without a device kernel: the same host calls before and after registration
    siblings = {"is_leap_year": lambda a: pc.is_leap_year(a), "subsecond": lambda a: pc.subsecond(a), "week": lambda a: pc.week(a),
                "us_week": lambda a: pc.us_week(a), "us_year": lambda a: pc.us_year(a), "year_month_day": lambda a: pc.year_month_day(a),
                "iso_calendar": lambda a: pc.iso_calendar(a), "strftime": lambda a: pc.strftime(a, format="%Y-%m-%dT%H:%M:%S"),
                "floor_temporal": lambda a: pc.floor_temporal(a, 3, "hour"), "ceil_temporal": lambda a: pc.ceil_temporal(a, 1, "day"),
                "round_temporal": lambda a: pc.round_temporal(a, 15, "minute")}
    recent = pa.array(rng.integers(0, 4 * 10**15, n), pa.int64(), mask=rng.random(n) < 0.1).view(pa.timestamp("us"))   # 1970 .. 2096
    # (the reference's own year_month_day on a host array of 64 rows or more brings the process down, in the call or
    # in whatever runs next, with or without this shim: its host call takes three rows)
    host_rows = lambda name: recent.slice(0, 3) if name == "year_month_day" else recent
    def outcome(f, arr):
        # the result, or the reference's own error (strftime needs the tz database even for a naive timestamp)
        try:
            return f(arr)
        except pa.ArrowException as e:
            return f"{type(e).__name__}: {e}"
    same = lambda x, y: x == y if isinstance(x, str) or isinstance(y, str) else x.equals(y)
    want_siblings = {name: outcome(f, host_rows(name)) for name, f in siblings.items()}
    assert sum(isinstance(w, str) for w in want_siblings.values()) <= 1, want_siblings
    v = pa.array(rng.integers(-100, 100, n), pa.int64(), mask=rng.random(n) < 0.05)
    d = pa.array(rng.integers(0, 20000, n).astype(np.int32), pa.int32(), mask=rng.random(n) < 0.05).view(pa.date32())
    table = pa.table({"d": d, "v": v})
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("project", acero.ProjectNodeOptions([pc.year(pc.field("d")), pc.month(pc.field("d")), pc.field("v")], ["y", "m", "v"])),
            acero.Declaration("aggregate_rocm" if source == "table_source_rocm" else "aggregate",
                              acero.AggregateNodeOptions([("v", "hash_sum", None, "s")], keys=["y", "m"]))])
    by_keys = [("y", "ascending"), ("m", "ascending")]
    want_plan = plan("table_source", table).to_table(use_threads=False).sort_by(by_keys)
    assert want_plan.num_rows > 100

    lib = ctypes.CDLL(path)
    lib.arrow_amd_plugin_last_error.restype = ctypes.c_char_p
    lib.arrow_amd_plugin_calls.restype = ctypes.c_int64
    lib.arrow_amd_plugin_calls.argtypes = [ctypes.c_char_p, ctypes.c_int]
    assert lib.arrow_amd_register() == 0, lib.arrow_amd_plugin_last_error()

    def to_device(arr):
        c_arr, c_schema, c_dev = (ctypes.create_string_buffer(m) for m in (80, 72, 128))
        arr._export_to_c(ctypes.addressof(c_arr), ctypes.addressof(c_schema))
        assert lib.arrow_amd_copy_to_device(c_arr, c_schema, c_dev) == 0, lib.arrow_amd_plugin_last_error()
        return pa.Array._import_from_c_device(ctypes.addressof(c_dev), arr.type)

    def to_host(darr):
        c_dev, c_schema, c_arr, c_schema2 = (ctypes.create_string_buffer(m) for m in (128, 72, 80, 72))
        darr._export_to_c_device(ctypes.addressof(c_dev), ctypes.addressof(c_schema))
        assert lib.arrow_amd_copy_to_host(c_dev, c_schema, c_arr, c_schema2) == 0, lib.arrow_amd_plugin_last_error()
        return pa.Array._import_from_c(ctypes.addressof(c_arr), ctypes.addressof(c_schema2))

    calls = lambda f, gpu: lib.arrow_amd_plugin_calls(f.encode(), gpu)
    for f in CALENDAR + TIME_OF_DAY:
        assert calls(f, 1) == 0 and calls(f, 0) == 0, f
    # ---- device-resident arrays: equal to the reference on the host copies, results in HBM, one GPU count per call
    device = {t: to_device(a) for t, a in columns.items()}
    device_plain = {t: to_device(a) for t, a in plain.items()}
    done = 0
    for f, t in pairs:
        for sl in (0, 7):
            g0 = calls(f, 1)
            got = getattr(pc, f)(device[t].slice(sl))
            assert calls(f, 1) == g0 + 1, (f, t, sl)
            done += 1
            assert got.buffers()[1] is not None and not got.buffers()[1].is_cpu, (f, t)
            w = want[f, t, sl]
            assert got.type == pa.int64() and got.offset == 0, (f, t, got.type)
            h = to_host(got)
            assert h.equals(w) and h.null_count == w.null_count, (f, t, sl)
        if t in plain:
            g0 = calls(f, 1)
            got = getattr(pc, f)(device_plain[t])
            assert calls(f, 1) == g0 + 1, (f, t)
            assert got.buffers()[0] is None and not got.buffers()[1].is_cpu, (f, t)      # no bitmap in, no bitmap out
            h = to_host(got)
            assert h.equals(want_plain[f, t]) and h.null_count == 0, (f, t)
    assert all(calls(f, 0) == 0 for f in CALENDAR + TIME_OF_DAY)
    # ---- host arrays keep the reference's kernels and results; the stock counter rises
    for f, t in pairs:
        s0 = calls(f, 0)
        assert getattr(pc, f)(columns[t].slice(7)).equals(want[f, t, 7]), (f, t)
        assert calls(f, 0) == s0 + 1, (f, t)
    assert pc.year(pa.scalar(0, pa.timestamp("s"))).as_py() == 1970
    # ---- day_of_week with options, both paths; a bad week_start is the reference's error on both
    for o, w in zip(dow_options, want_dow):
        assert pc.day_of_week(columns["timestamp[us]"], **o).equals(w), o
        assert to_host(pc.day_of_week(device["timestamp[us]"], **o)).equals(w), o
    for arr in (columns["date32[day]"], device["date32[day]"]):
        try:
            pc.day_of_week(arr, week_start=8)
            raise SystemExit("week_start=8 was accepted")
        except pa.ArrowInvalid as e:
            assert "week_start must follow ISO convention (Monday=1, Sunday=7). Got week_start=8" in str(e), e
    # ---- refused with a Status, not read by a CPU kernel
    zoned = to_device(columns["timestamp[us]"].cast(pa.timestamp("us", tz="UTC")))
    gpu_before = {f: calls(f, 1) for f in CALENDAR + TIME_OF_DAY}
    for f in ("year", "hour", "day_of_week"):
        try:
            getattr(pc, f)(zoned)
            raise SystemExit(f"{f}: a zoned device timestamp was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and f in str(e) and "tz=UTC" in str(e), (f, e)
    drecent = to_device(recent)
    for name, f in siblings.items():
        try:
            f(drecent)
            raise SystemExit(f"{name}: a device array was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and name in str(e), (name, e)
    for f, arr in (("year", device["time64[ns]"]), ("hour", device["date32[day]"])):
        try:
            getattr(pc, f)(arr)
            raise SystemExit(f"{f}: accepted a type it has no kernel for")
        except pa.ArrowNotImplementedError as e:
            assert "has no kernel matching input types" in str(e), (f, e)
    assert gpu_before == {f: calls(f, 1) for f in CALENDAR + TIME_OF_DAY}
    # ---- the guarded siblings' host results are what they were before registration
    for name, f in siblings.items():
        assert same(outcome(f, host_rows(name)), want_siblings[name]), name
    # ---- Acero: table_source_rocm -> project(year(d), month(d), v) -> aggregate_rocm over a device table equals the host plan
    g0 = calls("year", 1), calls("month", 1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=-(-n // 3))])
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by(by_keys)
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls("year", 1) - g0[0] >= 1 and calls("month", 1) - g0[1] >= 1
    print("TEMPORAL_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + TEMPORAL_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_temporal_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.01)
    assert r.returncode == 0 and "TEMPORAL_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_temporal_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "TEMPORAL_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
