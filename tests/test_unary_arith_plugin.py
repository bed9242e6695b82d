"""pc.negate .. pc.round_to_multiple through the Arrow registration shim (plugin/unary_arith.inc) on device-resident arrays.

The script runs in a fresh interpreter, like tests/test_temporal_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the CPU
tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  Every function on every type of its
list: the device-resident call must equal the same call on the host copy bit for bit on the valid slots (at slice 0 and at
slice 7), leave its result in HBM (without a bitmap when the input has none) and raise the shim's GPU counter
(`unary_arith` or `round`) by exactly one; host arrays and scalars keep the reference's kernels and results; pc.floor of a
device int32 column goes through the shim's device cast; round_binary and a decimal128 abs on a device array are refused
with a Status; the rounding and overflow errors arrive as the reference's Statuses; an Acero plan table_source_rocm ->
project(round(abs(v) * 0.37, 2), sign(v), -v) -> aggregate_rocm equals the host plan."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNARY_SCRIPT = textwrap.dedent(r'''
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
    rng = np.random.default_rng(47)
    n = SC(50_000)
    INTS = {"int8": np.int8, "uint8": np.uint8, "int16": np.int16, "uint16": np.uint16, "int32": np.int32, "uint32": np.uint32,
            "int64": np.int64, "uint64": np.uint64}
    FLOATS = {"float": np.float32, "double": np.float64}
    PA = {"int8": pa.int8(), "uint8": pa.uint8(), "int16": pa.int16(), "uint16": pa.uint16(), "int32": pa.int32(), "uint32": pa.uint32(),
          "int64": pa.int64(), "uint64": pa.uint64(), "float": pa.float32(), "double": pa.float64()}
    MODES = ["down", "up", "towards_zero", "towards_infinity", "half_down", "half_up", "half_towards_zero", "half_towards_infinity",
             "half_to_even", "half_to_odd"]
    def column(name, null_p=0.1):
        # integers away from the ends of their type (no row overflows), floats over 12 decades with the awkward values in front
        if name in INTS:
            info = np.iinfo(INTS[name])
            values = rng.integers(info.min // 2, info.max // 2, n, dtype=INTS[name], endpoint=True)
        else:
            values = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 6, n)).astype(FLOATS[name])
            values[:12] = [0.0, -0.0, np.nan, np.inf, -np.inf, 0.5, -0.5, 2.5, 2.675, 1.005, -0.4, 1e-40]
        valid = rng.random(n) >= null_p if null_p else None
        vbuf = None if valid is None else pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
        return pa.Array.from_buffers(PA[name], n, [vbuf, pa.py_buffer(values.tobytes())])
    columns = {name: column(name) for name in PA}
    plain = {name: column(name, 0.0) for name in ("int32", "uint8", "double")}
    def functions(name):
        fns = [("negate", {}), ("abs", {}), ("abs_checked", {}), ("sign", {}), ("round", {}), ("round", {"ndigits": -1, "round_mode": "half_up"}),
               ("round_to_multiple", {"multiple": 3, "round_mode": "half_towards_zero"}), ("round_to_multiple", {})]
        if not name.startswith("u"):
            fns.append(("negate_checked", {}))
        if name in FLOATS:
            fns += [("floor", {}), ("ceil", {}), ("trunc", {}), ("round", {"ndigits": 2}), ("round", {"ndigits": 11, "round_mode": "down"}),
                    ("round_to_multiple", {"multiple": 0.25, "round_mode": "up"})]
            fns += [("round", {"ndigits": 1, "round_mode": m}) for m in MODES]
        else:
            fns += [("round", {"ndigits": -1, "round_mode": m}) for m in MODES]
        return fns
    cases = [(f, name, tuple(sorted(o.items()))) for name in PA for f, o in functions(name)]
    want = {(f, name, o, sl): getattr(pc, f)(columns[name].slice(sl), **dict(o)) for f, name, o in cases for sl in (0, 7)}
    want_plain = {(f, name, o): getattr(pc, f)(plain[name], **dict(o)) for f, name, o in cases if name in plain}
    want_floor_i32 = pc.floor(columns["int32"])
    want_scalar = pc.round(pa.scalar(2.675), 2), pc.negate(pa.scalar(5, pa.int8())), pc.round_to_multiple(pa.scalar(7, pa.int32()), 5)
    # (v is float64 in quarter steps: sums of -v are exact in any order, and the plan needs no cast — a cast inside an
    # expression binds the reference's cast kernel, which is not this change's to take over)
    v = pa.array(rng.integers(-20, 20, n).astype(np.float64) / 4, pa.float64(), mask=rng.random(n) < 0.05)
    table = pa.table({"v": v})
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("project", acero.ProjectNodeOptions(
                [pc.round(pc.multiply(pc.abs(pc.field("v")), 0.37), 2), pc.sign(pc.field("v")), pc.negate(pc.field("v"))],
                ["r", "s", "m"])),
            acero.Declaration("aggregate_rocm" if source == "table_source_rocm" else "aggregate",
                              acero.AggregateNodeOptions([("m", "hash_sum", None, "total"), ("r", "hash_max", None, "largest"),
                                                          ("r", "hash_count", None, "rows")], keys=["s"]))])
    want_plan = plan("table_source", table).to_table(use_threads=False).sort_by([("s", "ascending")])
    assert want_plan.num_rows == 4          # -1, 0, 1 and null

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

    def same(got, w):
        # type, validity, null count, and the valid slots bit for bit
        if got.type != w.type or len(got) != len(w) or got.null_count != w.null_count:
            return False
        ok = np.ones(len(w), bool) if w.null_count == 0 else np.asarray(w.is_valid().to_numpy(zero_copy_only=False), bool)
        gok = np.ones(len(w), bool) if got.null_count == 0 else np.asarray(got.is_valid().to_numpy(zero_copy_only=False), bool)
        bits = lambda a: np.frombuffer(a.buffers()[1], dtype=f"u{a.type.bit_width // 8}", count=a.offset + len(a))[a.offset:]
        return bool((gok == ok).all() and (bits(got)[ok] == bits(w)[ok]).all())

    calls = lambda f, gpu: lib.arrow_amd_plugin_calls(f.encode(), gpu)
    counter = lambda f: "round" if f.startswith("round") else "unary_arith"
    assert all(calls(c, g) == 0 for c in ("unary_arith", "round") for g in (0, 1))
    # ---- device-resident arrays: equal to the reference on the host copies, results in HBM, one GPU count per call
    device = {name: to_device(a) for name, a in columns.items()}
    device_plain = {name: to_device(a) for name, a in plain.items()}
    done = 0
    for f, name, o in cases:
        for sl in (0, 7):
            g0 = calls(counter(f), 1)
            got = getattr(pc, f)(device[name].slice(sl), **dict(o))
            assert calls(counter(f), 1) == g0 + 1, (f, name, o, sl)
            done += 1
            assert got.buffers()[1] is not None and not got.buffers()[1].is_cpu and got.offset == 0, (f, name, o)
            assert same(to_host(got), want[f, name, o, sl]), (f, name, o, sl)
        if name in plain:
            got = getattr(pc, f)(device_plain[name], **dict(o))
            assert got.buffers()[0] is None and not got.buffers()[1].is_cpu, (f, name, o)      # no bitmap in, no bitmap out
            assert same(to_host(got), want_plain[f, name, o]), (f, name, o)
    assert calls("unary_arith", 0) == 0 and calls("round", 0) == 0
    # ---- host arrays and scalars keep the reference's kernels and results; the stock counter rises
    for f, name, o in cases:
        s0 = calls(counter(f), 0)
        assert same(getattr(pc, f)(columns[name].slice(7), **dict(o)), want[f, name, o, 7]), (f, name, o)
        assert calls(counter(f), 0) == s0 + 1, (f, name, o)
    got_scalar = pc.round(pa.scalar(2.675), 2), pc.negate(pa.scalar(5, pa.int8())), pc.round_to_multiple(pa.scalar(7, pa.int32()), 5)
    assert all(g.equals(w) for g, w in zip(got_scalar, want_scalar)), got_scalar
    # ---- floor of an integer column: DispatchBest casts to double, on the device, then the float kernel
    g0, c0 = calls("unary_arith", 1), calls("cast", 1)
    got = pc.floor(device["int32"])
    assert not got.buffers()[1].is_cpu and same(to_host(got), want_floor_i32)
    assert calls("unary_arith", 1) == g0 + 1 and calls("cast", 1) == c0 + 1
    # ---- errors: the reference's Statuses, on both paths
    def error_of(f, arr, **o):
        try:
            getattr(pc, f)(arr, **o)
        except pa.ArrowException as e:
            return type(e).__name__, str(e)
        raise SystemExit(f"{f}({arr.type}, {o}) was accepted")
    def both(f, arr, **o):
        host, dev = error_of(f, arr, **o), error_of(f, to_device(arr), **o)
        assert host == dev, (f, o, host, dev)
        return dev
    assert both("negate_checked", pa.array([1, -128, 3], pa.int8())) == ("ArrowInvalid", "overflow")
    assert both("abs_checked", pa.array([-2**63, 5], pa.int64())) == ("ArrowInvalid", "overflow")
    under_null = pa.Array.from_buffers(pa.int8(), 3, [pa.py_buffer(b"\x05"), pa.py_buffer(np.array([1, -128, 3], np.int8).tobytes())])
    assert to_host(pc.abs_checked(to_device(under_null))).to_pylist() == [1, None, 3]
    assert both("round", pa.array([1.0, 1e308]), ndigits=2) == ("ArrowInvalid", "overflow occurred during rounding")
    assert both("round", pa.array([32766, 5, 32767, 7], pa.int16()), ndigits=-1, round_mode="up") == \
        ("ArrowInvalid", "Rounding 32767 up to multiple of 10 would overflow")
    assert both("round", pa.array([32767, 5, -32768], pa.int16()), ndigits=-1, round_mode="half_up") == \
        ("ArrowInvalid", "Rounding -32768 down to multiples of 10 would overflow")
    assert error_of("round", to_device(pa.array([127, 5], pa.int8())), ndigits=-1, round_mode="up") == \
        ("ArrowInvalid", "Rounding 127 up to multiple of 10 would overflow")          # (8-bit: numbers, where the reference prints characters)
    assert both("round", pa.array([1, 2], pa.int8()), ndigits=-3) == ("ArrowInvalid", "Rounding to -3 digits is out of range for type int8")
    for m in (0, -2):
        assert both("round_to_multiple", pa.array([1.5, 2.5]), multiple=m) == ("ArrowInvalid", "Rounding multiple must be positive")
        assert both("round_to_multiple", pa.array([1, 2], pa.uint16()), multiple=m) == ("ArrowInvalid", "Rounding multiple must be positive")
    assert both("round_to_multiple", pa.array([1, 2], pa.int8()), multiple=pa.scalar(None, pa.int8())) == \
        ("ArrowInvalid", "Rounding multiple must be non-null and valid")
    assert both("round_to_multiple", pa.array([1, 2], pa.int8()), multiple=300)[1] == "Integer value 300 not in range: -128 to 127"
    assert both("round_to_multiple", pa.array([1, 2], pa.int8()), multiple=2.5)[1] == "Float value 2.500000 was truncated converting to int8"
    kind, text = error_of("round_to_multiple", to_device(pa.array([1, 2], pa.int8())), multiple=64, round_mode="half_up")
    assert kind == "ArrowNotImplementedError" and "arrow_amd" in text and "round_to_multiple" in text and "int8" in text and "64" in text, text
    assert to_host(pc.round_to_multiple(to_device(pa.array([1, 70], pa.int8())), multiple=64, round_mode="down")).to_pylist() == [0, 64]
    # ---- refused with a Status, not read by a CPU kernel
    gpu_before = calls("unary_arith", 1), calls("round", 1)
    dec = to_device(pa.array([1, -2, None], pa.int64()).cast(pa.decimal128(25, 2)))
    for f, call in (("round_binary", lambda: pc.round_binary(device["double"], device["int32"])), ("abs", lambda: pc.abs(dec)),
                    ("round", lambda: pc.round(dec, 1)), ("negate", lambda: pc.negate(dec))):
        try:
            call()
            raise SystemExit(f"{f}: a device array was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and f in str(e), (f, e)
    for f, arr in (("negate_checked", device["uint8"]), ("negate", to_device(pa.array([True, False])))):
        try:
            getattr(pc, f)(arr)
            raise SystemExit(f"{f}: accepted a type it has no kernel for")
        except pa.ArrowNotImplementedError as e:
            assert "has no kernel matching input types" in str(e), (f, e)
    assert gpu_before == (calls("unary_arith", 1), calls("round", 1))
    # ---- Acero: table_source_rocm -> project(round(abs(v) * 0.37, 2), sign(v), -v) -> aggregate_rocm equals the host plan
    g0 = calls("unary_arith", 1), calls("round", 1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=-(-n // 3))])
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by([("s", "ascending")])
    assert got_plan.equals(want_plan), (got_plan, want_plan)
    assert calls("unary_arith", 1) - g0[0] >= 3 and calls("round", 1) - g0[1] >= 1
    print("UNARY_ARITH_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + UNARY_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_unary_arith_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.02)
    assert r.returncode == 0 and "UNARY_ARITH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_unary_arith_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "UNARY_ARITH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
