"""pc.if_else through the Arrow registration shim (plugin/if_else.inc) on device-resident arrays.

The script runs in a fresh interpreter, like the rows of tests/plugin_scripts.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the
CPU tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  Device-resident calls must equal
the same calls on the host copies, leave their results in HBM (without a bitmap where nothing can be null) and raise the
shim's GPU counter once each; host arrays and scalars keep the reference's kernels, implicit casts included; device
arrays of a type without a device kernel, a mix of host and device arrays and a scalar cond over device operands are
refused with a Status; an Acero plan table_source_rocm -> project(if_else) -> aggregate_rocm equals the host plan."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IF_ELSE_SCRIPT = textwrap.dedent(r'''
    import ctypes, decimal, os, sys, faulthandler
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
    rng = np.random.default_rng(41)
    n = SC(100_000)
    def column(t, null_p=0.1):
        mask = (rng.random(n) < null_p) if null_p else None
        if pa.types.is_boolean(t):
            return pa.array(rng.random(n) < 0.5, t, mask=mask)
        if pa.types.is_floating(t):
            return pa.array(rng.standard_normal(n), pa.float64(), mask=mask).cast(t)
        if pa.types.is_decimal(t):
            return pa.array([decimal.Decimal(int(v)).scaleb(-3) for v in rng.integers(-10**15, 10**15, n)], t, mask=mask)
        if pa.types.is_integer(t):
            info = np.iinfo(t.to_pandas_dtype())
            return pa.array(rng.integers(info.min, info.max, n, dtype=t.to_pandas_dtype(), endpoint=True), t, mask=mask)
        width = t.bit_width
        ints = rng.integers(0, 86_000 if width == 32 else 2**40, n, dtype=np.int32 if width == 32 else np.int64)
        return pa.array(ints, pa.int32() if width == 32 else pa.int64(), mask=mask).view(t)
    TYPES = [pa.bool_(), pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64(), pa.float32(),
             pa.float64(), pa.date32(), pa.date64(), pa.time32("ms"), pa.time64("ns"), pa.timestamp("us", tz="UTC"), pa.duration("ms"),
             pa.decimal128(20, 3)]
    def scalar_of(t):
        if pa.types.is_boolean(t):
            return pa.scalar(True, t)
        if pa.types.is_decimal(t):
            return pa.scalar(decimal.Decimal("-12345.678"), t)
        if pa.types.is_floating(t):
            return pa.scalar(2.5, t)
        if pa.types.is_integer(t):
            return pa.scalar(77, t)
        return pa.array([77], pa.int32() if t.bit_width == 32 else pa.int64()).view(t)[0]      # (temporal: a typed scalar)
    cond = column(pa.bool_())
    cond_plain = column(pa.bool_(), 0.0)
    # (name) -> (cond, left, right); arrays are moved to the device below, scalars stay scalars
    cases = {}
    for t in TYPES:
        a, b = column(t), column(t)
        cases[f"{t} array/array"] = (cond, a, b)
        if t in (pa.int16(), pa.int64(), pa.bool_(), pa.decimal128(20, 3), pa.timestamp("us", tz="UTC"), pa.float32()):
            s = scalar_of(t)
            cases[f"{t} array/scalar"] = (cond, a, s)
            cases[f"{t} scalar/array"] = (cond, s, b)
            cases[f"{t} null scalar/array"] = (cond, pa.scalar(None, t), b)
            cases[f"{t} array/null scalar"] = (cond, a, pa.scalar(None, t))
            cases[f"{t} no nulls"] = (cond_plain, column(t, 0.0), s)
            cases[f"{t} no nulls array/array"] = (cond_plain, column(t, 0.0), column(t, 0.0))
    cut = lambda x, sl: x.slice(sl) if isinstance(x, pa.Array) else x
    want = {(name, sl): pc.if_else(*[cut(x, sl) for x in args]) for name, args in cases.items() for sl in (0, 7)}
    ints32, floats = column(pa.int32()), column(pa.float64())
    want_promoted = pc.if_else(cond, ints32, floats)
    want_scalar_cond = pc.if_else(pa.scalar(True), ints32, pa.scalar(5, pa.int32()))
    strings = pa.array([None if i % 7 == 0 else f"s{i % 13}" for i in range(n)], pa.string())
    want_strings = pc.if_else(cond, strings, "else")
    k = pa.array(rng.integers(0, 50, n).astype(np.int32))
    v = pa.array(rng.integers(-100, 100, n), pa.int64(), mask=rng.random(n) < 0.05)
    table = pa.table({"k": k, "v": v})
    def plan(source, t):
        clip = pc.if_else(pc.greater(pc.field("v"), pc.scalar(pa.scalar(0, pa.int64()))), pc.field("v"), pc.scalar(pa.scalar(0, pa.int64())))
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("project", acero.ProjectNodeOptions([pc.field("k"), clip], ["k", "c"])),
            acero.Declaration("aggregate_rocm" if source == "table_source_rocm" else "aggregate",
                              acero.AggregateNodeOptions([("c", "hash_sum", None, "s"), ("c", "hash_count", None, "n")], keys=["k"]))])
    want_plan = plan("table_source", table).to_table(use_threads=False).sort_by("k")

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

    calls = lambda gpu: lib.arrow_amd_plugin_calls(b"if_else", gpu)
    assert calls(1) == 0 and calls(0) == 0
    # ---- device-resident arrays: equal to the reference on the host copies, results in HBM, one GPU count per call
    done = 0
    for name, args in cases.items():
        dargs = [to_device(x) if isinstance(x, pa.Array) else x for x in args]
        for sl in (0, 7):
            got = pc.if_else(*[cut(x, sl) for x in dargs])
            done += 1
            assert got.buffers()[1] is not None and not got.buffers()[1].is_cpu, name
            w = want[name, sl]
            assert got.type == w.type and got.offset == 0, (name, got.type, w.type)
            if "no nulls" in name:
                assert got.buffers()[0] is None, name      # cannot have nulls: no bitmap
            h = to_host(got)
            assert h.equals(w) and h.null_count == w.null_count, (name, sl)
    assert calls(1) == done, (calls(1), done)
    assert calls(0) == 0
    # ---- host arrays and scalars keep the reference's kernels and results, implicit casts included
    for name, args in cases.items():
        assert pc.if_else(*[cut(x, 7) for x in args]).equals(want[name, 7]), name
    assert pc.if_else(cond, ints32, floats).equals(want_promoted) and want_promoted.type == pa.float64()
    assert pc.if_else(pa.scalar(True), ints32, pa.scalar(5, pa.int32())).equals(want_scalar_cond)
    assert pc.if_else(pa.scalar(True), pa.scalar(1), pa.scalar(2)).as_py() == 1
    assert pc.if_else(cond, strings, "else").equals(want_strings)
    assert calls(0) >= len(cases) + 3, calls(0)
    assert calls(1) == done
    # ---- refused with a Status, not read by a CPU kernel
    dcond, dints, dstrings = to_device(cond), to_device(ints32), to_device(strings)
    refused = {"device utf8 left": lambda: pc.if_else(dcond, dstrings, "else"),
               "device utf8 right": lambda: pc.if_else(dcond, "then", dstrings),
               "device utf8 both": lambda: pc.if_else(dcond, dstrings, dstrings),
               "host cond, device values": lambda: pc.if_else(cond, dints, dints),
               "device cond, host values": lambda: pc.if_else(dcond, ints32, ints32),
               "device cond, device / host values": lambda: pc.if_else(dcond, dints, ints32),
               "scalar cond, device values": lambda: pc.if_else(pa.scalar(True), dints, dints),
               "scalar cond, device / scalar": lambda: pc.if_else(pa.scalar(False), dints, pa.scalar(1, pa.int32()))}
    for name, f in refused.items():
        try:
            f()
            raise SystemExit(f"if_else: {name} was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and "if_else" in str(e), (name, e)
    assert calls(1) == done
    # ---- Acero: table_source_rocm -> project(k, if_else(v > 0, v, 0)) -> aggregate_rocm over a device table equals the host plan
    g0 = calls(1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=-(-n // 3))])
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by("k")
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls(1) - g0 >= 3, calls(1) - g0
    print("IF_ELSE_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + IF_ELSE_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_if_else_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.01)
    assert r.returncode == 0 and "IF_ELSE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_if_else_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "IF_ELSE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
