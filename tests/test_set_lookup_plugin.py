"""pc.is_in / pc.index_in through the Arrow registration shim (plugin/set_lookup.inc) on device-resident arrays.

The script runs in a fresh interpreter, like the rows of tests/plugin_scripts.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the
CPU tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  Device-resident calls must equal
the same calls on the host copies and raise the shim's GPU counters; host arrays keep the reference's kernels; an Acero
plan table_source_rocm -> filter(isin) -> aggregate_rocm equals the host plan; dictionary, fixed_size_binary and
decimal256 inputs are refused with a Status instead of reaching a CPU kernel."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SET_LOOKUP_SCRIPT = textwrap.dedent(r'''
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
    rng = np.random.default_rng(23)
    n = SC(1_000_000)

    def col(typ, card, null_p):
        mask = (rng.random(n) < null_p) if null_p else None
        if pa.types.is_boolean(typ):
            return pa.array(rng.random(n) < 0.5, mask=mask)
        if pa.types.is_string(typ) or pa.types.is_large_string(typ) or pa.types.is_binary(typ):
            pool = ["", "a", "b" * 20] + [f"v{i}" * (1 + i % 4) for i in range(card)]
            return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask).cast(typ)
        if pa.types.is_decimal(typ):
            pool = [decimal.Decimal(int(x)).scaleb(-3) for x in rng.integers(-10**15, 10**15, card)]
            return pa.array([pool[i] for i in rng.integers(0, card, n)], typ, mask=mask)
        if pa.types.is_floating(typ):
            pool = rng.standard_normal(card)
            pool[:3] = [0.0, -0.0, np.nan]
            return pa.array(pool[rng.integers(0, card, n)], typ, mask=mask)
        raw = rng.integers(0, 250, card)[rng.integers(0, card, n)]
        if pa.types.is_date32(typ):
            return pa.array(raw.astype(np.int32), mask=mask).view(typ)
        return pa.array(raw, mask=mask).cast(typ)

    cases = {"i64": (col(pa.int64(), 500, 0.05), 16), "i32": (col(pa.int32(), 500, 0.0), 300),
             "u8": (col(pa.uint8(), 200, 0.1), 5), "f64": (col(pa.float64(), 300, 0.1), 40),
             "bool": (col(pa.bool_(), 2, 0.1), 2), "ts": (col(pa.timestamp("us"), 500, 0.1), 20),
             "ts_s": (col(pa.timestamp("s"), 500, 0.1), 20), "d32": (col(pa.date32(), 500, 0.0), 9),
             "dec": (col(pa.decimal128(20, 3), 300, 0.05), 30), "utf8": (col(pa.string(), 300, 0.05), 25),
             "large": (col(pa.large_string(), 300, 0.05), 25), "bin": (col(pa.binary(), 300, 0.0), 10)}
    sets = {}
    for name, (a, m) in cases.items():
        vs = a.take(pa.array(rng.integers(0, len(a), m)))
        sets[name] = pa.concat_arrays([vs, pa.array([None], a.type)]) if name != "bin" else vs
    want = {}
    for name, (a, _) in cases.items():
        for skip in (False, True):
            for sl in (0, 7):
                x = a.slice(sl)
                want[name, skip, sl] = (pc.is_in(x, value_set=sets[name], skip_nulls=skip),
                                        pc.index_in(x, value_set=sets[name], skip_nulls=skip))
    i8 = pa.array([1, 2, 3], pa.int8())
    res_sets = (pa.array([300]), pa.array([1.5, 2.0]), pa.array(["1"]))
    want_res = [(pc.is_in(i8, value_set=v), pc.index_in(i8, value_set=v)) for v in res_sets]
    s_large = pa.array(["a", "bb", None, ""])
    want_large_set = pc.index_in(s_large, value_set=pa.array(["bb", "", None], pa.large_string()))
    chunked_set = pa.chunked_array([sets["i64"].slice(0, 5), sets["i64"].slice(5)])
    want_chunked = pc.index_in(cases["i64"][0], value_set=chunked_set)
    table = pa.table({"k": pa.array(rng.integers(0, 50, n).astype(np.int32)), "v": pa.array(rng.integers(-100, 100, n)),
                      "x": cases["i64"][0]})
    in_list = [int(v) for v in sets["i64"].drop_null().to_pylist()]
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("filter", acero.FilterNodeOptions(pc.field("x").isin(in_list))),
            acero.Declaration("aggregate_rocm" if source == "table_source_rocm" else "aggregate",
                              acero.AggregateNodeOptions([("v", "hash_sum", None, "s"), ("v", "hash_count", None, "c")], keys=["k"]))])
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

    def on_device(arr):
        return arr.buffers()[1] is not None and not arr.buffers()[1].is_cpu

    calls = lambda f, gpu: lib.arrow_amd_plugin_calls(f.encode(), gpu)
    # ---- device-resident arrays: equal to the reference on the host copies, results in HBM, the GPU counters raised
    gpu0 = {f: calls(f, 1) for f in ("is_in", "index_in")}
    done = 0
    for name, (a, _) in cases.items():
        d = to_device(a)
        for skip in (False, True):
            for sl in (0, 7):
                x = d.slice(sl)
                got_is = pc.is_in(x, value_set=sets[name], skip_nulls=skip)
                got_idx = pc.index_in(x, value_set=sets[name], skip_nulls=skip)
                assert on_device(got_is) and on_device(got_idx), name
                w_is, w_idx = want[name, skip, sl]
                assert to_host(got_is).equals(w_is), (name, skip, sl)
                h_idx = to_host(got_idx)
                assert h_idx.equals(w_idx) and h_idx.null_count == w_idx.null_count, (name, skip, sl)
                done += 1
    for f in ("is_in", "index_in"):
        assert calls(f, 1) - gpu0[f] == done, (f, done, calls(f, 1) - gpu0[f])
    # ---- host arrays keep the reference's kernels and results, every type of the cases
    stock0 = {f: calls(f, 0) for f in ("is_in", "index_in")}
    for name, (a, _) in cases.items():
        assert pc.is_in(a.slice(7), value_set=sets[name], skip_nulls=True).equals(want[name, True, 7][0]), name
        assert pc.index_in(a, value_set=sets[name]).equals(want[name, False, 0][1]), name
    for f in ("is_in", "index_in"):
        assert calls(f, 0) - stock0[f] == len(cases), (f, calls(f, 0) - stock0[f])
    # ---- type resolution (the set cast to the input, or the input cast on the device), a large_string set, a chunked set
    d8 = to_device(i8)
    for v, (w_is, w_idx) in zip(res_sets, want_res):
        assert to_host(pc.is_in(d8, value_set=v)).equals(w_is), v
        assert to_host(pc.index_in(d8, value_set=v)).equals(w_idx), v
    assert to_host(pc.index_in(to_device(s_large), value_set=pa.array(["bb", "", None], pa.large_string()))).equals(want_large_set)
    assert to_host(pc.index_in(to_device(cases["i64"][0]), value_set=chunked_set)).equals(want_chunked)
    try:
        pc.is_in(to_device(pa.array([1, 2], pa.int32())), value_set=pa.array([1], pa.timestamp("s")))
        raise SystemExit("int32 against a timestamp set was accepted")
    except pa.ArrowTypeError:
        pass
    # ---- Acero: table_source_rocm -> filter(x.isin(...)) -> aggregate_rocm over a device table equals the host plan
    g0 = calls("is_in", 1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=max(64, n // 3))])
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by("k")
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls("is_in", 1) - g0 >= 3, calls("is_in", 1) - g0
    # ---- types without a device kernel: a Status, not a crash
    dic = pa.DictionaryArray.from_arrays(to_device(pa.array([0, 1, 0, None], pa.int32())), to_device(pa.array(["a", "b"])), safe=False)
    refused = [(dic, pa.array(["a"])),
               (to_device(pa.array([b"ab", None], pa.binary(2))), pa.array([b"ab"], pa.binary(2))),
               (to_device(pa.array([decimal.Decimal("1.5"), None], pa.decimal256(40, 2))),
                pa.array([decimal.Decimal("1.5")], pa.decimal256(40, 2)))]
    for arr, vs in refused:
        for fn in (pc.is_in, pc.index_in):
            try:
                fn(arr, value_set=vs)
                raise SystemExit(f"a device-resident {arr.type} array was accepted")
            except pa.ArrowNotImplementedError as e:
                assert "arrow_amd" in str(e) and "device-resident" in str(e), e
    print("SET_LOOKUP_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + SET_LOOKUP_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_set_lookup_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.01)
    assert r.returncode == 0 and "SET_LOOKUP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_set_lookup_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "SET_LOOKUP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
