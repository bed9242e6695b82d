"""pc.binary_length / utf8_length / binary_slice / utf8_slice_codeunits through the Arrow registration shim
(plugin/string_slice.inc) on device-resident arrays.

The script runs in a fresh interpreter, like tests/test_temporal_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the CPU
tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  Every function on every input type of
its list, at slice 0 and at slice 7: the device-resident call equals the same call on the host copy, leaves its result in
HBM (without a bitmap when the input has none) and raises the shim's GPU counter of that function by exactly one.  Host
arrays keep the reference's kernels and results, step=2 and step=-1 included.  On a device array step=2,
fixed_size_binary and each guarded sibling (replace_slice, reverse, case mapping) are a Status that names the function;
the siblings' host results are what they were before registration.  An Acero plan table_source_rocm -> filter(utf8_length)
-> project(utf8_slice_codeunits) -> aggregate_rocm equals the host plan."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRING_SLICE_SCRIPT = textwrap.dedent(r'''
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
    pool = ["", "a", "héllo wörld", "日本語テキスト", "x" * 15, "y" * 16, "z" * 17, "aé日😀" * 3, "q" * 13 + "😀" + "r" * 20, "abc", "0123456789" * 7]
    def column(t, null_p=0.1):
        mask = (rng.random(n) < null_p) if null_p else None
        return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask).cast(t)
    UTF8, BINARY = [pa.string(), pa.large_string()], [pa.binary(), pa.large_binary()]
    columns = {str(t): column(t) for t in UTF8 + BINARY}
    plain = {str(t): column(t, 0.0) for t in (pa.string(), pa.large_binary())}
    # (function, arguments) on every input type of its list; binary_slice with a stop: the reference's own kernel fails
    # on start >= 0 without one
    CALLS = [("binary_length", (), UTF8 + BINARY), ("utf8_length", (), UTF8),
             ("binary_slice", (1, 7), BINARY), ("binary_slice", (-5, None), BINARY), ("binary_slice", (2, -1), BINARY),
             ("utf8_slice_codeunits", (0, 2), UTF8), ("utf8_slice_codeunits", (1, None), UTF8), ("utf8_slice_codeunits", (-3, None), UTF8),
             ("utf8_slice_codeunits", (5, -2), UTF8)]
    FUNCTIONS = ["binary_length", "utf8_length", "binary_slice", "utf8_slice_codeunits"]
    pairs = [(f, args, str(t)) for f, args, types in CALLS for t in types]
    want = {(f, args, t, sl): getattr(pc, f)(columns[t].slice(sl), *args) for f, args, t in pairs for sl in (0, 7)}
    want_plain = {(f, args, t): getattr(pc, f)(plain[t], *args) for f, args, t in pairs if t in plain}
    want_steps = {(f, t, step): getattr(pc, f)(columns[t].slice(7), 0, 9, step) for f, t in
                  (("binary_slice", "binary"), ("binary_slice", "large_binary"), ("utf8_slice_codeunits", "string"),
                   ("utf8_slice_codeunits", "large_string")) for step in (2, -1)}
    # the guarded siblings without a device kernel: the same host calls before and after registration
    siblings = {"binary_replace_slice": (lambda a: pc.binary_replace_slice(a, 1, 3, b"XY"), "binary"),
                "utf8_replace_slice": (lambda a: pc.utf8_replace_slice(a, 1, 3, "XY"), "string"),
                "binary_reverse": (lambda a: pc.binary_reverse(a), "binary"), "utf8_reverse": (lambda a: pc.utf8_reverse(a), "string"),
                "ascii_reverse": (lambda a: pc.ascii_reverse(a), "string"), "utf8_upper": (lambda a: pc.utf8_upper(a), "string"),
                "utf8_lower": (lambda a: pc.utf8_lower(a), "string"), "ascii_upper": (lambda a: pc.ascii_upper(a), "string"),
                "ascii_lower": (lambda a: pc.ascii_lower(a), "string")}
    def outcome(f, arr):
        # the result, or the reference's own error (ascii_reverse refuses non-ASCII rows)
        try:
            return f(arr)
        except pa.ArrowException as e:
            return f"{type(e).__name__}: {e}"
    same = lambda x, y: x == y if isinstance(x, str) or isinstance(y, str) else x.equals(y)
    want_siblings = {name: outcome(f, columns[t]) for name, (f, t) in siblings.items()}
    assert sum(isinstance(w, str) for w in want_siblings.values()) <= 1, want_siblings
    fsb = pa.array([b"abcd", None, b"wxyz"] * 30, pa.binary(4))
    want_fsb = pc.binary_length(fsb), pc.binary_slice(fsb, 1, 3)
    # the Acero plan: hash_sum(x) by the first two codepoints of s, over the rows whose s has more than k codepoints
    keys = ["ab" + "c" * int(k) for k in range(9)] + ["é日本", "éa", "日", "", "😀😀😀😀"]
    s = pa.array([keys[i] for i in rng.integers(0, len(keys), n)], pa.string(), mask=rng.random(n) < 0.05)
    x = pa.array(rng.integers(-100, 100, n), pa.int64(), mask=rng.random(n) < 0.05)
    table = pa.table({"s": s, "x": x})
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("filter", acero.FilterNodeOptions(pc.greater(pc.utf8_length(pc.field("s")), pa.scalar(1, pa.int32())))),
            acero.Declaration("project", acero.ProjectNodeOptions([pc.utf8_slice_codeunits(pc.field("s"), 0, 2), pc.field("x")], ["p", "x"])),
            acero.Declaration("aggregate_rocm" if source == "table_source_rocm" else "aggregate",
                              acero.AggregateNodeOptions([("x", "hash_sum", None, "t")], keys=["p"]))])
    want_plan = plan("table_source", table).to_table(use_threads=False).sort_by([("p", "ascending")])
    assert want_plan.num_rows >= 4

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
    for f in FUNCTIONS:
        assert calls(f, 1) == 0 and calls(f, 0) == 0, f
    # ---- device-resident arrays: equal to the reference on the host copies, results in HBM, one GPU count per call
    device = {t: to_device(a) for t, a in columns.items()}
    device_plain = {t: to_device(a) for t, a in plain.items()}
    done = 0
    for f, args, t in pairs:
        for sl in (0, 7):
            g0 = calls(f, 1)
            got = getattr(pc, f)(device[t].slice(sl), *args)
            assert calls(f, 1) == g0 + 1, (f, args, t, sl)
            done += 1
            assert all(b is None or not b.is_cpu for b in got.buffers()) and got.buffers()[1] is not None, (f, t)
            w = want[f, args, t, sl]
            assert got.type == w.type and got.offset == 0, (f, t, got.type, w.type)
            h = to_host(got)
            assert h.equals(w) and h.null_count == w.null_count, (f, args, t, sl)
        if t in plain:
            g0 = calls(f, 1)
            got = getattr(pc, f)(device_plain[t], *args)
            assert calls(f, 1) == g0 + 1, (f, t)
            assert got.buffers()[0] is None and not got.buffers()[1].is_cpu, (f, t)      # no bitmap in, no bitmap out
            h = to_host(got)
            assert h.equals(want_plain[f, args, t]) and h.null_count == 0, (f, args, t)
    assert all(calls(f, 0) == 0 for f in FUNCTIONS)
    # ---- host arrays keep the reference's kernels and results, every step included; the stock counter rises
    for f, args, t in pairs:
        s0 = calls(f, 0)
        got = getattr(pc, f)(columns[t].slice(7), *args)
        assert got.equals(want[f, args, t, 7]) and got.null_count == want[f, args, t, 7].null_count, (f, args, t)
        assert calls(f, 0) == s0 + 1, (f, t)
    for (f, t, step), w in want_steps.items():
        s0 = calls(f, 0)
        assert getattr(pc, f)(columns[t].slice(7), 0, 9, step).equals(w), (f, t, step)
        assert calls(f, 0) == s0 + 1, (f, t, step)
    assert pc.utf8_length(pa.scalar("héllo")).as_py() == 5 and pc.utf8_slice_codeunits(pa.scalar("héllo"), 1, 3).as_py() == "él"
    assert pc.binary_length(fsb).equals(want_fsb[0]) and pc.binary_slice(fsb, 1, 3).equals(want_fsb[1])
    # ---- step: 0 is the reference's error on both paths; any other step but 1 has no device kernel
    gpu_before = {f: calls(f, 1) for f in FUNCTIONS}
    for f, t in (("binary_slice", "binary"), ("utf8_slice_codeunits", "large_string")):
        for arr in (columns[t], device[t]):
            try:
                getattr(pc, f)(arr, 0, 4, 0)
                raise SystemExit(f"{f}: step=0 was accepted")
            except pa.ArrowInvalid as e:
                assert "Slice step cannot be zero" in str(e), e
        for step in (2, -1):
            try:
                getattr(pc, f)(device[t], 0, 9, step)
                raise SystemExit(f"{f}: step={step} on a device array was accepted")
            except pa.ArrowNotImplementedError as e:
                assert "arrow_amd" in str(e) and f in str(e) and f"step={step}" in str(e) and "device-resident" in str(e), (f, e)
    # ---- refused with a Status that names the function, not read by a CPU kernel
    dfsb = to_device(fsb)
    for name, call in (("binary_length", lambda: pc.binary_length(dfsb)), ("binary_slice", lambda: pc.binary_slice(dfsb, 1, 3))):
        try:
            call()
            raise SystemExit(f"{name}: a device fixed_size_binary array was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and name in str(e), (name, e)
    for name, (f, t) in siblings.items():
        try:
            f(device[t])
            raise SystemExit(f"{name}: a device array was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and name in str(e), (name, e)
    for f, arr, args in (("utf8_length", device["binary"], ()), ("binary_slice", device["string"], (0, 2)),
                         ("utf8_slice_codeunits", device["large_binary"], (0, 2))):
        try:
            getattr(pc, f)(arr, *args)
            raise SystemExit(f"{f}: accepted a type it has no kernel for")
        except pa.ArrowNotImplementedError as e:
            assert "has no kernel matching input types" in str(e), (f, e)
    assert gpu_before == {f: calls(f, 1) for f in FUNCTIONS}
    # ---- the guarded siblings' host results are what they were before registration
    for name, (f, t) in siblings.items():
        assert same(outcome(f, columns[t]), want_siblings[name]), name
    # ---- Acero: table_source_rocm -> filter(utf8_length(s) > 1) -> project(utf8_slice_codeunits(s, 0, 2), x) -> aggregate_rocm
    g0 = calls("utf8_length", 1), calls("utf8_slice_codeunits", 1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=-(-n // 3))])
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by([("p", "ascending")])
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls("utf8_length", 1) - g0[0] >= 1 and calls("utf8_slice_codeunits", 1) - g0[1] >= 1
    print("STRING_SLICE_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + STRING_SLICE_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_string_slice_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.02)
    assert r.returncode == 0 and "STRING_SLICE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_string_slice_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "STRING_SLICE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
