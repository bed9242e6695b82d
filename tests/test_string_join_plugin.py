"""pc.binary_join_element_wise through the Arrow registration shim (plugin/string_join.inc) on device-resident arrays.

The script runs in a fresh interpreter, like tests/test_string_replace_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the
CPU tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  utf8, binary and their large forms,
the three null_handling modes, slices 0 and 7, a literal and a column separator: the device-resident call equals the same
call on the host copies, leaves its result in HBM at offset 0 (without a bitmap when no row is null) and raises the shim's
GPU counter of binary_join_element_wise by exactly one.  Host arrays and all-scalar calls keep the reference's kernels and
results.  A call that mixes host and device columns, a device call with one operand more than the cap, binary_join on a
device list column and binary_repeat on a device column are a Status that names the function, with the GPU counters
unchanged, and the host results of those two siblings are what they were before registration.  An Acero plan
table_source_rocm -> project(binary_join_element_wise(a, b, " ")) -> aggregate_rocm equals the host plan.

Under "skip" the device keeps a row whose values are all null as the empty string, where pyarrow 25.0.0 drops the row
(tests/test_string_join.py): the columns here hold no such row, and the script asserts it."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRING_JOIN_SCRIPT = textwrap.dedent(r'''
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
    rng = np.random.default_rng(61)
    n = SC(50_000)
    F = "binary_join_element_wise"
    CAP = 32
    pool = ["", "a", "ab", "héllo wörld", "q" * 15, "q" * 16, "q" * 17, "0123456789abcdefg" * 3, "x" * 65, "日本語", "a\0b", "-"]
    TYPES = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
    is_bin = lambda t: pa.types.is_binary(t) or pa.types.is_large_binary(t)
    mask_a = rng.random(n) < 0.1
    mask_b = (rng.random(n) < 0.1) & ~mask_a                       # no row has every value null: the reference stays well-formed
    def column(t, mask):
        return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask).cast(t)
    cols = {str(t): (column(t, mask_a), column(t, mask_b), column(t, rng.random(n) < 0.05)) for t in TYPES}
    plain = {str(t): (column(t, None), column(t, None)) for t in TYPES}
    MODES = [("emit_null", ""), ("skip", ""), ("replace", "NA"), ("replace", "x" * 1025)]
    def call(a, b, sep, mode, t):
        null_handling, rep = mode
        if not isinstance(sep, pa.Array):
            sep = pa.scalar(sep.encode() if is_bin(t) else sep, t)
        return pc.binary_join_element_wise(a, b, sep, null_handling=null_handling, null_replacement=rep.encode() if is_bin(t) else rep)
    cases = [(mode, str(t), sl, sep) for mode in MODES for t in TYPES for sl in (0, 7) for sep in ("lit", "col")]
    def host_case(mode, t, sl, sep, source=cols):
        a, b, s = (c.slice(sl) for c in source[t])
        if source is cols:
            assert not pc.any(pc.and_(pc.is_null(a), pc.is_null(b))).as_py()
        return call(a, b, s if sep == "col" else ", ", mode, TYPES[[str(x) for x in TYPES].index(t)])
    want = {c: host_case(*c) for c in cases}
    want_plain = {(mode, str(t)): call(*plain[str(t)], "-", mode, t) for mode in MODES for t in TYPES}
    # the guarded siblings without a device kernel: the same host calls before and after registration
    lists = pa.array([["a", "b"], None, [], ["c", None], ["d"]], pa.list_(pa.string()))
    want_join = pc.binary_join(lists, "-")
    want_repeat = pc.binary_repeat(cols["string"][0], 3)
    want_plus = pc.binary_join_element_wise(cols["string"][0], cols["string"][1], "+", null_handling="skip")
    want_wide = pc.binary_join_element_wise(*([cols["string"][0]] * (CAP - 1)), "")

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
    assert calls(F, 1) == 0 and calls(F, 0) == 0
    # ---- device-resident arrays: equal to the reference on the host copies, results in HBM, one GPU count per call
    device = {t: tuple(to_device(c) for c in cs) for t, cs in cols.items()}
    device_plain = {t: tuple(to_device(c) for c in cs) for t, cs in plain.items()}
    done = 0
    for c in cases:
        g0 = calls(F, 1)
        got = host_case(*c, source=device)
        assert calls(F, 1) == g0 + 1, c
        done += 1
        w = want[c]
        assert all(b is None or not b.is_cpu for b in got.buffers()) and got.buffers()[1] is not None, c
        assert got.type == w.type and got.offset == 0, (c, got.type, w.type)
        h = to_host(got)
        assert h.equals(w) and h.null_count == w.null_count, c
        assert (got.buffers()[0] is None) == (w.null_count == 0), c
    for (mode, t), w in want_plain.items():
        g0 = calls(F, 1)
        got = call(*device_plain[t], "-", mode, w.type)
        assert calls(F, 1) == g0 + 1, (mode, t)
        assert got.buffers()[0] is None and not got.buffers()[1].is_cpu, (mode, t)      # no null row, no bitmap
        h = to_host(got)
        assert h.equals(w) and h.null_count == 0, (mode, t)
    # a null scalar separator: every row null; a null scalar value under skip: left out
    t = "string"
    got = to_host(pc.binary_join_element_wise(device[t][0], device[t][1], pa.scalar(None, pa.string()), null_handling="skip"))
    assert got.null_count == n and got.equals(pa.array([None] * n, pa.string()))
    got = to_host(pc.binary_join_element_wise(device[t][0], pa.scalar(None, pa.string()), device[t][1], "+", null_handling="skip"))
    assert got.equals(want_plus)
    assert calls(F, 0) == 0
    # ---- host arrays and all-scalar calls keep the reference's kernels and results; the stock counter rises
    for c in cases:
        s0 = calls(F, 0)
        got = host_case(*c)
        assert got.equals(want[c]) and got.null_count == want[c].null_count, c
        assert calls(F, 0) == s0 + 1, c
    s0 = calls(F, 0)
    assert pc.binary_join_element_wise("a", "b", "-").as_py() == "a-b"
    assert pc.binary_join_element_wise(pa.scalar("a"), pa.scalar(None, pa.string()), "-", null_handling="replace", null_replacement="NA").as_py() == "a-NA"
    assert pc.binary_join_element_wise(pa.scalar(b"a", pa.large_binary()), pa.scalar(None, pa.large_binary()), pa.scalar(b"-", pa.large_binary())).as_py() is None
    assert calls(F, 0) == s0 + 3
    gpu_before = calls(F, 1)
    # ---- refused with a Status that names the function, not read by a CPU kernel
    a, b, s = device["string"]
    try:
        pc.binary_join_element_wise(a, cols["string"][1], "-")
        raise SystemExit("a mix of host and device columns was accepted")
    except pa.ArrowNotImplementedError as e:
        assert "arrow_amd" in str(e) and F in str(e) and "host and device-resident columns" in str(e), e
    try:
        pc.binary_join_element_wise(cols["string"][0], b, s)
        raise SystemExit("a mix of host and device columns was accepted")
    except pa.ArrowNotImplementedError as e:
        assert "arrow_amd" in str(e) and F in str(e), e
    assert to_host(pc.binary_join_element_wise(*([a] * (CAP - 1)), "")).equals(want_wide)
    gpu_before += 1
    try:
        pc.binary_join_element_wise(*([a] * CAP), "")
        raise SystemExit("one operand more than the cap was accepted")
    except pa.ArrowNotImplementedError as e:
        assert "arrow_amd" in str(e) and F in str(e) and str(CAP + 1) in str(e) and str(CAP) in str(e), e
    assert pc.binary_join_element_wise(*([cols["string"][0]] * CAP), "").null_count == cols["string"][0].null_count     # (the host takes any count)
    dlists = to_device(lists)
    try:
        pc.binary_join(dlists, "-")
        raise SystemExit("binary_join: a device list column was accepted")
    except pa.ArrowNotImplementedError as e:
        assert "arrow_amd" in str(e) and "device-resident" in str(e) and "binary_join " in str(e), e
    for t in ("string", "large_binary"):
        try:
            pc.binary_repeat(device[t][0], 3)
            raise SystemExit("binary_repeat: a device column was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and "binary_repeat" in str(e), e
    assert calls(F, 1) == gpu_before and calls("binary_join", 1) == -1 and calls("binary_repeat", 1) == -1
    # ---- the guarded siblings' host results are what they were before registration
    assert pc.binary_join(lists, "-").equals(want_join) and pc.binary_repeat(cols["string"][0], 3).equals(want_repeat)
    # ---- Acero: table_source_rocm -> project(binary_join_element_wise(a, b, " "), x) -> aggregate_rocm (hash_sum by the joined key)
    first, last = ["ada", "bo", "cy", "", "日本"], ["x", "yy", "", "zé"]
    ta = pa.array([first[i] for i in rng.integers(0, len(first), n)], pa.string(), mask=rng.random(n) < 0.05)
    tb = pa.array([last[i] for i in rng.integers(0, len(last), n)], pa.string(), mask=rng.random(n) < 0.05)
    x = pa.array(rng.integers(-100, 100, n), pa.int64(), mask=rng.random(n) < 0.05)
    table = pa.table({"a": ta, "b": tb, "x": x})
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("project", acero.ProjectNodeOptions([pc.binary_join_element_wise(pc.field("a"), pc.field("b"), " "), pc.field("x")], ["p", "x"])),
            acero.Declaration("aggregate_rocm" if source == "table_source_rocm" else "aggregate",
                              acero.AggregateNodeOptions([("x", "hash_sum", None, "t")], keys=["p"]))])
    want_plan = plan("table_source", table).to_table(use_threads=False).sort_by([("p", "ascending")])
    assert want_plan.num_rows >= 10
    g0 = calls(F, 1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=-(-n // 3))])
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by([("p", "ascending")])
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls(F, 1) - g0 >= 1
    print("STRING_JOIN_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + STRING_JOIN_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_string_join_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.02)
    assert r.returncode == 0 and "STRING_JOIN_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_string_join_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "STRING_JOIN_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
