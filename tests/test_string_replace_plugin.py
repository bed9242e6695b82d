"""pc.replace_substring through the Arrow registration shim (plugin/string_replace.inc) on device-resident arrays.

The script runs in a fresh interpreter, like tests/test_string_trim_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the
CPU tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  utf8, binary and their large forms,
with nulls and without, at slice 0 and at slice 7, under several (pattern, replacement, max_replacements): the
device-resident call equals the same call on the host copy, leaves its result in HBM at offset 0 (without a bitmap when
the input has none) and raises the shim's GPU counter of replace_substring by exactly one.  Host arrays and scalars keep
the reference's kernels and results.  An empty pattern, replace_substring_regex and a fixed_size_binary on a device array
are a Status that names the function, with the GPU counters unchanged, and replace_substring_regex on host arrays is what
it was before registration.  An Acero plan table_source_rocm -> filter(match_substring) -> project(replace_substring) ->
aggregate_rocm equals the host plan.

The reference is never called with an empty pattern and unlimited replacements: it does not terminate."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRING_REPLACE_SCRIPT = textwrap.dedent(r'''
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
    rng = np.random.default_rng(59)
    n = SC(50_000)
    F = "replace_substring"
    pool = ["", "a", "ab", "aaaa", "aaa", "abababa", "xxabxx", "ab" * 9, "héllo wörld ab", "q" * 15 + "ab", "ab" + "q" * 16,
            "0123456789abcdefg" * 3, "x" * 40, "aabaabaac" + "-" * 30 + "aabaabaac", "日本ab語", "b" + "a" * 33]
    def column(t, null_p=0.1):
        mask = (rng.random(n) < null_p) if null_p else None
        return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask).cast(t)
    TYPES = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
    columns = {str(t): column(t) for t in TYPES}
    plain = {str(t): column(t, 0.0) for t in TYPES}
    TRIPLES = [("ab", "", None), ("aa", "b", -1), ("a", "<a>", 2), ("aabaabaac", "Z", 0), ("0123456789abcdefg", "0123456789abcdefg###", 1),
               ("ab", "x" * 40, -5), ("日本", "に", None)]
    def call(arr, triple, fn=None):
        pattern, rep, cap = triple
        if pa.types.is_binary(arr.type) or pa.types.is_large_binary(arr.type):
            pattern, rep = pattern.encode(), rep.encode()
        return (fn or pc.replace_substring)(arr, pattern, rep, max_replacements=cap)
    pairs = [(tr, str(t)) for tr in TRIPLES for t in TYPES]
    want = {(tr, t, sl): call(columns[t].slice(sl), tr) for tr, t in pairs for sl in (0, 7)}
    want_plain = {(tr, t): call(plain[t], tr) for tr, t in pairs}
    # the guarded sibling without a device kernel: the same host calls before and after registration
    REGEX = [("a+", "<\\0>", None), ("(a)(b)", "\\2\\1", 1), ("x*$", "!", -1)]
    want_regex = {(tr, str(t)): call(columns[str(t)], tr, pc.replace_substring_regex) for tr in REGEX for t in TYPES}
    # the Acero plan: hash_sum(x) by replace_substring(s, "ab", "-"), over the rows whose s holds "ab"
    keys = ["ab" * int(k) for k in range(5)] + ["xaby", "xy", "", "a", "b", "abab-", "-abab", "é日ab"]
    s = pa.array([keys[i] for i in rng.integers(0, len(keys), n)], pa.string(), mask=rng.random(n) < 0.05)
    x = pa.array(rng.integers(-100, 100, n), pa.int64(), mask=rng.random(n) < 0.05)
    table = pa.table({"s": s, "x": x})
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("filter", acero.FilterNodeOptions(pc.match_substring(pc.field("s"), "ab"))),
            acero.Declaration("project", acero.ProjectNodeOptions([pc.replace_substring(pc.field("s"), "ab", "-"), pc.field("x")], ["p", "x"])),
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
    assert calls(F, 1) == 0 and calls(F, 0) == 0
    # ---- device-resident arrays: equal to the reference on the host copies, results in HBM, one GPU count per call
    device = {t: to_device(a) for t, a in columns.items()}
    device_plain = {t: to_device(a) for t, a in plain.items()}
    done = 0
    for tr, t in pairs:
        for sl in (0, 7):
            g0 = calls(F, 1)
            got = call(device[t].slice(sl), tr)
            assert calls(F, 1) == g0 + 1, (tr, t, sl)
            done += 1
            assert all(b is None or not b.is_cpu for b in got.buffers()) and got.buffers()[1] is not None, (tr, t)
            w = want[tr, t, sl]
            assert got.type == w.type and got.offset == 0, (tr, t, got.type, w.type)
            h = to_host(got)
            assert h.equals(w) and h.null_count == w.null_count, (tr, t, sl)
        g0 = calls(F, 1)
        got = call(device_plain[t], tr)
        assert calls(F, 1) == g0 + 1, (tr, t)
        assert got.buffers()[0] is None and not got.buffers()[1].is_cpu, (tr, t)      # no bitmap in, no bitmap out
        h = to_host(got)
        assert h.equals(want_plain[tr, t]) and h.null_count == 0, (tr, t)
    assert calls(F, 0) == 0
    # ---- host arrays and scalars keep the reference's kernels and results; the stock counter rises
    for tr, t in pairs:
        s0 = calls(F, 0)
        got = call(columns[t].slice(7), tr)
        assert got.equals(want[tr, t, 7]) and got.null_count == want[tr, t, 7].null_count, (tr, t)
        assert calls(F, 0) == s0 + 1, (tr, t)
    s0 = calls(F, 0)
    assert pc.replace_substring(pa.scalar("aaaa"), "aa", "b").as_py() == "bb"
    assert pc.replace_substring(pa.scalar(None, pa.large_string()), "x", "y").as_py() is None
    assert pc.replace_substring(pa.scalar("abab"), "", "X", max_replacements=2).as_py() == "XXabab"   # (the host keeps the empty pattern)
    assert calls(F, 0) == s0 + 3
    gpu_before = calls(F, 1)
    # ---- refused with a Status that names the function, not read by a CPU kernel
    for cap in (None, 0, 2):
        for t in ("string", "large_binary"):
            try:
                pc.replace_substring(device[t], "", "x", max_replacements=cap)
                raise SystemExit("an empty pattern on a device array was accepted")
            except pa.ArrowNotImplementedError as e:
                assert "arrow_amd" in str(e) and F in str(e) and "empty pattern" in str(e) and "device-resident" in str(e), e
    for tr in REGEX:
        for t in ("string", "binary", "large_string", "large_binary"):
            try:
                call(device[t], tr, pc.replace_substring_regex)
                raise SystemExit("replace_substring_regex: a device array was accepted")
            except pa.ArrowNotImplementedError as e:
                assert "arrow_amd" in str(e) and "device-resident" in str(e) and "replace_substring_regex" in str(e), e
    dfixed = to_device(pa.array([b"abc", b"aab", None], pa.binary(3)))
    try:
        pc.replace_substring(dfixed, b"a", b"b")
        raise SystemExit("replace_substring: accepted a type it has no kernel for")
    except pa.ArrowNotImplementedError as e:
        assert F in str(e) and "has no kernel matching input types" in str(e), e
    assert calls(F, 1) == gpu_before and calls("replace_substring_regex", 1) == -1
    # ---- the guarded sibling's host results are what they were before registration
    for tr in REGEX:
        for t in TYPES:
            assert call(columns[str(t)], tr, pc.replace_substring_regex).equals(want_regex[tr, str(t)]), (tr, t)
    # ---- Acero: table_source_rocm -> filter(match_substring(s, "ab")) -> project(replace_substring(s, "ab", "-"), x) -> aggregate_rocm
    g0 = calls("match_substring", 1), calls(F, 1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=-(-n // 3))])
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by([("p", "ascending")])
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls("match_substring", 1) - g0[0] >= 1 and calls(F, 1) - g0[1] >= 1
    print("STRING_REPLACE_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + STRING_REPLACE_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_string_replace_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.02)
    assert r.returncode == 0 and "STRING_REPLACE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_string_replace_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "STRING_REPLACE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
