"""pc.equal / not_equal / greater / greater_equal / less / less_equal of utf8 / binary columns through the Arrow
registration shim (plugin/string_compare.inc) on device-resident arrays.

The script runs in a fresh interpreter, like tests/test_string_trim_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the
CPU tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  Six functions x utf8, binary,
large_utf8, large_binary x array-array, array-scalar, scalar-array, with nulls and without, at slice 0 and at slice 7:
the device-resident call equals the same call on the host copies, leaves its result in HBM at offset 0 (without a bitmap
when no input has one) and raises the shim's GPU counter `compare_string` by exactly one.  Host arrays and two scalars keep
the reference's kernels and results and raise the stock counter only.  A host array with a device array is a Status that
names arrow_amd; utf8 with large_utf8 on the device equals the host result or is NotImplemented, never a wrong answer;
fixed_size_binary on the device is still refused by name.  An Acero plan table_source_rocm -> filter((s >= "b") &
(s != "zz")) -> aggregate_rocm equals the host plan."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRING_COMPARE_SCRIPT = textwrap.dedent(r'''
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
    n = SC(20_000)
    pool = ["", "a", "ab", "abc", "b", "a\x00", "é", "ée", "日本", "zz", "z" * 15, "z" * 16, "z" * 17, "z" * 16 + "a", "0123456789" * 7,
            "0123456789" * 7 + "x", "0123456789" * 6 + "012345678"]
    def column(t, null_p):
        mask = (rng.random(n + 7) < null_p) if null_p else None
        return pa.array([pool[i] for i in rng.integers(0, len(pool), n + 7)], pa.string(), mask=mask).cast(t)
    TYPES = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
    FUNCTIONS = ["equal", "not_equal", "greater", "greater_equal", "less", "less_equal"]
    left = {(str(t), p): column(t, p) for t in TYPES for p in (0.1, 0.0)}
    right = {(str(t), p): column(t, p) for t in TYPES for p in (0.1, 0.0)}
    literal = {str(t): pa.scalar("z" * 16, pa.string()).cast(t) for t in TYPES}
    def operands(t, p, sl, form, l=left, r=right):
        """(left, right) of a call: array-array, array-scalar, scalar-array"""
        a, b = l[t, p].slice(sl), r[t, p].slice(sl)
        return {"aa": (a, b), "as": (a, literal[t]), "sa": (literal[t], b)}[form]
    CASES = [(f, str(t), p, sl, form) for f in FUNCTIONS for t in TYPES for p in (0.1, 0.0) for sl in (0, 7) for form in ("aa", "as", "sa")]
    want = {c: getattr(pc, c[0])(*operands(*c[1:])) for c in CASES}
    fsb = pa.array([b"ab", b"cd", None, b"ab"], pa.binary(2))
    want_fsb = pc.equal(fsb, fsb)
    # the Acero plan: hash_sum(x) by k over the rows with s >= "b" and s != "zz"
    keys = ["a", "b", "ba", "zz", "zzz", "é", "", "bb", "az"]
    s = pa.array([keys[i] for i in rng.integers(0, len(keys), n)], pa.string(), mask=rng.random(n) < 0.05)
    k = pa.array(rng.integers(0, 10, n), pa.int32())
    x = pa.array(rng.integers(-100, 100, n), pa.int64(), mask=rng.random(n) < 0.05)
    table = pa.table({"s": s, "k": k, "x": x})
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("filter", acero.FilterNodeOptions((pc.field("s") >= pa.scalar("b")) & (pc.field("s") != pa.scalar("zz")))),
            acero.Declaration("aggregate_rocm" if source == "table_source_rocm" else "aggregate",
                              acero.AggregateNodeOptions([("x", "hash_sum", None, "t")], keys=["k"]))])
    want_plan = plan("table_source", table).to_table(use_threads=False).sort_by([("k", "ascending")])
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

    gpu = lambda: lib.arrow_amd_plugin_calls(b"compare_string", 1)
    stock = lambda: lib.arrow_amd_plugin_calls(b"compare_string", 0)
    others = lambda: [lib.arrow_amd_plugin_calls(name, which) for name in (b"compare", b"greater") for which in (0, 1)]
    assert gpu() == 0 and stock() == 0
    others0 = others()
    # ---- device-resident operands: equal to the reference on the host copies, results in HBM, one GPU count per call
    dleft = {key: to_device(a) for key, a in left.items()}
    dright = {key: to_device(a) for key, a in right.items()}
    done = 0
    for c in CASES:
        f, t, p, sl, form = c
        a, b = operands(t, p, sl, form, dleft, dright)
        g0 = gpu()
        got = getattr(pc, f)(a, b)
        assert gpu() == g0 + 1, c
        done += 1
        assert got.type == pa.bool_() and got.offset == 0, c
        assert got.buffers()[1] is not None and all(buf is None or not buf.is_cpu for buf in got.buffers()), c
        if p == 0.0:
            assert got.buffers()[0] is None, c                  # no bitmap in, no bitmap out
        h, w = to_host(got), want[c]
        assert h.equals(w) and h.null_count == w.null_count, c
    assert stock() == 0
    # a null scalar: every slot null
    for t in TYPES:
        for form in ("as", "sa"):
            null = pa.scalar(None, t)
            g0 = gpu()
            got = pc.less(dleft[str(t), 0.0], null) if form == "as" else pc.less(null, dleft[str(t), 0.0])
            assert gpu() == g0 + 1
            h = to_host(got)
            assert h.null_count == len(h) == n + 7 and not got.buffers()[1].is_cpu, (t, form)
    # ---- host arrays and two scalars keep the reference's kernels and results; only the stock counter rises
    g_before = gpu()
    for c in CASES:
        f, t, p, sl, form = c
        if sl == 0:
            continue
        s0 = stock()
        got = getattr(pc, f)(*operands(t, p, sl, form))
        assert got.equals(want[c]) and got.null_count == want[c].null_count, c
        assert stock() == s0 + 1, c
    for f, a, b, w in (("equal", "a", "a", True), ("less", "a\x00", "ab", True), ("less", "é", "ab", False), ("greater_equal", "a", "ab", False),
                       ("less_equal", "ab", "ab", True), ("not_equal", "", "\x00", True), ("greater", "b", "ab", True)):
        for t in TYPES:
            s0 = stock()
            assert getattr(pc, f)(pa.scalar(a, pa.string()).cast(t), pa.scalar(b, pa.string()).cast(t)).as_py() is w, (f, a, b, t)
            assert stock() == s0 + 1, (f, t)
    assert pc.less(pa.scalar(None, pa.string()), pa.scalar("a")).as_py() is None
    assert gpu() == g_before and others() == others0           # the numeric counters keep their meaning
    assert pc.less(pa.array([1, 2, 3]), pa.scalar(2)).to_pylist() == [True, False, False]
    # ---- one host and one device array: a Status naming arrow_amd, not a read
    for f in FUNCTIONS:
        for a, b in ((left["string", 0.1], dright["string", 0.1]), (dleft["large_binary", 0.0], right["large_binary", 0.0])):
            try:
                getattr(pc, f)(a, b)
                raise SystemExit(f"{f}: a host array with a device array was accepted")
            except pa.ArrowNotImplementedError as e:
                assert "arrow_amd" in str(e) and f in str(e), (f, e)
    # ---- utf8 with large_utf8 on the device (the reference casts implicitly): the host result or NotImplemented
    for f in FUNCTIONS:
        w = getattr(pc, f)(left["string", 0.1], right["large_string", 0.1])
        try:
            got = getattr(pc, f)(dleft["string", 0.1], dright["large_string", 0.1])
        except pa.ArrowNotImplementedError:
            continue
        h = to_host(got) if not got.buffers()[1].is_cpu else got
        assert h.equals(w), f
    # ---- fixed_size_binary: still refused by name on the device, the reference's on the host
    assert pc.equal(fsb, fsb).equals(want_fsb)
    dfsb = to_device(fsb)
    for f in FUNCTIONS:
        try:
            getattr(pc, f)(dfsb, dfsb)
            raise SystemExit(f"{f}: a device fixed_size_binary array was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and f in str(e) and "fixed_size_binary" in str(e), (f, e)
    # ---- Acero: table_source_rocm -> filter((s >= "b") & (s != "zz")) -> aggregate_rocm(hash_sum(x) by k)
    g0 = gpu()
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=-(-n // 3))])
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by([("k", "ascending")])
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert gpu() - g0 >= 6, gpu() - g0
    print("STRING_COMPARE_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + STRING_COMPARE_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_string_compare_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.02)
    assert r.returncode == 0 and "STRING_COMPARE_OK 288" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_string_compare_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "STRING_COMPARE_OK 288" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
