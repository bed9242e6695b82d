"""pc.{ascii,utf8}_{,l,r}trim{,_whitespace} through the Arrow registration shim (plugin/string_trim.inc) on
device-resident arrays.

The script runs in a fresh interpreter, like tests/test_string_slice_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the
CPU tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  All twelve functions on utf8 and
large_utf8, with nulls and without, at slice 0 and at slice 7: the device-resident call equals the same call on the host
copy, leaves its result in HBM at offset 0 (without a bitmap when the input has none) and raises the shim's GPU counter of
that function by exactly one.  Host arrays and scalars keep the reference's kernels and results.  An invalid `characters`
is the reference's Invalid on both paths; 65 distinct codepoints on a device array, a binary device array and each guarded
sibling (padding, swapcase, capitalize, title) are a Status that names the function, and the siblings' host results are what
they were before registration.  An Acero plan table_source_rocm -> filter(binary_length(utf8_trim_whitespace)) ->
project(ascii_rtrim) -> aggregate_rocm equals the host plan."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRING_TRIM_SCRIPT = textwrap.dedent(r'''
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
    rng = np.random.default_rng(53)
    n = SC(50_000)
    MIXED = "xé 　\U0001f600"
    pool = ["", "a", " a ", "\t héllo wörld \n", "　日本語　", " " * 15 + "p", "p" + " " * 16, " " * 17 + "p" + "\t" * 33,
            "xxéqéxx", "\U0001f600 abc \U0001f600", "   ", " " * 40, "\u0085 z \u0085", "\u200b z \u200b", "0123456789" * 7 + " "]
    def column(t, null_p=0.1):
        mask = (rng.random(n) < null_p) if null_p else None
        return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask).cast(t)
    UTF8 = [pa.string(), pa.large_string()]
    columns = {str(t): column(t) for t in UTF8}
    plain = {str(t): column(t, 0.0) for t in UTF8}
    SIDES = ("trim", "ltrim", "rtrim")
    FUNCTIONS = [f"{enc}_{side}{ws}" for enc in ("ascii", "utf8") for side in SIDES for ws in ("_whitespace", "")]
    CALLS = [(f, () if f.endswith("_whitespace") else (MIXED,)) for f in FUNCTIONS] + [("utf8_trim", ("",)), ("ascii_rtrim", (" ",))]
    pairs = [(f, args, str(t)) for f, args in CALLS for t in UTF8]
    want = {(f, args, t, sl): getattr(pc, f)(columns[t].slice(sl), *args) for f, args, t in pairs for sl in (0, 7)}
    want_plain = {(f, args, t): getattr(pc, f)(plain[t], *args) for f, args, t in pairs}
    # the guarded siblings without a device kernel: the same host calls before and after registration
    siblings = {f"{enc}_{f}": (lambda a, name=f"{enc}_{f}": getattr(pc, name)(a, 12, "*")) for enc in ("ascii", "utf8") for f in ("lpad", "rpad", "center")}
    siblings.update({f"{enc}_{f}": (lambda a, name=f"{enc}_{f}": getattr(pc, name)(a)) for enc in ("ascii", "utf8")
                     for f in ("swapcase", "capitalize", "title")})
    assert len(siblings) == 12
    want_siblings = {name: f(columns["string"]) for name, f in siblings.items()}
    # the Acero plan: hash_sum(x) by rtrim(s), over the rows whose s is not all whitespace
    keys = ["ab" + " " * int(k) for k in range(6)] + [" ab  ", "é日 ", "   ", "", "\t\n", "　", "q"]
    s = pa.array([keys[i] for i in rng.integers(0, len(keys), n)], pa.string(), mask=rng.random(n) < 0.05)
    x = pa.array(rng.integers(-100, 100, n), pa.int64(), mask=rng.random(n) < 0.05)
    table = pa.table({"s": s, "x": x})
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("filter", acero.FilterNodeOptions(
                pc.greater(pc.binary_length(pc.utf8_trim_whitespace(pc.field("s"))), pa.scalar(0, pa.int32())))),
            acero.Declaration("project", acero.ProjectNodeOptions([pc.ascii_rtrim(pc.field("s"), " "), pc.field("x")], ["p", "x"])),
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
        g0 = calls(f, 1)
        got = getattr(pc, f)(device_plain[t], *args)
        assert calls(f, 1) == g0 + 1, (f, t)
        assert got.buffers()[0] is None and not got.buffers()[1].is_cpu, (f, t)      # no bitmap in, no bitmap out
        h = to_host(got)
        assert h.equals(want_plain[f, args, t]) and h.null_count == 0, (f, args, t)
    assert all(calls(f, 0) == 0 for f in FUNCTIONS)
    # ---- host arrays and scalars keep the reference's kernels and results; the stock counter rises
    for f, args, t in pairs:
        s0 = calls(f, 0)
        got = getattr(pc, f)(columns[t].slice(7), *args)
        assert got.equals(want[f, args, t, 7]) and got.null_count == want[f, args, t, 7].null_count, (f, args, t)
        assert calls(f, 0) == s0 + 1, (f, t)
    s0 = calls("utf8_trim_whitespace", 0), calls("ascii_ltrim", 0)
    assert pc.utf8_trim_whitespace(pa.scalar("　 hé ")).as_py() == "hé" and pc.ascii_ltrim(pa.scalar("xxaxx"), "x").as_py() == "axx"
    assert pc.utf8_rtrim(pa.scalar(None, pa.large_string()), "x").as_py() is None
    assert (calls("utf8_trim_whitespace", 0), calls("ascii_ltrim", 0)) == (s0[0] + 1, s0[1] + 1)
    gpu_before = {f: calls(f, 1) for f in FUNCTIONS}
    # ---- an invalid `characters`: the reference's Invalid on both paths
    for f in ("utf8_trim", "utf8_ltrim", "utf8_rtrim"):
        for arr in (columns["string"], device["string"], device["large_string"]):
            for bad in (b"\xff", b"x\xc3"):
                try:
                    getattr(pc, f)(arr, bad)
                    raise SystemExit(f"{f}: characters={bad!r} was accepted")
                except pa.ArrowInvalid as e:
                    assert "Invalid UTF8 sequence in input" in str(e), e
    # ---- refused with a Status that names the function, not read by a CPU kernel
    many = "".join(chr(0x100 + i) for i in range(65))
    for f in ("utf8_trim", "utf8_ltrim", "utf8_rtrim"):
        assert getattr(pc, f)(columns["string"], many).equals(columns["string"])         # (the host path has no such bound)
        try:
            getattr(pc, f)(device["string"], many)
            raise SystemExit(f"{f}: 65 distinct codepoints on a device array were accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and f in str(e) and "65 distinct" in str(e) and "device-resident" in str(e), (f, e)
    g0 = calls("utf8_trim", 1)
    assert to_host(pc.utf8_trim(device["string"], many[:64] + many[:9])).equals(columns["string"])   # 64 distinct, with duplicates
    assert calls("utf8_trim", 1) == g0 + 1
    gpu_before["utf8_trim"] += 1
    dbin = to_device(columns["string"].cast(pa.binary()))
    for f, args in CALLS:
        try:
            getattr(pc, f)(dbin, *args)
            raise SystemExit(f"{f}: accepted a type it has no kernel for")
        except pa.ArrowNotImplementedError as e:
            assert "has no kernel matching input types" in str(e), (f, e)
    for name, f in siblings.items():
        try:
            f(device["string"])
            raise SystemExit(f"{name}: a device array was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and name in str(e), (name, e)
    assert gpu_before == {f: calls(f, 1) for f in FUNCTIONS}
    # ---- the guarded siblings' host results are what they were before registration
    for name, f in siblings.items():
        assert f(columns["string"]).equals(want_siblings[name]), name
    # ---- Acero: table_source_rocm -> filter(binary_length(utf8_trim_whitespace(s)) > 0) -> project(ascii_rtrim(s, " "), x) -> aggregate_rocm
    g0 = calls("utf8_trim_whitespace", 1), calls("ascii_rtrim", 1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=-(-n // 3))])
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by([("p", "ascending")])
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls("utf8_trim_whitespace", 1) - g0[0] >= 1 and calls("ascii_rtrim", 1) - g0[1] >= 1
    print("STRING_TRIM_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + STRING_TRIM_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_string_trim_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.02)
    assert r.returncode == 0 and "STRING_TRIM_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_string_trim_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "STRING_TRIM_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
