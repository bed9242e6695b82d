"""pc.match_substring / pc.starts_with / pc.ends_with through the Arrow registration shim (plugin/match_substring.inc) on
device-resident arrays.

The script runs in a fresh interpreter, like the rows of tests/plugin_scripts.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the
CPU tier (the shim on the emulated kernels) and for real on the MI355X under -m gpu.  Device-resident calls must equal
the same calls on the host copies and raise the shim's GPU counters; host arrays keep the reference's kernels
(ignore_case included); ignore_case and the string-search siblings without a device kernel are refused on device arrays
with a Status; an Acero plan table_source_rocm -> filter(match_substring) -> aggregate_rocm equals the host plan."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MATCH_SUBSTRING_SCRIPT = textwrap.dedent(r'''
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
    rng = np.random.default_rng(29)
    n = SC(300_000)
    FNS = ("match_substring", "starts_with", "ends_with")
    PAT = "v1"
    pool = ["", "a", "v1", "xv1", "v1x", "b" * 20 + "v1", "v", "1v", None] + [f"v{i}" * (1 + i % 4) for i in range(40)]
    base = pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string())
    wide = pa.array(["w" * 3000 + "v1" + "w" * 2000, None, "w" * 6000, "v1" + "w" * 5000] * 16, pa.string())   # auto: the bytes kernel
    cases = {"utf8": base, "binary": base.cast(pa.binary()), "large_utf8": base.cast(pa.large_string()),
             "large_binary": base.cast(pa.large_binary()), "wide": wide, "no_nulls": base.drop_null()}
    want = {(name, fn, sl): getattr(pc, fn)(a.slice(sl), PAT) for name, a in cases.items() for fn in FNS for sl in (0, 7)}
    want_empty = pc.match_substring(base, "")
    want_icase = pc.match_substring(base, "V1", ignore_case=True)
    SIBLINGS = {"match_like": lambda a: pc.match_like(a, "%v1%"), "match_substring_regex": lambda a: pc.match_substring_regex(a, "v1+"),
                "find_substring": lambda a: pc.find_substring(a, "v1"), "find_substring_regex": lambda a: pc.find_substring_regex(a, "v1+"),
                "count_substring": lambda a: pc.count_substring(a, "v1"), "count_substring_regex": lambda a: pc.count_substring_regex(a, "v1+")}
    want_siblings = {name: f(base) for name, f in SIBLINGS.items()}
    table = pa.table({"k": pa.array(rng.integers(0, 50, n).astype(np.int32)), "v": pa.array(rng.integers(-100, 100, n)), "s": base})
    def plan(source, t):
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("filter", acero.FilterNodeOptions(pc.match_substring(pc.field("s"), PAT))),
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
    gpu0 = {f: calls(f, 1) for f in FNS}
    done = 0
    for name, a in cases.items():
        d = to_device(a)
        for sl in (0, 7):
            x = d.slice(sl)
            for fn in FNS:
                got = getattr(pc, fn)(x, PAT)
                assert on_device(got), (name, fn)
                h = to_host(got)
                w = want[name, fn, sl]
                assert h.equals(w) and h.null_count == w.null_count, (name, fn, sl)
            done += 1
    for f in FNS:
        assert calls(f, 1) - gpu0[f] == done, (f, done, calls(f, 1) - gpu0[f])
    dbase = to_device(base)
    assert to_host(pc.match_substring(dbase, "")).equals(want_empty)
    # ---- host arrays keep the reference's kernels and results, ignore_case included
    stock0 = {f: calls(f, 0) for f in FNS}
    for name, a in cases.items():
        for fn in FNS:
            assert getattr(pc, fn)(a.slice(7), PAT).equals(want[name, fn, 7]), (name, fn)
    assert pc.match_substring(base, "V1", ignore_case=True).equals(want_icase)
    assert pc.match_substring(pa.scalar("xv1"), PAT).as_py() is True
    for f in FNS:
        assert calls(f, 0) - stock0[f] >= len(cases), (f, calls(f, 0) - stock0[f])
    # ---- ignore_case and the siblings without a device kernel on a device array: a Status, not a CPU read of device memory
    refused = {f"{fn} ignore_case": (lambda a, fn=fn: getattr(pc, fn)(a, "V1", ignore_case=True)) for fn in FNS}
    refused.update(SIBLINGS)
    for name, f in refused.items():
        try:
            f(dbase)
            raise SystemExit(f"{name} on a device-resident utf8 array was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e), (name, e)
    # ---- the same siblings on host arrays still equal the reference
    for name, f in SIBLINGS.items():
        assert f(base).equals(want_siblings[name]), name
    # ---- Acero: table_source_rocm -> filter(match_substring(s, ...)) -> aggregate_rocm over a device table equals the host plan
    g0 = calls("match_substring", 1)
    dt = pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                for b in table.to_batches(max_chunksize=max(64, n // 3))])
    got_plan = plan("table_source_rocm", dt).to_table(use_threads=False).sort_by("k")
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls("match_substring", 1) - g0 >= 3, calls("match_substring", 1) - g0
    print("MATCH_SUBSTRING_OK", done)
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + MATCH_SUBSTRING_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_match_substring_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.01)
    assert r.returncode == 0 and "MATCH_SUBSTRING_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_match_substring_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "MATCH_SUBSTRING_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
