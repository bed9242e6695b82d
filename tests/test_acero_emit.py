"""What the Acero nodes share (plugin/acero_common.inc, plugin/grouper_chain.inc), pinned where the plugin scripts do not
reach under the emulator: a result of more than one output batch (the slicing, the numbering, the exact null counts of
device slices), the host-in / host-out copy-back, inputs without batches or rows, and a key row that crosses a Grouper
level with the strings hashed and with their exact chunks.

One script in a fresh interpreter, like tests/test_hash_join_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the CPU tier
and for real on the MI355X under -m gpu.  The sizes are fixed (ARROW_AMD_TEST_SCALE is not read): 40,000 rows are the
fewest that give a second output batch of ExecPlan::kMaxBatchSize = 32768 rows.

ExecBatch::index cannot be read from Python.  The numbering is checked through what depends on it: the order in which the
batches reach the table, and aggregate_rocm's hash_first / hash_last downstream of the join, which refuse batches without
an index and take "first" and "last" in index order.  string_key_hash_bits is a setting of the plugin
(arrow_amd_plugin_set_string_key_hash_bits), not an arx_set_option knob, and has no getter: the script sets it through that
call and puts the default (64) back in a finally."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ACERO_EMIT_SCRIPT = textwrap.dedent(r'''
    import ctypes, os, sys, faulthandler
    faulthandler.enable()
    import numpy as np
    import pyarrow as pa, pyarrow.compute as pc, pyarrow.acero as acero
    sys.path.insert(0, ROOT)
    if os.environ.get("ARROW_AMD_PLUGIN_EMULATED") == "1":
        from tests.emu.build_plugin_emu import build_plugin
    else:
        from arrow_amd.plugin_build import build_plugin
    path = build_plugin()
    rng = np.random.default_rng(97)
    N, NB, BATCH = 40_000, 1_000, 32_768

    def nulls(n, p):
        return rng.random(n) < p

    def strings(n, card, null_p):
        pool = ["", "a", "b" * 20] + [f"s{i}" * (1 + i % 3) for i in range(card)]
        return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=nulls(n, null_p))

    def probe_table(n):
        return pa.table({"k": pa.array(rng.integers(0, NB, n), pa.int64()),
                         "v": pa.array(rng.integers(-2**40, 2**40, n), pa.int64(), mask=nulls(n, 0.1)),
                         "s": strings(n, 40, 0.1)})

    left = probe_table(N)
    right = pa.table({"k": pa.array(rng.permutation(NB), pa.int64()),
                      "g": pa.array(rng.integers(0, 7, NB), pa.int64()),
                      "t": strings(NB, 10, 0.1)})
    small = pa.concat_tables([probe_table(1_700), probe_table(1_300)])          # 3,000 host rows in two batches
    no_batches = pa.Table.from_batches([], schema=right.schema)
    no_rows = left.slice(0, 0)

    src = lambda name, t: acero.Declaration(name, acero.TableSourceNodeOptions(t))
    def join(node, source, lt, rt, jt="inner"):
        return acero.Declaration(node, acero.HashJoinNodeOptions(jt, ["k"], ["k"], ["k", "v", "s"], ["g", "t"]), [src(source, lt), src(source, rt)])
    def order(node, source, t):
        return acero.Declaration(node, acero.OrderByNodeOptions([("k", "ascending")]), [src(source, t)])
    canon = lambda t: t.sort_by([(c, "ascending") for c in t.column_names])
    run = lambda decl: decl.to_table(use_threads=False)

    # ---- the reference's plans over the host tables, before registration
    want_order, want_join = run(order("order_by", "table_source", left)), canon(run(join("hashjoin", "table_source", left, right)))
    want_small_order, want_small_join = run(order("order_by", "table_source", small)), canon(run(join("hashjoin", "table_source", small, right)))
    want_empty = {(side, jt): run(join("hashjoin", "table_source", lt, rt, jt))
                  for side, lt, rt in (("build", small, no_batches), ("probe", no_rows, right)) for jt in ("inner", "left outer")}
    long_pool = [f"a long key string, number {i:04d}" for i in range(60)]
    grouped = pa.table({"ks": pa.array([long_pool[i] for i in rng.integers(0, 60, 5_000)], pa.string(), mask=nulls(5_000, 0.05)),
                        "ki": pa.array(rng.integers(0, 9, 5_000), pa.int64()),
                        "v": pa.array(rng.integers(-2**40, 2**40, 5_000), pa.int64(), mask=nulls(5_000, 0.1))})
    agg = acero.AggregateNodeOptions([("v", "hash_sum", None, "sum"), ("v", "hash_first", None, "first")], keys=["ks", "ki"])
    by_keys = lambda t: t.sort_by([("ks", "ascending"), ("ki", "ascending")])
    want_grouped = by_keys(run(acero.Declaration("aggregate", agg, [src("table_source", grouped)])))

    lib = ctypes.CDLL(path)
    lib.arrow_amd_plugin_last_error.restype = ctypes.c_char_p
    assert lib.arrow_amd_register() == 0, lib.arrow_amd_plugin_last_error()

    def to_device(arr):
        c_arr, c_schema, c_dev = (ctypes.create_string_buffer(m) for m in (80, 72, 128))
        arr._export_to_c(ctypes.addressof(c_arr), ctypes.addressof(c_schema))
        assert lib.arrow_amd_copy_to_device(c_arr, c_schema, c_dev) == 0, lib.arrow_amd_plugin_last_error()
        return pa.Array._import_from_c_device(ctypes.addressof(c_dev), arr.type)

    def to_host(darr, carried=None):
        c_dev, c_schema, c_arr, c_schema2 = (ctypes.create_string_buffer(m) for m in (128, 72, 80, 72))
        darr._export_to_c_device(ctypes.addressof(c_dev), ctypes.addressof(c_schema))
        if carried is not None:      # ArrowArray::null_count as the array carries it (-1: unknown); Python refuses to read it off the CPU
            carried.append(ctypes.c_int64.from_buffer(c_dev, 8).value)
        assert lib.arrow_amd_copy_to_host(c_dev, c_schema, c_arr, c_schema2) == 0, lib.arrow_amd_plugin_last_error()
        return pa.Array._import_from_c(ctypes.addressof(c_arr), ctypes.addressof(c_schema2))

    def on_device(arr):
        return any(b is not None and not b.is_cpu for b in arr.buffers())

    def device_table(t, batches=3):
        return pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                      for b in t.to_batches(max_chunksize=-(-len(t) // batches))])

    def host_table(t):
        return pa.table([pa.chunked_array([to_host(ch) for ch in c.chunks], c.type) for c in t.columns], names=t.column_names)

    # ---- 40,000 device rows: two output batches, every slice device-resident with its exact null count
    dleft, dright = device_table(left), device_table(right, 1)
    assert [len(b) for b in dleft.to_batches()] == [13_334, 13_334, 13_332]
    outputs = {}
    for name, decl in (("order_by_rocm", order("order_by_rocm", "table_source_rocm", dleft)),
                       ("hashjoin_rocm", join("hashjoin_rocm", "table_source_rocm", dleft, dright)),
                       ("hashjoin", join("hashjoin", "table_source", dleft, dright))):
        got = run(decl)
        assert got.num_rows == N, (name, got.num_rows)
        host_columns = []
        for column, field in zip(got.columns, got.schema):
            assert [len(ch) for ch in column.chunks] == [BATCH, N - BATCH], (name, field.name, [len(ch) for ch in column.chunks])
            carried, host_chunks = [], []
            for ch in column.chunks:
                assert on_device(ch), (name, field.name, "an output slice is not device-resident")
                host_chunks.append(to_host(ch, carried))
            counted = [len(h) - pc.count(h).as_py() for h in host_chunks]      # (pc.count: the valid values of the host copy)
            assert carried == counted, (name, field.name, carried, counted)
            host_columns.append(pa.chunked_array(host_chunks, column.type))
        host = pa.table(host_columns, names=got.column_names)
        outputs[name] = (got, host)
    assert outputs["order_by_rocm"][1].equals(want_order), "order_by_rocm differs from order_by over the host table"
    for name in ("hashjoin_rocm", "hashjoin"):
        got = canon(outputs[name][1])
        assert got.schema.equals(want_join.schema), (name, got.schema, want_join.schema)
        assert got.equals(want_join), (name, "differs from hashjoin over the host tables")
    # the slices are numbered 0, 1 in the order they were cut: hash_first / hash_last downstream need the numbers and follow them
    edges = acero.AggregateNodeOptions([("v", "hash_first", None, "first"), ("v", "hash_last", None, "last")], keys=["g"])
    got_edges = run(acero.Declaration("aggregate_rocm", edges, [join("hashjoin_rocm", "table_source_rocm", dleft, dright)])).sort_by("g")
    joined = outputs["hashjoin_rocm"][1].select(["g", "v"]).filter(pc.is_valid(pc.field("v")))     # in output order
    rows = {}
    for g, v in zip(joined.column("g").to_pylist(), joined.column("v").to_pylist()):
        rows.setdefault(g, []).append(v)
    assert got_edges.column("g").to_pylist() == sorted(rows)
    assert got_edges.column("first").to_pylist() == [rows[g][0] for g in sorted(rows)], "hash_first does not follow the slices' numbers"
    assert got_edges.column("last").to_pylist() == [rows[g][-1] for g in sorted(rows)], "hash_last does not follow the slices' numbers"

    # ---- host in, host out
    for name, decl, want, prepare in (("order_by_rocm", order("order_by_rocm", "table_source", small), want_small_order, lambda t: t),
                                      ("hashjoin_rocm", join("hashjoin_rocm", "table_source", small, right), want_small_join, canon)):
        got = run(decl)
        for column in got.columns:
            assert all(not on_device(ch) for ch in column.chunks), (name, "a host plan returned device-resident columns")
        assert prepare(got).equals(want), (name, "over host tables differs from the reference")

    # ---- a build side without batches, a probe side without rows
    dsmall = device_table(small)
    for (side, jt), want in want_empty.items():
        lt, rt = (dsmall, no_batches) if side == "build" else (no_rows, dright)
        got = run(join("hashjoin_rocm", "table_source_rocm", lt, rt, jt))
        assert got.schema.equals(want.schema), (side, jt, got.schema, want.schema)
        assert got.num_rows == want.num_rows == (3_000 if (side, jt) == ("build", "left outer") else 0), (side, jt, got.num_rows, want.num_rows)
        if got.num_rows:
            got = host_table(got)
            assert got.column("g").null_count == got.column("t").null_count == 3_000
            assert canon(got).equals(canon(want)), (side, jt)

    # ---- aggregate_rocm over (utf8 of more than 12 bytes, int64): two Grouper levels, hashed strings and exact chunks
    dgrouped = device_table(grouped)
    lib.arrow_amd_plugin_set_string_key_hash_bits.argtypes = [ctypes.c_int64]
    try:
        for bits in (64, 0):
            lib.arrow_amd_plugin_set_string_key_hash_bits(bits)
            got = by_keys(run(acero.Declaration("aggregate_rocm", agg, [src("table_source_rocm", dgrouped)])))
            assert got.schema.equals(want_grouped.schema), (bits, got.schema, want_grouped.schema)
            assert got.equals(want_grouped), ("aggregate_rocm differs from aggregate", bits)
    finally:
        lib.arrow_amd_plugin_set_string_key_hash_bits(64)
    print("ACERO_EMIT_OK")
''')


def run_script(extra_env):
    env = dict(os.environ, ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + ACERO_EMIT_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_acero_emit_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"})
    assert r.returncode == 0 and "ACERO_EMIT_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_acero_emit_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({})
    assert r.returncode == 0 and "ACERO_EMIT_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
