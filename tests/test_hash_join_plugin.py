"""The hashjoin_rocm Acero node (plugin/hash_join_node.inc) and the guard in front of the stock `hashjoin` factory
(plugin/acero_override.inc), through the Arrow registration shim.

One script in a fresh interpreter, like tests/test_set_lookup_plugin.py: under ARROW_AMD_PLUGIN_EMULATED=1 in the CPU tier
(the shim on the emulated kernels, scale 0.01) and for real on the MI355X under -m gpu (about 2 x 10^5 probe rows against
5 x 10^4 build rows).  Device tables are cut into three batches per side.  Every device plan must equal the reference's
`hashjoin` over the host tables after sorting.  pyarrow's HashJoinNodeOptions does not expose key_cmp, so JoinKeyCmp::IS
cannot be reached from here; the mirror's tests pin null_equals_null.  pa.Table.join refuses device tables in Python
(Table._assert_cpu) before it builds a plan, so the stock name is covered through the Declaration."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HASH_JOIN_SCRIPT = textwrap.dedent(r'''
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
    rng = np.random.default_rng(41)
    nl, nb = SC(200_000), SC(50_000)
    JOIN_TYPES = ["left semi", "right semi", "left anti", "right anti", "inner", "left outer", "right outer", "full outer"]

    def nulls(n, p):
        return rng.random(n) < p

    def strings(n, card, null_p=0.0):
        pool = ["", "a", "b" * 20] + [f"s{i}" * (1 + i % 3) for i in range(card)]
        return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=nulls(n, null_p) if null_p else None)

    card = max(8, nb // 2)      # about two build rows per key: the output stays near the input's size
    fpool = rng.standard_normal(card)
    fpool[:3] = [0.0, -0.0, np.nan]
    left = pa.table({
        "k": pa.array(rng.integers(0, card, nl), pa.int64(), mask=nulls(nl, 0.05)),
        "k32": pa.array(rng.integers(0, 40, nl).astype(np.int32)), "ks": strings(nl, 12, 0.03),
        "kf": pa.array(fpool[rng.integers(0, card, nl)], mask=nulls(nl, 0.02)),
        "lid": pa.array(np.arange(nl, dtype=np.int64)), "a": pa.array(rng.integers(0, 100, nl)),
        "s": strings(nl, 50, 0.1), "f": pa.array(rng.random(nl) < 0.5, mask=nulls(nl, 0.1)),
        "p": pa.array(rng.integers(-5, 5, nl), mask=nulls(nl, 0.2))})
    right = pa.table({
        "k": pa.array(rng.integers(0, card, nb), pa.int64(), mask=nulls(nb, 0.05)),
        "k32": pa.array(rng.integers(0, 40, nb).astype(np.int32)), "ks": strings(nb, 12, 0.03),
        "kf": pa.array(fpool[rng.integers(0, card, nb)], mask=nulls(nb, 0.02)),
        "rid": pa.array(np.arange(nb, dtype=np.int64)), "b": pa.array(rng.integers(0, 100, nb), mask=nulls(nb, 0.05)),
        "g": pa.array(rng.integers(0, 20, nb).astype(np.int32)), "t": strings(nb, 30),
        "p": pa.array(rng.standard_normal(nb), mask=nulls(nb, 0.1))})

    def plan(join, source, lt, rt, *args, **kw):
        opts = acero.HashJoinNodeOptions(*args, **kw)
        return acero.Declaration(join, opts, [acero.Declaration(source, acero.TableSourceNodeOptions(lt)),
                                              acero.Declaration(source, acero.TableSourceNodeOptions(rt))])

    def ordered(t):
        # sorted by the row numbers; NaN keys become a marker value, since equals() holds NaN != NaN
        for i, f in enumerate(t.schema):
            if pa.types.is_floating(f.type):
                t = t.set_column(i, f, pc.if_else(pc.is_nan(t.column(i)), 1e300, t.column(i)))
        ids = [(c, "ascending") for c in ("lid", "rid") if c in t.column_names]
        return t.sort_by(ids)

    two_col_small = lambda t: t.slice(0, max(64, len(t) // 8))     # the two-column keys multiply: a smaller cut
    CASES = []
    for jt in JOIN_TYPES:                                            # int64 keys with nulls, every payload, suffixes
        CASES.append(("i64 " + jt, left, right, (jt, ["k"], ["k"]), dict(output_suffix_for_left="_l", output_suffix_for_right="_r")))
    for jt in ("inner", "full outer", "right anti", "left semi"):    # int32 + utf8 keys
        lo = [] if jt == "right anti" else ["lid", "ks", "f"]
        ro = [] if jt == "left semi" else ["rid", "t"]
        CASES.append(("i32+utf8 " + jt, two_col_small(left), two_col_small(right), (jt, ["k32", "ks"], ["k32", "ks"], lo, ro), {}))
    for jt in ("inner", "left outer"):                               # float keys: -0.0 and NaN compare by bits
        CASES.append(("f64 " + jt, left, right, (jt, ["kf"], ["kf"], ["lid", "s"], ["rid"]), {}))
    flt = pc.field("a") < pc.field("b")
    for jt in ("inner", "left outer", "full outer", "left anti", "right semi"):
        lo = [] if jt == "right semi" else ["lid", "a", "s"]
        ro = [] if jt == "left anti" else ["rid", "b"]
        CASES.append(("filter " + jt, left, right, (jt, ["k"], ["k"], lo, ro), dict(filter_expression=flt)))
    CASES.append(("filter & inner", left, right, ("inner", ["k"], ["k"], ["lid"], ["rid", "g"]),
                  dict(filter_expression=flt & (pc.field("g") > 4))))
    CASES.append(("subset + suffix", left, right, ("left outer", ["k"], ["k"], ["lid", "p"], ["p", "rid"]),
                  dict(output_suffix_for_left="_x", output_suffix_for_right="_y")))
    want = [ordered(plan("hashjoin", "table_source", lt, rt, *args, **kw).to_table(use_threads=False))
            for _, lt, rt, args, kw in CASES]
    agg = acero.AggregateNodeOptions([("a", "hash_sum", None, "sa"), ("a", "hash_count", None, "c")], keys=["g"])
    want_agg = acero.Declaration("aggregate", agg, [plan("hashjoin", "table_source", left, right, "inner", ["k"], ["k"],
                                                         ["a"], ["g"])]).to_table(use_threads=False).sort_by("g")
    want_join = left.select(["k", "lid", "a"]).join(right.select(["k", "rid", "g"]), "k", join_type="inner").sort_by(
        [("lid", "ascending"), ("rid", "ascending")])

    lib = ctypes.CDLL(path)
    lib.arrow_amd_plugin_last_error.restype = ctypes.c_char_p
    lib.arrow_amd_plugin_calls.restype = ctypes.c_int64
    lib.arrow_amd_plugin_calls.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.arrow_amd_plugin_acero_guard.restype = ctypes.c_int64
    lib.arrow_amd_plugin_acero_guard.argtypes = [ctypes.c_int]
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
        return any(b is not None and not b.is_cpu for b in arr.buffers())

    def device_table(t):       # three batches per side
        return pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(c) for c in b.columns], names=b.schema.names)
                                      for b in t.to_batches(max_chunksize=-(-len(t) // 3))])

    def host_table(t):
        for c in t.columns:
            for ch in c.chunks:
                assert len(ch) == 0 or on_device(ch), "an output column is not device-resident"
        return pa.table([pa.chunked_array([to_host(ch) for ch in c.chunks], c.type) for c in t.columns], names=t.column_names)

    calls = lambda: lib.arrow_amd_plugin_calls(b"hashjoin", 1)
    takeovers = lambda: lib.arrow_amd_plugin_acero_guard(1)
    assert calls() == 0
    devs = {}
    def dev(t):
        if id(t) not in devs:
            devs[id(t)] = device_table(t)
        return devs[id(t)]

    # ---- hashjoin_rocm over table_source_rocm equals the host hashjoin after sorting
    for (name, lt, rt, args, kw), w in zip(CASES, want):
        c0 = calls()
        got = ordered(host_table(plan("hashjoin_rocm", "table_source_rocm", dev(lt), dev(rt), *args, **kw).to_table(use_threads=False)))
        assert got.schema.names == w.schema.names, (name, got.schema.names, w.schema.names)
        assert got.schema.equals(w.schema), (name, got.schema, w.schema)
        assert got.equals(w), (name, got.num_rows, w.num_rows, got.slice(0, 5), w.slice(0, 5))
        assert calls() - c0 == 1, name
    # ---- the stock name over device tables: the guard takes the plan over
    dl, dr = dev(left), dev(right)
    t0, c0 = takeovers(), calls()
    name, lt, rt, args, kw = CASES[4]
    got = ordered(host_table(plan("hashjoin", "table_source", dl, dr, *args, **kw).to_table(use_threads=False)))
    assert got.equals(want[4]), name
    assert takeovers() - t0 == 1 and calls() - c0 == 1, (takeovers() - t0, calls() - c0)
    # pa.Table.join itself refuses device tables in Python (Table._assert_cpu) before any plan is built: the Declaration
    # above is the route a device join takes under the stock name
    try:
        dl.select(["k", "lid", "a"]).join(dr.select(["k", "rid", "g"]), "k", join_type="inner")
        raise SystemExit("pa.Table.join accepts device tables now: compare it with want_join here")
    except NotImplementedError as e:
        assert "CPU device" in str(e), e
    # ---- host-only plans keep the stock node and leave both counters alone
    t0, c0 = takeovers(), calls()
    assert ordered(plan("hashjoin", "table_source", left, right, *CASES[7][3], **CASES[7][4]).to_table(use_threads=False)).equals(want[7])
    assert left.select(["k", "lid", "a"]).join(right.select(["k", "rid", "g"]), "k", join_type="inner").sort_by(
        [("lid", "ascending"), ("rid", "ascending")]).equals(want_join)
    assert takeovers() == t0 and calls() == c0
    # ---- a dictionary key column on the device: a Status
    dic = pa.DictionaryArray.from_arrays(to_device(pa.array([0, 1, 0, None], pa.int32())), to_device(pa.array(["a", "b"])), safe=False)
    dt = pa.table({"d": dic, "x": to_device(pa.array([1, 2, 3, 4]))})
    for join, source in (("hashjoin_rocm", "table_source_rocm"), ("hashjoin", "table_source")):
        try:
            plan(join, source, dt, dt, "inner", ["d"], ["d"], ["x"], []).to_table(use_threads=False)
            raise SystemExit("a device-resident dictionary key was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e), e
    # ---- a join feeding aggregate_rocm
    join = plan("hashjoin_rocm", "table_source_rocm", dl, dr, "inner", ["k"], ["k"], ["a"], ["g"])
    got_agg = acero.Declaration("aggregate_rocm", agg, [join]).to_table(use_threads=False).sort_by("g")
    assert got_agg.equals(want_agg), (got_agg, want_agg)
    print("HASH_JOIN_PLUGIN_OK", len(CASES))
''')


def run_script(extra_env, scale):
    env = dict(os.environ, ARROW_AMD_TEST_SCALE=str(scale), ARROW_AMD_TEST_LIGHT="1", **extra_env)
    return subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + HASH_JOIN_SCRIPT], capture_output=True, text=True,
                          timeout=1500, cwd=ROOT, env=env)


@pytest.mark.emu
def test_hash_join_plugin_emulated():
    pytest.importorskip("pyarrow")
    r = run_script({"ARROW_AMD_PLUGIN_EMULATED": "1"}, 0.01)
    assert r.returncode == 0 and "HASH_JOIN_PLUGIN_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_hash_join_plugin_gpu():
    pytest.importorskip("pyarrow")
    r = run_script({}, 1)
    assert r.returncode == 0 and "HASH_JOIN_PLUGIN_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
