"""case_when, min_element_wise and max_element_wise through the Arrow registration shim (plugin/case_when.inc,
plugin/element_wise.inc): unmodified pyarrow.compute calls and an Acero plan on device-resident arrays against the same
calls on host copies.  The rows below are run the way tests/plugin_scripts.py::CASES are — in a fresh interpreter, by
`run_case` / `assert_ran` — once on the MI355X and once on the emulated build (as tests/test_plugin_emulated.py does);
the helpers come from tests/plugin_prelude.py."""
import textwrap

import pytest

from . import plugin_scripts as S

CASE_WHEN_SCRIPT = textwrap.dedent(r'''
    import functools, sys, faulthandler
    faulthandler.enable()
    import numpy as np
    import pyarrow as pa, pyarrow.compute as pc, pyarrow.acero as acero
    sys.path.insert(0, ROOT)
    from tests.plugin_prelude import build, calls, device_table, load, register, SC, to_device, to_host
    path = build()
    rng = np.random.default_rng(47)
    n = SC(100_000)
    def column(t, null_p=0.1):
        mask = (rng.random(n) < null_p) if null_p else None
        if pa.types.is_boolean(t):
            return pa.array(rng.random(n) < 0.5, t, mask=mask)
        if pa.types.is_floating(t):
            return pa.array(rng.standard_normal(n), pa.float64(), mask=mask).cast(t)
        if pa.types.is_integer(t):
            return pa.array(rng.integers(-100, 100, n) % (2 ** min(t.bit_width - 1, 20)), pa.int64(), mask=mask).cast(t)
        return pa.array(rng.integers(0, 86_000, n), pa.int32() if t.bit_width == 32 else pa.int64(), mask=mask).view(t)
    def scalar_of(t):
        if pa.types.is_boolean(t):
            return pa.scalar(True, t)
        if pa.types.is_floating(t):
            return pa.scalar(0.25, t)
        if pa.types.is_integer(t):
            return pa.scalar(7, t)
        return pa.array([77], pa.int32() if t.bit_width == 32 else pa.int64()).view(t)[0]      # (temporal: a typed scalar)
    NUMERIC = [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64(), pa.float32(), pa.float64()]
    TEMPORAL = [pa.date32(), pa.date64(), pa.time32("ms"), pa.time64("ns"), pa.timestamp("us", tz="UTC"), pa.duration("ms")]
    conds = [column(pa.bool_()) for _ in range(3)]
    struct_of = lambda cs: pa.StructArray.from_arrays(cs, [f"c{j}" for j in range(len(cs))])
    cut = lambda x, sl: x.slice(sl) if isinstance(x, pa.Array) else x
    # ---- the cases, computed by the reference BEFORE the plugin is loaded: (name) -> (function, arguments, options)
    cases = {}
    for t in [pa.bool_()] + NUMERIC + TEMPORAL:
        v = [column(t) for _ in range(4)]
        cases[f"case_when {t} arrays, else"] = ("case_when", [conds, v[0], v[1], v[2], v[3]], {})
        cases[f"case_when {t} arrays"] = ("case_when", [conds[:2], v[0], v[1]], {})
        if t in (pa.bool_(), pa.int16(), pa.float64(), pa.timestamp("us", tz="UTC")):
            cases[f"case_when {t} scalar / array / null"] = ("case_when", [conds[:2], scalar_of(t), v[1], pa.scalar(None, t)], {})
            cases[f"case_when {t} no nulls"] = ("case_when", [conds[:1], column(t, 0.0), scalar_of(t)], {})
    for t in NUMERIC + [pa.date32(), pa.date64(), pa.time32("ms"), pa.time64("ns"), pa.timestamp("us"), pa.duration("ms")]:      # (exact types: no zone)
        v = [column(t) for _ in range(3)]
        for fn in ("min_element_wise", "max_element_wise"):
            cases[f"{fn} {t} arrays"] = (fn, [v[0], v[1], v[2]], {})
            cases[f"{fn} {t} arrays, nulls kept"] = (fn, [v[0], v[1]], {"skip_nulls": False})
            if t in (pa.int16(), pa.uint64(), pa.float32(), pa.float64(), pa.date32()):
                cases[f"{fn} {t} array / scalar"] = (fn, [v[0], scalar_of(t)], {})
                cases[f"{fn} {t} null scalar / array"] = (fn, [pa.scalar(None, t), v[1]], {"skip_nulls": False})
                cases[f"{fn} {t} no nulls"] = (fn, [column(t, 0.0), scalar_of(t)], {})
                cases[f"{fn} {t} one operand"] = (fn, [v[2]], {})
    def run(fn, args, options, sl, move=lambda x: x):
        if fn == "case_when":
            return pc.case_when(struct_of([move(cut(c, sl)) for c in args[0]]), *[move(cut(x, sl)) if isinstance(x, pa.Array) else x for x in args[1:]])
        return getattr(pc, fn)(*[move(cut(x, sl)) if isinstance(x, pa.Array) else x for x in args], **options)
    want = {(name, sl): run(*case, sl) for name, case in cases.items() for sl in (0, 7)}
    ints32, floats = column(pa.int32()), column(pa.float64())
    want_promoted = pc.max_element_wise(ints32, floats)
    strings = pa.array([None if i % 7 == 0 else f"s{i % 13}" for i in range(n)], pa.string())
    want_strings = [pc.case_when(struct_of(conds[:1]), strings, "else"), pc.min_element_wise(strings, "m"), pc.max_element_wise(strings, "m")]
    want_choose = pc.choose(pa.array(rng.integers(0, 2, n)), ints32, ints32)
    k = pa.array(rng.integers(0, 50, n).astype(np.int32))
    x = pa.array(rng.integers(-100, 100, n), pa.int64(), mask=rng.random(n) < 0.05)
    table = pa.table({"k": k, "x": x})
    lit = lambda v: pc.scalar(pa.scalar(v, pa.int64()))
    def plan(source, t, with_case_when):
        clip = pc.max_element_wise(pc.field("x"), lit(0))
        bucket = pc.case_when(pc.make_struct(pc.less(pc.field("x"), lit(-30)), pc.less(pc.field("x"), lit(40))), lit(1), lit(2), lit(3))
        cols, names = ([pc.field("k"), clip, bucket], ["k", "c", "b"]) if with_case_when else ([pc.field("k"), clip], ["k", "c"])
        aggs = [("c", "hash_sum", None, "s"), ("c", "hash_count", None, "n")] + ([("b", "hash_sum", None, "bs")] if with_case_when else [])
        return acero.Declaration.from_sequence([
            acero.Declaration(source, acero.TableSourceNodeOptions(t)),
            acero.Declaration("project", acero.ProjectNodeOptions(cols, names)),
            acero.Declaration("aggregate_rocm" if source == "table_source_rocm" else "aggregate", acero.AggregateNodeOptions(aggs, keys=["k"]))])
    want_plan = plan("table_source", table, True).to_table(use_threads=False).sort_by("k")

    lib = load(path)
    register(lib)

    to_device = functools.partial(to_device, lib)
    to_host = functools.partial(to_host, lib)
    calls = functools.partial(calls, lib)
    FUNCTIONS = ("case_when", "min_element_wise", "max_element_wise")
    assert all(calls(f, 1) == 0 and calls(f, 0) == 0 for f in FUNCTIONS)
    def same(h, w):      # Array.equals with NaN == NaN and -0.0 != 0.0: floats compare by their bits, like the kernels
        if not pa.types.is_floating(w.type):
            return h.equals(w)
        valid = np.asarray(pc.is_valid(w))
        bits = lambda a: np.frombuffer(pa.concat_arrays([a]).buffers()[1], dtype=f"u{w.type.bit_width // 8}", count=len(a))
        return h.type == w.type and (np.asarray(pc.is_valid(h)) == valid).all() and (bits(h)[valid] == bits(w)[valid]).all()
    # ---- device-resident arrays: equal to the reference on the host copies, results in HBM, one GPU count per call
    done = {f: 0 for f in FUNCTIONS}
    for name, case in cases.items():
        for sl in (0, 7):
            got = run(*case, sl, move=to_device)
            done[case[0]] += 1
            assert got.buffers()[1] is not None and not got.buffers()[1].is_cpu, name
            w = want[name, sl]
            assert got.type == w.type and got.offset == 0, (name, got.type, w.type)
            if "no nulls" in name:
                assert got.buffers()[0] is None, name      # cannot have nulls: no bitmap
            h = to_host(got)
            assert same(h, w) and h.null_count == w.null_count, (name, sl)
    assert all(calls(f, 1) == done[f] and calls(f, 0) == 0 for f in FUNCTIONS), [(calls(f, 1), calls(f, 0), done[f]) for f in FUNCTIONS]
    # a struct that is itself a slice: every field carries its own offset on top of the struct's
    case = cases["case_when int32 arrays, else"]
    dstruct = struct_of([to_device(c) for c in conds]).slice(7)
    got = pc.case_when(dstruct, *[to_device(v).slice(7) for v in case[1][1:]])
    assert same(to_host(got), want["case_when int32 arrays, else", 7])
    done["case_when"] += 1
    # ---- host arrays and scalars keep the reference's kernels and results, implicit casts included
    for name, case in cases.items():
        assert same(run(*case, 7), want[name, 7]), name
    assert pc.max_element_wise(ints32, floats).equals(want_promoted) and want_promoted.type == pa.float64()
    assert pc.case_when(struct_of(conds[:1]), strings, "else").equals(want_strings[0])
    assert pc.min_element_wise(strings, "m").equals(want_strings[1]) and pc.max_element_wise(strings, "m").equals(want_strings[2])
    assert pc.max_element_wise(pa.scalar(1), pa.scalar(2)).as_py() == 2
    assert all(calls(f, 0) >= sum(1 for c in cases.values() if c[0] == f) for f in FUNCTIONS), [calls(f, 0) for f in FUNCTIONS]
    assert all(calls(f, 1) == done[f] for f in FUNCTIONS)
    # the reference's argument checks keep their texts on device operands
    dconds, dints = [to_device(c) for c in conds], to_device(ints32)
    # (a validity bitmap in HBM whose null count the struct does not know: counted on the device)
    top_nulls = pa.StructArray.from_buffers(pa.struct([("a", pa.bool_())]), n, [to_device(pa.array(rng.random(n) >= 0.1)).buffers()[1]], children=dconds[:1])
    for f, text in ((lambda: pc.case_when(struct_of(dconds), dints), "number of struct fields must be equal to or one less than count of remaining arguments (1), got: 3"),
                    (lambda: pc.case_when(top_nulls, dints), "cond struct must not be a null scalar or have top-level nulls")):
        try:
            f()
            raise SystemExit(f"case_when: accepted a call that must fail with {text!r}")
        except pa.ArrowInvalid as e:
            assert text in str(e), e
    # ---- refused with a Status, not read by a CPU kernel
    dstrings, dflags = to_device(strings), to_device(conds[0])
    dchoice = to_device(pa.array(rng.integers(0, 2, n)))
    refused = {"case_when device utf8": lambda: pc.case_when(struct_of(dconds[:1]), dstrings, "else"),
               "case_when device utf8 else": lambda: pc.case_when(struct_of(dconds[:1]), "then", dstrings),
               "case_when host conds, device values": lambda: pc.case_when(struct_of(conds[:1]), dints, dints),
               "case_when device conds, host values": lambda: pc.case_when(struct_of(dconds[:1]), ints32, ints32),
               "case_when device conds, device / host values": lambda: pc.case_when(struct_of(dconds[:1]), dints, ints32),
               "min_element_wise device utf8": lambda: pc.min_element_wise(dstrings, dstrings),
               "max_element_wise device utf8": lambda: pc.max_element_wise(dstrings, "m"),
               "min_element_wise device / host": lambda: pc.min_element_wise(dints, ints32),
               "max_element_wise host / device": lambda: pc.max_element_wise(ints32, dints),
               "choose device indices": lambda: pc.choose(dchoice, ints32, ints32),
               "choose device values": lambda: pc.choose(pa.array(rng.integers(0, 2, n)), dints, ints32),
               "choose all on the device": lambda: pc.choose(dchoice, dints, dints),
               "choose device utf8": lambda: pc.choose(dchoice, dstrings, dstrings)}
    for name, f in refused.items():
        try:
            f()
            raise SystemExit(f"{name} was accepted")
        except pa.ArrowNotImplementedError as e:
            assert "arrow_amd" in str(e) and "device-resident" in str(e) and name.split()[0] in str(e), (name, e)
    assert pc.choose(pa.array(rng.integers(0, 2, n)), ints32, ints32).type == want_choose.type      # host arrays: the reference's kernel
    assert all(calls(f, 1) == done[f] for f in FUNCTIONS)
    # ---- Acero: table_source_rocm -> project(k, max_element_wise(x, 0), case_when(make_struct(x < -30, x < 40), 1, 2, 3)) ->
    # aggregate_rocm over a three-batch device table equals the host plan
    g0 = {f: calls(f, 1) for f in FUNCTIONS}
    dt = device_table(lib, table)
    assert dt.column(0).num_chunks == 3
    got_plan = plan("table_source_rocm", dt, True).to_table(use_threads=False).sort_by("k")
    assert got_plan.equals(want_plan), (got_plan.slice(0, 5), want_plan.slice(0, 5))
    assert calls("max_element_wise", 1) - g0["max_element_wise"] >= 3 and calls("case_when", 1) - g0["case_when"] >= 3
    print("CASE_WHEN_OK", sum(done.values()))
''')

# (id, script, marker, emu_scale, doc), as the rows of tests/plugin_scripts.py::CASES
CASES = [
    ('case_when_min_max_element_wise_on_device_resident_arrays', CASE_WHEN_SCRIPT, 'CASE_WHEN_OK', 0.01,
     'pc.case_when / pc.min_element_wise / pc.max_element_wise on device-resident arrays equal the host calls (results in HBM, one GPU '
     'count per call); host arrays keep the reference kernels; utf8 operands, mixed host / device arrays and any device argument of '
     'pc.choose are refused with a Status; an Acero plan projecting max_element_wise and case_when over a device table equals the host plan'),
]


@pytest.mark.gpu
@pytest.mark.parametrize("script,marker", [pytest.param(c[1], c[2], id=c[0]) for c in CASES])
def test_plugin_case_when(script, marker):
    pytest.importorskip("pyarrow")
    S.assert_ran(S.run_case(script, emulated=False, scale=1, timeout=900), marker)


@pytest.mark.emu
@pytest.mark.parametrize("script,marker,scale", [pytest.param(c[1], c[2], c[3], id=c[0]) for c in CASES])
def test_plugin_case_when_emulated(script, marker, scale):
    pytest.importorskip("pyarrow")
    S.assert_ran(S.run_case(script, emulated=True, scale=scale, timeout=1500), marker)
