"""The residual filter of the hash join (HashJoinNodeOptions::filter) on the device: compute.hash_join_indices /
hash_join with `filter=`, csrc/hash_join.hip's filter count / compact / flags-to-mask kernels.

Every case is compared exactly, order included, with a Python restatement of the rules (a key-equal pair is a match
only where the filter is true; a null result is no match; outer, semi and anti rows follow from the passing pairs, per
build ROW), and after a canonical sort with the reference's HashJoinNode over host tables with the same filter
expression.  The emu tier runs the kernel sources under the SIMT emulator; the gpu tier runs the same cases on the MI355X."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.acero as acero  # noqa: E402
import pyarrow.compute as pc  # noqa: E402

JOIN_TYPES = ["left semi", "right semi", "left anti", "right anti", "inner", "left outer", "right outer", "full outer"]
FILTERS = ["none", "all", "half", "half_nulls"]


class Case:
    """Two host tables (k, a, lid) / (k, b, rid), and the filter three ways: a pyarrow expression for the reference, a
    host predicate (i, j) -> True / False / None for the restatement, and the mirror's callable."""

    def __init__(self, lk, rk, a, b, expression=None, predicate=None):
        self.lk, self.rk, self.a, self.b = lk, rk, a, b
        self.left = pa.table({"k": lk, "a": a, "lid": pa.array(np.arange(len(lk), dtype=np.int64))})
        self.right = pa.table({"k": rk, "b": b, "rid": pa.array(np.arange(len(rk), dtype=np.int64))})
        self.expression = expression if expression is not None else pc.field("a") < pc.field("b")
        av, bv = a.to_pylist(), b.to_pylist()
        self.predicate = predicate or (lambda i, j: None if av[i] is None or bv[j] is None else av[i] < bv[j])
        self.calls = 0

    def mirror_filter(self, amd, bit_offset=0):
        def fn(left_rows, right_rows):
            self.calls += 1
            res = [self.predicate(i, j) for i, j in zip(left_rows.to_pylist(), right_rows.to_pylist())]
            arr = pa.array([True, None, False][:bit_offset] + res, pa.bool_())
            return amd.Array.from_pyarrow(arr).slice(bit_offset)
        return fn


def restated(case, jt):
    """Part 1 of the contract: probe order, ascending build rows among the passing pairs, right-only rows last in
    build-row order, semi / anti rows in input order."""
    lk, rk = case.lk.to_pylist(), case.rk.to_pylist()
    groups = {}
    for j, k in enumerate(rk):
        if k is not None:
            groups.setdefault(k, []).append(j)
    hits = [[j for j in groups.get(k, []) if case.predicate(i, j) is True] if k is not None else []
            for i, k in enumerate(lk)]
    matched = set(j for h in hits for j in h)
    if jt == "left semi":
        return [i for i, h in enumerate(hits) if h], None
    if jt == "left anti":
        return [i for i, h in enumerate(hits) if not h], None
    if jt == "right semi":
        return None, sorted(matched)
    if jt == "right anti":
        return None, [j for j in range(len(rk)) if j not in matched]
    left, right = [], []
    for i, h in enumerate(hits):
        if h:
            left += [i] * len(h)
            right += h
        elif jt in ("left outer", "full outer"):
            left.append(i)
            right.append(None)
    if jt in ("right outer", "full outer"):
        tail = [j for j in range(len(rk)) if j not in matched]
        left += [None] * len(tail)
        right += tail
    return left, right


def via_reference(case, jt):
    lo = [] if jt in ("right semi", "right anti") else ["lid"]
    ro = [] if jt in ("left semi", "left anti") else ["rid"]
    opts = acero.HashJoinNodeOptions(jt, ["k"], ["k"], lo, ro, filter_expression=case.expression)
    out = acero.Declaration("hashjoin", opts, [acero.Declaration("table_source", acero.TableSourceNodeOptions(case.left)),
                                               acero.Declaration("table_source", acero.TableSourceNodeOptions(case.right))]
                            ).to_table(use_threads=False)
    return [out[c].to_pylist() if c in out.column_names else None for c in ("lid", "rid")]


def canonical(left, right):
    n = len(left) if left is not None else len(right)
    rows = list(zip(left if left is not None else [None] * n, right if right is not None else [None] * n))
    return sorted(rows, key=lambda r: tuple(-1 if v is None else v for v in r))


def run(amd, case, jt, bit_offset=0, **kw):
    li, ri = amd.compute.hash_join_indices([amd.Array.from_pyarrow(case.lk)], [amd.Array.from_pyarrow(case.rk)], jt,
                                           filter=case.mirror_filter(amd, bit_offset), **kw)
    for x in (li, ri):
        assert x is None or x.type.name == "int64"
    return (li.to_pylist() if li is not None else None), (ri.to_pylist() if ri is not None else None)


def check(amd, case, jt, bit_offset=0):
    got = run(amd, case, jt, bit_offset)
    assert got == restated(case, jt), jt
    assert canonical(*got) == canonical(*via_reference(case, jt)), jt


def keys(rng, n, card, null_p):
    return pa.array(rng.integers(0, card, n), pa.int64(), mask=(rng.random(n) < null_p) if null_p else None)


def grid_case(which, nl=1500, nb=1000):
    """About 30 distinct keys with 5 % nulls: ~50 000 candidate pairs over ~780 pass words and ~100 tiles of 512."""
    rng = np.random.default_rng([0xF17, FILTERS.index(which)])
    lk, rk = keys(rng, nl, 30, 0.05), keys(rng, nb, 30, 0.05)
    if which == "none":
        a, b = pa.array(np.ones(nl, np.int64)), pa.array(np.zeros(nb, np.int64))
    elif which == "all":
        a, b = pa.array(np.zeros(nl, np.int64)), pa.array(np.ones(nb, np.int64))
    else:
        null_p = 0.05 if which == "half_nulls" else 0.0       # a null on either side: ~10 % null results
        a = pa.array(rng.integers(0, 100, nl), mask=(rng.random(nl) < null_p) if null_p else None)
        b = pa.array(rng.integers(0, 100, nb), mask=(rng.random(nb) < null_p) if null_p else None)
    return Case(lk, rk, a, b)


def _grid(ctx, jt):
    for which in FILTERS:
        check(ctx, grid_case(which), jt)


def hot_key_case():
    """One key with 700 build rows hit by 5 probe rows (other keys around them): runs of 700 slots that cross 64-slot
    words and 512-slot tiles.  Only scattered slots pass: the first and last of every run, the slots on both sides of
    every word boundary near them and of the tile boundaries, and a few inside."""
    nb_hot, probes = 700, 5
    rk = pa.array([7] * nb_hot + [100 + i for i in range(40)], pa.int64())
    lk = pa.array([3, 7, 7, 100, 7, 9, 7, 7, 120], pa.int64())
    hot_rows = [i for i, k in enumerate(lk.to_pylist()) if k == 7]
    assert len(hot_rows) == probes
    # candidate slots: row 1 -> [0, 700), row 2 -> [700, 1400), row 3 (key 100) -> 1400, row 4 -> [1401, 2101), ...
    starts, pos = {}, 0
    for i, k in enumerate(lk.to_pylist()):
        starts[i] = pos
        pos += nb_hot if k == 7 else (1 if k >= 100 else 0)
    passing = set()
    for i in hot_rows:
        s = starts[i]
        passing |= {s, s + nb_hot - 1, s + 350}
        for boundary in range(((s + 63) // 64) * 64, s + nb_hot, 64):
            if boundary % 512 == 0 or boundary - s < 130 or s + nb_hot - boundary < 130:
                passing |= {x for x in (boundary - 1, boundary) if s <= x < s + nb_hot}
    passing.discard(starts[hot_rows[2]])     # one run without its first slot
    pairs = set()
    for i in hot_rows:
        pairs |= {(i, x - starts[i]) for x in passing if starts[i] <= x < starts[i] + nb_hot}
    code = sorted(i * 1000 + j for i, j in pairs)
    expression = pc.is_in(pc.field("lid") * 1000 + pc.field("rid"), pa.array(code, pa.int64()))
    a, b = pa.array(np.zeros(len(lk), np.int64)), pa.array(np.zeros(len(rk), np.int64))
    return Case(lk, rk, a, b, expression, lambda i, j: (i, j) in pairs)


def _hot_key(ctx):
    case = hot_key_case()
    for jt in JOIN_TYPES:
        check(ctx, case, jt)


def _edges(ctx):
    i64 = lambda v: pa.array(v, pa.int64())   # noqa: E731
    # T = 0: no key in common; the filter is not asked
    case = Case(i64([1, 2, None, 3]), i64([10, 11, None]), i64([0] * 4), i64([1] * 3))
    for jt in JOIN_TYPES:
        check(ctx, case, jt)
    assert case.calls == 0
    # an empty side
    for lk, rk in (([], [1, 2, 2]), ([1, 2, 2], [])):
        case = Case(i64(lk), i64(rk), i64([0] * len(lk)), i64([1] * len(rk)))
        for jt in JOIN_TYPES:
            check(ctx, case, jt)
    # a probe row whose every candidate fails (a = 9), between rows that pass; build row 2 (b = 0) passes for nobody
    case = Case(i64([1, 1, 1, 2, 1]), i64([1, 1, 1, 2]), i64([0, 9, 0, 9, 1]), i64([5, 1, 0, 3]))
    for jt in JOIN_TYPES:
        check(ctx, case, jt)
    # the pass column as a slice with a bit offset of 3
    case = grid_case("half_nulls", 300, 200)
    for jt in JOIN_TYPES:
        check(ctx, case, jt, bit_offset=3)


def _capacity(ctx):
    amd = ctx
    i64 = lambda v: pa.array(v, pa.int64())   # noqa: E731
    # left outer: 6 candidates, all pass, plus 4 probe rows without a candidate = 10 rows: the filtered total is refused
    case = Case(i64([1, 1, 1, 5, 5, 5, 5]), i64([1, 1]), i64([0] * 7), i64([1] * 2))
    with pytest.raises(amd._lib.ArrowCapacityError):
        run(amd, case, "left outer", max_output_rows=9)
    assert len(run(amd, case, "left outer", max_output_rows=10)[0]) == 10
    # the candidates are allocated first: they count
    with pytest.raises(amd._lib.ArrowCapacityError):
        run(amd, case, "left semi", max_output_rows=5)
    # full outer: 9 candidates, 6 pass (not build row 0), 6 right-only rows: the excess is only the tail
    case = Case(i64([1, 1, 1]), i64([1, 1, 1, 2, 2, 2, 2, 2]), i64([0] * 3), i64([0, 1, 1, 1, 1, 1, 1, 1]))
    with pytest.raises(amd._lib.ArrowCapacityError):
        run(amd, case, "full outer", max_output_rows=11)
    li, ri = run(amd, case, "full outer", max_output_rows=12)
    assert len(li) == 12 and li.count(None) == 6 and ri[-6:] == [0, 3, 4, 5, 6, 7]


def _filter_none_is_todays_path(ctx):
    amd = ctx
    case = grid_case("half", 300, 200)
    lk, rk = [amd.Array.from_pyarrow(case.lk)], [amd.Array.from_pyarrow(case.rk)]
    for jt in JOIN_TYPES:
        a = amd.compute.hash_join_indices(lk, rk, jt)
        b = amd.compute.hash_join_indices(lk, rk, jt, filter=None)
        assert [x if x is None else x.to_pylist() for x in a] == [x if x is None else x.to_pylist() for x in b], jt


def _tables(ctx):
    """hash_join(filter=): the callable gets the gathered columns by name and evaluates on the device."""
    amd = ctx
    case = grid_case("half_nulls", 400, 300)
    dl = {n: amd.Array.from_pyarrow(case.left[n].combine_chunks()) for n in case.left.column_names}
    dr = {n: amd.Array.from_pyarrow(case.right[n].combine_chunks()) for n in case.right.column_names}
    seen = []

    def on_device(left, right):
        seen.append((sorted(left), sorted(right)))
        out = amd.compute.less(left["a"], right["b"])
        seen.append((sorted(left), sorted(right)))
        return out

    for jt in JOIN_TYPES:
        out = amd.compute.hash_join(dl, dr, "k", "k", jt, left_output=["lid"], right_output=["rid"], filter=on_device)
        got = {n: a.to_pylist() for n, a in out}
        assert (got.get("lid"), got.get("rid")) == restated(case, jt), jt
    assert seen[0] == ([], []) and seen[1] == (["a"], ["b"])      # only what the filter reads is gathered
    with pytest.raises(amd._lib.ArrowInvalid, match="boolean Array"):
        amd.compute.hash_join(dl, dr, "k", "k", "inner", filter=lambda left, right: left["a"])


@pytest.mark.emu
@pytest.mark.parametrize("jt", JOIN_TYPES)
def test_hash_join_filter_grid(emu_ctx, jt):
    _grid(emu_ctx, jt)


@pytest.mark.emu
def test_hash_join_filter_hot_key_scattered_slots(emu_ctx):
    _hot_key(emu_ctx)


@pytest.mark.emu
def test_hash_join_filter_edges(emu_ctx):
    _edges(emu_ctx)


@pytest.mark.emu
def test_hash_join_filter_capacity(emu_ctx):
    _capacity(emu_ctx)


@pytest.mark.emu
def test_hash_join_filter_none_is_todays_path(emu_ctx):
    _filter_none_is_todays_path(emu_ctx)


@pytest.mark.emu
def test_hash_join_filter_tables(emu_ctx):
    _tables(emu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("jt", JOIN_TYPES)
def test_gpu_hash_join_filter_grid(gpu_ctx, jt):
    _grid(gpu_ctx, jt)


@pytest.mark.gpu
def test_gpu_hash_join_filter_hot_key_scattered_slots(gpu_ctx):
    _hot_key(gpu_ctx)


@pytest.mark.gpu
def test_gpu_hash_join_filter_edges(gpu_ctx):
    _edges(gpu_ctx)


@pytest.mark.gpu
def test_gpu_hash_join_filter_capacity(gpu_ctx):
    _capacity(gpu_ctx)


@pytest.mark.gpu
def test_gpu_hash_join_filter_none_is_todays_path(gpu_ctx):
    _filter_none_is_todays_path(gpu_ctx)


@pytest.mark.gpu
def test_gpu_hash_join_filter_tables(gpu_ctx):
    _tables(gpu_ctx)
