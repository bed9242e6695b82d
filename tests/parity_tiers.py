"""The parity cases that both tiers run, written once.  define(T) returns {test name: function}; tests/test_emu_parity.py
and tests/test_gpu_parity.py put that dict into their own namespace (pytest collects a function where it finds it) and
supply the `ctx` fixture: the SIMT emulator's context or the device's.  What a tier runs at its own size stands next to
the case as T.pick(emu=..., gpu=...): the emulator context-switches at every wave collective, so its rows are few; the
device tier runs the sizes at which a kernel takes its multi-block paths.  The check_* helpers are in parity_cases.py;
cases that only one tier runs are in that tier's file."""
import numpy as np
import pytest

from oracle import oracle as O

from . import parity_cases as P
from . import util as U


class Tier:
    def __init__(self, name):
        self.name = name

    def pick(self, *, emu, gpu):
        """This tier's one of two values."""
        return emu if self.name == "emu" else gpu


EMU, GPU = Tier("emu"), Tier("gpu")


def rng_for(*key):
    return U.rng_for(U.kRandomSeed, *key)


def _cast_inputs(rng, n):
    x = rng.standard_normal(n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e39, -1e39, 3.4028235677973366e38,
                        1e-40, -1e-46, 1.0000000596046448, 1.00000017881393433, 2.0 ** -126, 2.0 ** -150])
    x[: min(len(special), n)] = special[: min(len(special), n)]
    x[rng.integers(0, n, size=n // 20)] *= 1e40
    x[rng.integers(0, n, size=n // 20)] *= 1e-42
    return x


def check_min_max_merge_of_two_states(amd, k, v, cut, capacity):
    """Two states over the rows before and from `cut`, merged (Merge, hash_aggregate.cc:371-399) == one state."""
    n = k.length
    dk, dv = k.to_device(amd), v.to_device(amd)
    a, b = amd.compute.GroupBySum(capacity, dk.device), amd.compute.GroupBySum(capacity, dk.device)
    a.consume_min_max(dk.slice(0, cut), dv.slice(0, cut))
    b.consume_min_max(dk.slice(cut), dv.slice(cut))
    a.merge_min_max(b.export_min_max())
    gk, gkv, gmin, gmax, gvalid = (x.cpu().numpy() for x in a.finalize_min_max())
    w = O.groupby_minmax_i64(k.values, k.valid_bitmap(), 0, v.values, v.valid_bitmap(), 0, n, True)
    key = lambda r: (r[0] is None, r[0] or 0)  # noqa: E731
    got = sorted(((int(x) if y else None, (int(c), int(d)) if e else None) for x, y, c, d, e in zip(gk, gkv, gmin, gmax, gvalid)), key=key)
    want = sorted(((int(x) if y else None, (int(c), int(d)) if e else None)
                   for x, y, c, d, e in zip(w["keys"], w["key_is_valid"], w["mins"], w["maxs"], w["valid"])), key=key)
    assert got == want


# every compaction form the dispatch can choose
FORM_CELLS = [(w, f) for w in (1, 2, 4, 8, 16) for f in (P.COMPACT_GATHER, P.COMPACT_SWEEP_PIPELINED, P.COMPACT_SWEEP_PLAIN,
                                                         P.COMPACT_SWEEP_UNALIGNED)] + [(32, P.COMPACT_GATHER)]
ROW_NUMBER_CELLS = [(2, P.COMPACT_GATHER), (2, P.COMPACT_SWEEP_PIPELINED), (2, P.COMPACT_SWEEP_PLAIN),
                    (4, P.COMPACT_GATHER), (4, P.COMPACT_SWEEP_PIPELINED), (4, P.COMPACT_SWEEP_PLAIN)]


def _form_id(cell):
    return f"W{cell[0]}-{P.COMPACT_FORM_NAMES[cell[1]]}"


def define(T):
    """The shared cases at tier T's sizes, in the order they run."""

    # ------------------------------------------------------------------ filter
    @pytest.mark.parametrize("sel", ["drop", "emit_null"])
    @pytest.mark.parametrize("n", T.pick(emu=[0, 1, 63, 64, 65, 129, 4095, 4096, 4097, 9000],
                                         gpu=[0, 1, 63, 64, 65, 4095, 4096, 4097, 262144, 262145, 1_000_003]))
    def test_filter_int64_lengths(ctx, n, sel):
        rng = rng_for("f64len", n, sel)
        v = U.random_array(rng, np.int64, n, null_p=0.1)
        m = U.random_mask(rng, n, 0.3, null_p=0.05)
        P.check_filter(ctx, v, m, sel)

    @pytest.mark.parametrize("sel", ["drop", "emit_null"])
    @pytest.mark.parametrize("true_p", [0.0, 0.1, 0.5, 0.999, 1.0])
    @pytest.mark.parametrize("vnull,mnull", T.pick(emu=[(0.0, 0.0), (0.1, 0.0), (0.0, 0.05), (0.999, 0.5), (1.0, 1.0)],
                                                   gpu=[(0.0, 0.0), (0.01, 0.0), (0.1, 0.05), (0.999, 0.5), (1.0, 1.0)]))
    def test_filter_random_grid(ctx, true_p, vnull, mnull, sel):
        """The grid of FilterRandomTest (vector_selection_test.cc:2241-2260), n scaled for the emulator, 300k rows on the
        device.  (The emulator tier knows it as test_filter_int64_probabilities.)"""
        rng = rng_for("fprob", true_p, vnull, mnull, sel)
        n = T.pick(emu=5000, gpu=300_007)
        v = U.random_array(rng, np.int64, n, null_p=vnull)
        m = U.random_mask(rng, n, true_p, null_p=mnull)
        P.check_filter(ctx, v, m, sel)

    @pytest.mark.parametrize("sel", ["drop", "emit_null"])
    @pytest.mark.parametrize("voff,moff", T.pick(emu=[(1, 0), (0, 3), (7, 13), (64, 65), (3, 4099)],
                                                 gpu=[(1, 0), (0, 3), (7, 13), (64, 65), (3, 4099), (100001, 77)]))
    def test_filter_offsets(ctx, voff, moff, sel):
        """Sliced inputs with non-zero, non-byte-aligned offsets (vector_selection_test.cc:286-302)."""
        rng = rng_for("foff", voff, moff, sel)
        n = T.pick(emu=6000, gpu=500_000)
        v = U.random_array(rng, np.int64, n, null_p=0.2, offset=voff, tail=5)
        m = U.random_mask(rng, n, 0.4, null_p=0.1, offset=moff, tail=9)
        P.check_filter(ctx, v, m, sel)

    @pytest.mark.parametrize("dtype", [np.int8, np.uint16, np.int32, np.float32, np.float64, np.uint64])
    @pytest.mark.parametrize("sel", ["drop", "emit_null"])
    def test_filter_widths(ctx, dtype, sel):
        rng = rng_for("fw", dtype, sel)
        n = T.pick(emu=8200, gpu=400_003)
        v = U.random_array(rng, dtype, n, null_p=0.1, offset=3)
        m = U.random_mask(rng, n, 0.5, null_p=0.05, offset=1)
        P.check_filter(ctx, v, m, sel, use_pyarrow=True)

    def test_filter_tuning_variants_agree(ctx):
        """The tuning knobs must never change results.  (The emulator tier knows it as
        test_filter_dense_and_batch_variants.)"""
        lib = ctx._lib.get_lib()
        rng = rng_for("fvariants")
        n = T.pick(emu=9000, gpu=2_000_003)
        v = U.random_array(rng, np.int64, n, null_p=0.1, offset=2)
        m = U.random_mask(rng, n, 0.1, null_p=0.05)
        with U.options(lib, {b"filter_batch": 1, b"filter_pipe": 0}):
            for batch in (1, 4):
                for pipe in (0, 1):
                    assert lib.arx_set_option(b"filter_batch", batch) == 0
                    assert lib.arx_set_option(b"filter_pipe", pipe) == 0
                    for sel in ("drop", "emit_null"):
                        P.check_filter(ctx, v, m, sel, use_pyarrow=False)
            # int64 under the automatic choice runs the gather form, which reads neither knob: the forms the knobs do select
            # are the aligned sweeps, of a narrow type above 25 % and of int64 with the gather form switched off
            for dtype, offset, sparse in ((np.int32, 8, -1), (np.int64, 2, 0)):
                v = U.random_array(rng, dtype, 9000, null_p=0.1, offset=offset)
                m = U.random_mask(rng, 9000, 0.5, null_p=0.05)
                dv = v.to_device(ctx)
                with U.options(lib, {b"filter_sparse": sparse}):
                    for batch in (1, 4):
                        for pipe in (0, 1):
                            assert lib.arx_set_option(b"filter_batch", batch) == 0
                            assert lib.arx_set_option(b"filter_pipe", pipe) == 0
                            for sel in ("drop", "emit_null"):
                                want = P.COMPACT_SWEEP_PIPELINED if (batch, pipe) == (4, 1) else P.COMPACT_SWEEP_PLAIN
                                assert P.compact_form_of_filter(ctx, dv, m, sel) == want, (dtype, batch, pipe, sel)
                                P.check_filter(ctx, v, m, sel, use_pyarrow=False)

    def test_filter_length_mismatch_is_invalid(ctx):
        """vector_selection_test.cc:338-341."""
        v = U.HostArray(np.array([7, 8, 9], dtype=np.int64), None, 0, 3).to_device(ctx)
        m = U.HostArray(np.zeros(0, dtype=bool), None, 0, 0).to_device(ctx)
        for sel in ("drop", "emit_null"):
            with pytest.raises(ctx.ArrowInvalid):
                ctx.compute.filter(v, m, sel)

    # ------------------------------------------------------------------ GetTakeIndices
    @pytest.mark.parametrize("sel", ["drop", "emit_null"])
    @pytest.mark.parametrize("n,off", T.pick(emu=[(0, 0), (1, 0), (100, 5), (4097, 0), (9000, 3), (70000, 1)],
                                             gpu=[(0, 0), (1, 0), (100, 5), (65535, 0), (65536, 3), (3_000_001, 1)]))
    def test_mask_to_indices(ctx, n, off, sel):
        rng = rng_for("m2i", n, off, sel)
        true_p = T.pick(emu={70000: 0.02}, gpu={}).get(n, 0.2)    # (the emulator's longest mask is sparse)
        m = U.random_mask(rng, n, true_p, null_p=0.05, offset=off, tail=3)
        P.check_mask_to_indices(ctx, m, sel)

    def test_record_batch_filter_is_take_of_indices(ctx):
        """FilterRecordBatch (vector_selection_filter_internal.cc:925-960): filter(v, m) must equal
        take(v, GetTakeIndices(m)) — the identity the reference's ValidateFilter relies on (:345-373)."""
        amd = ctx
        rng = rng_for("rb")
        n = T.pick(emu=5000, gpu=1_000_000)
        a = U.random_array(rng, np.int64, n, null_p=0.1)
        b = U.random_array(rng, np.int32, n)
        m = U.random_mask(rng, n, 0.3, null_p=0.1)
        for sel in ("drop", "emit_null"):
            rb = amd.compute.RecordBatch({"a": a.to_device(amd), "b": b.to_device(amd)})
            out = amd.compute.filter(rb, m.to_device(amd), sel)
            for name, col in (("a", a), ("b", b)):
                direct = amd.compute.filter(col.to_device(amd), m.to_device(amd), sel)
                gv, gm = out.columns[name].to_numpy()
                dv, dmk = direct.to_numpy()
                gm = np.ones(len(gv), bool) if gm is None else gm
                dmk = np.ones(len(dv), bool) if dmk is None else dmk
                assert (gm == dmk).all() and (gv[gm] == dv[dmk]).all()

    # ------------------------------------------------------------------ take
    @pytest.mark.parametrize("idx_dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32,
                                           np.uint64, np.int64])
    def test_take_index_types(ctx, idx_dtype):
        """TakeRandomTest shape (vector_selection_test.cc:2282-2315; its values 1025, indices 257 on the emulator)."""
        rng = rng_for("tk", idx_dtype)
        size = np.dtype(idx_dtype).itemsize
        nv = 100 if size == 1 else T.pick(emu=1025, gpu=30_000 if size == 2 else 1_000_000)
        v = U.random_array(rng, np.int64, nv, null_p=0.1, offset=3)
        i = U.random_array(rng, idx_dtype, T.pick(emu=257, gpu=300_001), null_p=0.1, offset=5, lo=0, hi=nv - 1)
        P.check_take(ctx, v, i)

    @pytest.mark.parametrize("dtype", [np.int8, np.int16, np.float32, np.float64])
    @pytest.mark.parametrize("vnull,inull", [(0.0, 0.0), (0.1, 0.0), (0.0, 0.3), (1.0, 0.0), (0.5, 1.0)])
    def test_take_widths_and_nulls(ctx, dtype, vnull, inull):
        rng = rng_for("tkw", dtype, vnull, inull)
        nv, ni = T.pick(emu=(3000, 1500), gpu=(300_000, 150_001))
        v = U.random_array(rng, dtype, nv, null_p=vnull)
        i = U.random_array(rng, np.int32, ni, null_p=inull, lo=0, hi=nv - 1)
        P.check_take(ctx, v, i)

    def test_take_empty_and_no_boundscheck(ctx):
        rng = rng_for("tke")
        v = U.random_array(rng, np.int64, 50)
        P.check_take(ctx, v, U.HostArray(np.zeros(0, dtype=np.int32), None, 0, 0))
        i = U.random_array(rng, np.uint32, T.pick(emu=700, gpu=70_000), lo=0, hi=49)
        P.check_take(ctx, v, i, boundscheck=False)

    @pytest.mark.parametrize("bad", [9, -1])
    def test_take_out_of_bounds(ctx, bad):
        """IndexError naming the first offender (vector_selection_test.cc:1545-1556; int_util.cc:554)."""
        v = U.HostArray(np.arange(5, dtype=np.int64), None, 0, 5)
        idx = np.array([0, bad, 0, 77], dtype=np.int64)
        P.check_take_out_of_bounds(ctx, v, U.HostArray(idx, None, 0, 4))

    def test_take_null_index_is_not_bounds_checked(ctx):
        v = U.HostArray(np.arange(5, dtype=np.int64), None, 0, 5)
        idx = U.HostArray(np.array([1, 99, 2], dtype=np.int32), np.array([True, False, True]), 0, 3)
        out = P.check_take(ctx, v, idx)
        assert out.to_pylist() == [1, None, 2]

    # ------------------------------------------------------------------ cast / compare / add
    @pytest.mark.parametrize("n,off", T.pick(emu=[(0, 0), (1, 0), (13, 1), (2048, 0), (2049, 3), (5000, 2)],
                                             gpu=[(0, 0), (1, 0), (13, 1), (2048, 0), (2049, 3), (4_000_001, 2)]))
    def test_cast_f64_f32(ctx, n, off):
        rng = rng_for("cast", n, off)
        x = _cast_inputs(rng, n + off + 2) if n else np.zeros(off + 2)
        valid = rng.random(len(x)) > 0.1 if n % 2 else None
        P.check_cast_f64_f32(ctx, U.HostArray(x, valid, off, n))

    @pytest.mark.parametrize("n,off", T.pick(emu=[(1, 0), (64, 0), (127, 1), (513, 0), (3000, 5)],
                                             gpu=[(1, 0), (64, 0), (127, 1), (513, 0), (3_000_001, 5)]))
    def test_greater_f64_array_array(ctx, n, off):
        rng = rng_for("gt", n, off)
        a = U.random_array(rng, np.float64, n, null_p=0.1, offset=off)
        b = U.random_array(rng, np.float64, n, null_p=0.1 if n % 2 else 0.0, offset=2 * off)
        a.values[rng.integers(0, len(a.values), 5)] = np.nan
        k = min(len(a.values), len(b.values))
        b.values[:k:7] = a.values[:k:7]
        P.check_greater_f64(ctx, a, b)

    def test_greater_scalar_forms_and_i64(ctx):
        rng = rng_for("gts")
        a = U.random_array(rng, np.float64, T.pick(emu=1000, gpu=1_000_000), null_p=0.1, offset=1)
        P.check_greater_f64(ctx, a, 0.25)
        P.check_greater_f64(ctx, -0.5, a)
        P.check_greater_f64(ctx, a, float("nan"))
        n = T.pick(emu=777, gpu=777_777)
        x = U.random_array(rng, np.int64, n, lo=-5, hi=5)
        y = U.random_array(rng, np.int64, n, lo=-5, hi=5)
        P.check_greater_f64(ctx, x, y)

    def test_add(ctx):
        rng = rng_for("add")
        n = T.pick(emu=3001, gpu=3_000_001)
        x = U.random_array(rng, np.int64, n, null_p=0.1, offset=1)   # full range: wraps
        y = U.random_array(rng, np.int64, n, offset=3)
        P.check_add(ctx, x, y)
        n = T.pick(emu=1000, gpu=1_000_000)
        a = U.random_array(rng, np.float64, n, null_p=0.1)
        b = U.random_array(rng, np.float64, n, null_p=0.1)
        P.check_add(ctx, a, b)

    # ------------------------------------------------------------------ sort
    @pytest.mark.parametrize("order", ["ascending", "descending"])
    @pytest.mark.parametrize("placement", ["at_end", "at_start"])
    def test_sort_small_range_with_ties_and_nulls(ctx, order, placement):
        """Stability on ties + null placement (vector_sort_test.cc:640-960)."""
        rng = rng_for("sort1", order, placement)
        a = U.random_array(rng, np.uint64, T.pick(emu=700, gpu=200_003), null_p=0.2, offset=3, lo=0, hi=7)
        P.check_sort_indices(ctx, a, order, placement)

    @pytest.mark.parametrize("dtype", [np.uint64, np.int64])
    @pytest.mark.parametrize("n", T.pick(emu=[1, 2, 255, 4096, 4097, 9000], gpu=[1, 2, 255, 4096, 4097, 1_000_003]))
    def test_sort_full_range(ctx, dtype, n):
        rng = rng_for("sort2", dtype, n)
        a = U.random_array(rng, dtype, n)
        P.check_sort_indices(ctx, a, "ascending" if n % 2 else "descending", "at_end")

    def test_sort_all_null_and_empty(ctx):
        a = U.HostArray(np.arange(10, dtype=np.uint64), np.zeros(10, dtype=bool), 0, 10)
        P.check_sort_indices(ctx, a)
        P.check_sort_indices(ctx, U.HostArray(np.zeros(0, dtype=np.uint64), None, 0, 0))

    # ------------------------------------------------------------------ group-by
    @pytest.mark.parametrize("skip_nulls,min_count", [(True, 1), (False, 1), (True, 0), (True, 3), (False, 0)])
    def test_groupby_sum_options(ctx, skip_nulls, min_count):
        """min_count / keep-nulls semantics (acero/hash_aggregate_test.cc:3481-3530)."""
        rng = rng_for("gb", skip_nulls, min_count)
        n = T.pick(emu=3000, gpu=300_000)
        k = U.random_array(rng, np.int32, n, null_p=0.05, offset=1, lo=-20, hi=20)
        v = U.random_array(rng, np.int64, n, null_p=0.2, offset=2)
        P.check_groupby_sum(ctx, k, v, skip_nulls, min_count, batches=3)

    def test_groupby_sum_wraparound_many_groups(ctx):
        rng = rng_for("gbwrap")
        n, hi, capacity = T.pick(emu=(5000, 1500, None), gpu=(2_000_000, 200_000, 1 << 19))
        k = U.random_array(rng, np.int32, n, lo=0, hi=hi)
        v = U.random_array(rng, np.int64, n)  # full int64 range: sums wrap (to_unsigned add)
        P.check_groupby_sum(ctx, k, v, capacity=capacity)

    def test_groupby_sum_golden_sum_only(ctx):
        """SumOnly (acero/hash_aggregate_test.cc:839-883) restated on int64 values: null key is its own
        group; a group whose values are all null sums to null."""
        keys = [1, 1, 2, 3, None, 1, 2, 2, None, 3]
        vals = [10, None, None, 1, 30, 5, None, 20, 40, None]
        k = U.HostArray(np.array([0 if x is None else x for x in keys], dtype=np.int32),
                        np.array([x is not None for x in keys]), 0, len(keys))
        v = U.HostArray(np.array([0 if x is None else x for x in vals], dtype=np.int64),
                        np.array([x is not None for x in vals]), 0, len(vals))
        got = P.check_groupby_sum(ctx, k, v)
        assert got == [(0, 1, 15), (0, 2, 20), (0, 3, 1), (1, 0, 70)]

    def test_hash_sum_direct_call_is_rejected(ctx):
        """acero/hash_aggregate_test.cc:646-665 / function.cc:325-326."""
        a = U.HostArray(np.arange(4, dtype=np.int64), None, 0, 4).to_device(ctx)
        g = U.HostArray(np.zeros(4, dtype=np.uint32), None, 0, 4).to_device(ctx)
        with pytest.raises(ctx.ArrowNotImplementedError, match="Direct execution of HASH_AGGREGATE"):
            ctx.compute.call_function("hash_sum", [a, g])

    @pytest.mark.parametrize("skip_nulls,min_count", [(True, 1), (False, 1), (True, 0), (True, 40), (False, 0)])
    def test_hash_sum_kernel_vtable(ctx, skip_nulls, min_count):
        """hash_sum(int64, uint32) through its HashAggregateKernel vtable: resize / consume (arrays,
        slices, broadcast + null scalars) / merge via group_id_mapping / finalize
        (hash_aggregate_numeric.cc:61-152; driven like groupby_aggregate_node.cc:210-337)."""
        n, num_groups = T.pick(emu=(3000, 37), gpu=(400000, 5003))
        P.check_hash_sum_kernel(ctx, rng_for("hsk", skip_nulls, min_count), n=n, num_groups=num_groups,
                                skip_nulls=skip_nulls, min_count=min_count)

    @pytest.mark.parametrize("num_groups,n", T.pick(emu=[(37, 6000), (5000, 20000), (300000, 20000)],
                                                    gpu=[(100, 2_000_000), (100_000, 4_000_000), (10_000_000, 8_000_000)]))
    def test_hash_sum_kernel_partitioned_by_group_id(ctx, num_groups, n):
        """The scratch form of the vtable consume (arx_hash_sum_i64_consume_ws) forced on: rows partitioned by the top bits
        of the dense group id, LDS aggregation, one flush per partition — no partition level (<= 2048 ids), one level,
        two levels; null values, hot groups, several consumes into the same state.  Same results as the per-row form."""
        lib = ctx._lib.get_lib()
        with U.options(lib, {b"groupby_partition_min_rows": 0}):
            P.check_hash_sum_kernel(ctx, rng_for("hskp", num_groups), n=n, num_groups=num_groups, null_p=0.1,
                                    use_pyarrow=False)

    def test_hash_sum_kernel_no_nulls_has_no_bitmap(ctx):
        P.check_hash_sum_kernel(ctx, rng_for("hsk0"), n=T.pick(emu=1500, gpu=200000), num_groups=11, null_p=0.0)

    @pytest.mark.parametrize("mode", [0, 1])
    def test_filter_forced_sweep_and_sparse_forms(ctx, mode):
        """filter_sparse = 0 forces the sweeping compaction, 1 the gather form, for EVERY selectivity,
        null density, offset, width and length class: both must be bit-exact (auto picks by S/N)."""
        lib = ctx._lib.get_lib()
        with U.options(lib, {b"filter_sparse": mode}):
            for n in (1, 63, 64, 65, 4095, 4096, 4097, T.pick(emu=9000, gpu=1000003)):
                for sel in ("drop", "emit_null"):
                    rng = rng_for("fform", n, sel)
                    v = U.random_array(rng, np.int64, n, null_p=0.1, offset=n % 5)
                    m = U.random_mask(rng, n, 0.3, null_p=0.05, offset=n % 3)
                    P.check_filter(ctx, v, m, sel, use_pyarrow=False)
            for true_p in (0.0, 0.02, 0.5, 1.0):
                for vnull, mnull in ((0.0, 0.0), (0.2, 0.0), (0.0, 0.3), (1.0, 1.0)):
                    for sel in ("drop", "emit_null"):
                        rng = rng_for("fform2", true_p, vnull, mnull, sel)
                        v = U.random_array(rng, np.int64, 20000, null_p=vnull, offset=7)
                        m = U.random_mask(rng, 20000, true_p, null_p=mnull, offset=13)
                        P.check_filter(ctx, v, m, sel, use_pyarrow=False)
            for dtype in (np.int8, np.uint16, np.float32, np.float64):
                rng = rng_for("fform3", str(dtype))
                v = U.random_array(rng, dtype, 12345, null_p=0.1, offset=3)
                m = U.random_mask(rng, 12345, 0.15, null_p=0.05, offset=1)
                P.check_filter(ctx, v, m, "emit_null", use_pyarrow=False)

    @pytest.mark.parametrize("l1_global,agg_chunk,bits", [(0, 1 << 16, 9), (1, 1 << 12, 9), (0, 1 << 20, 5), (1, 1 << 18, 11)])
    def test_groupby_partition_knobs(ctx, l1_global, agg_chunk, bits):
        """Tuning knobs of the partitioned consume never change results: level 1 with chunked exact offsets vs global
        cursors, the rows per LDS-aggregate work unit (how often a partition's groups are flushed)."""
        lib = ctx._lib.get_lib()
        opts = {b"groupby_partition_min_rows": 0, b"groupby_partition_bits": bits, b"groupby_l1_global": l1_global,
                b"groupby_agg_chunk_rows": agg_chunk}
        with U.options(lib, opts):
            rng = rng_for("gbpknobs", l1_global, agg_chunk, bits)
            n = T.pick(emu=20000, gpu=3000000)
            k = U.random_array(rng, np.int32, n, null_p=0.02, offset=3, lo=-2**31, hi=2**31 - 1)
            k.values[: n // 2] = k.values[: n // 2] % 1777
            v = U.random_array(rng, np.int64, n, null_p=0.1, offset=1)
            P.check_groupby_sum(ctx, k, v, skip_nulls=True, min_count=1, batches=2, use_pyarrow=False)
            k2 = U.random_array(rng, np.int32, n, lo=0, hi=50000)
            v2 = U.random_array(rng, np.int64, n)
            P.check_groupby_sum(ctx, k2, v2, use_pyarrow=False)

    def test_groupby_range_state(ctx):
        """Round 6: the range-partitioned state through its C ABI (plan / consume / merge / finalize); on the device 20x
        the emulated tier's rows, the 12288-wide partitions."""
        P.check_groupby_range_state(ctx, rng_for, scale=T.pick(emu=1, gpu=20))

    def test_groupby_lines_plan(ctx):
        """Round 6: the dense-range lines plan (write-combined whole-line scatter + direct-indexed LDS aggregate); on the
        device every case of the emulated tier at 20x the rows, plus the 12288- and 8192-wide partitions."""
        scale, wide_width = T.pick(emu=(1, False), gpu=(20, True))
        P.check_groupby_lines_plan(ctx, rng_for, scale=scale, wide_width=wide_width)

    @pytest.mark.parametrize("bits", T.pick(emu=[0, 1, 5, 9], gpu=[0, 1, 5, 9, 11]))   # (11 = a second two-level plan)
    def test_groupby_partitioned_path(ctx, bits):
        """The radix-partitioned consume (hist -> scatter level 1 [-> level 2] -> LDS aggregate -> flush)
        forced on, for one-level (bits <= 8) and two-level plans, with null keys / null values /
        wrap-around, several consume calls, and keys that overflow one partition's LDS table."""
        lib = ctx._lib.get_lib()
        with U.options(lib, {b"groupby_partition_min_rows": 0, b"groupby_partition_bits": bits}):
            rng = rng_for("gbp", bits)
            n = T.pick(emu=20000, gpu=3000003)
            k = U.random_array(rng, np.int32, n, null_p=0.02, offset=3, lo=-2**31, hi=2**31 - 1)
            k.values[: n // 2] = k.values[: n // 2] % 1777          # many repeats + distinct tail
            v = U.random_array(rng, np.int64, n, null_p=0.1, offset=1)
            P.check_groupby_sum(ctx, k, v, skip_nulls=(bits % 2 == 1), min_count=1, batches=2,
                                use_pyarrow=(bits == 9))
            # no nulls at all (the HAS_NULLS = false kernels)
            k2 = U.random_array(rng, np.int32, n, lo=0, hi=50000)
            v2 = U.random_array(rng, np.int64, n)
            P.check_groupby_sum(ctx, k2, v2, use_pyarrow=False)

    @pytest.mark.parametrize("bits", [1, 4, 8, 11])
    def test_groupby_wide_one_level_form(ctx, bits):
        """The wide one-level plan forced on (groupby_wide = 2): ONE flat scatter of register-held 24576-row tiles into
        2^bits bins of 12-byte records + 8192-slot LDS tables; null keys / null values / wrap-around, several consume
        calls, partial last tiles, more groups than the LDS tables hold (rows spill to the HBM table, still exact)."""
        lib = ctx._lib.get_lib()
        opts = {b"groupby_partition_min_rows": 0, b"groupby_wide": 2, b"groupby_partition_bits": bits,
                b"groupby_wide_agg_chunk_rows": 1 << (14 + bits % 3)}
        wide0 = lib.arx_get_counter(b"groupby_slices_wide")
        with U.options(lib, opts):
            rng = rng_for("gbwide", bits)
            n = T.pick(emu=30000, gpu=3000000)
            k = U.random_array(rng, np.int32, n, null_p=0.02, offset=3, lo=-2**31, hi=2**31 - 1)
            k.values[: n // 2] = k.values[: n // 2] % 1777          # many repeats + distinct tail
            v = U.random_array(rng, np.int64, n, null_p=0.1, offset=1)
            P.check_groupby_sum(ctx, k, v, skip_nulls=(bits % 2 == 1), min_count=1, batches=2, use_pyarrow=(bits == 4))
            # no nulls: the HAS_NULLS = false kernels
            k2 = U.random_array(rng, np.int32, n + 4097, lo=0, hi=T.pick(emu=50000, gpu=9000000))
            v2 = U.random_array(rng, np.int64, n + 4097)
            P.check_groupby_sum(ctx, k2, v2, use_pyarrow=False)
            assert lib.arx_get_counter(b"groupby_slices_wide") >= wide0 + 3, "the wide plan did not run"

    @pytest.mark.parametrize("stripe", T.pick(emu=[0, 4, 68], gpu=[0, 276]))
    @pytest.mark.parametrize("hot", [False, True])
    def test_groupby_wide_form_without_histogram(ctx, hot, stripe):
        """The wide plan with fixed rooms instead of a histogram pass: evenly spread keys fit their rooms (no overflow);
        a few hot keys outgrow one room — the slice is redone with counted partitions (null rows are not consumed twice)
        and the call's later slices stay on the counted plan.  Results exact either way — and whether the rooms lie one after
        the other or in stripes of `stripe` records (groupby_stripe)."""
        lib = ctx._lib.get_lib()
        bits, max_slice_rows, n = T.pick(emu=(6, 98304, 250000), gpu=(11, 2457600, 3200000))
        opts = {b"groupby_partition_min_rows": 0, b"groupby_wide": 2, b"groupby_partition_bits": bits, b"groupby_wide_room_min_mean": 16,
                b"groupby_stripe": stripe, b"groupby_wide_max_slice_rows": max_slice_rows}
        names = (b"groupby_slices_rooms", b"groupby_rooms_overflows")
        before = [lib.arx_get_counter(c) for c in names]
        with U.options(lib, opts):
            rng = rng_for("gbrooms", hot)
            k = U.random_array(rng, np.int32, n, null_p=0.02, lo=-2**31, hi=2**31 - 1)
            if hot:
                k.values[n // 3:] = 7            # two thirds of the rows in ONE group: its partition outgrows its room
            v = U.random_array(rng, np.int64, n, null_p=0.1)
            P.check_groupby_sum(ctx, k, v, skip_nulls=False, min_count=2, batches=1, use_pyarrow=not hot)
        rooms, overflows = (lib.arx_get_counter(c) - b for c, b in zip(names, before))
        assert rooms >= 1, "the plan without a histogram did not run"
        assert (overflows >= 1) == hot, (rooms, overflows)
        if hot:
            assert rooms == 1, "after an overflow the call stays on the counted plan"

    @pytest.mark.parametrize("distinct", T.pick(emu=[900, 0], gpu=[50000, 0]))
    def test_groupby_probe_slice_selects_the_plan(ctx, distinct):
        """A capacity that only bounds the group count from above (two-level plan) + enough rows: a HyperLogLog sketch of
        the first groupby_probe_rows keys estimates the distinct keys; few of them, seen often -> the rows run the wide plan, keys
        that do not repeat -> the two-level plan.  Same groups either way."""
        lib = ctx._lib.get_lib()
        names = (b"groupby_slices_probe", b"groupby_slices_wide", b"groupby_slices_two_level")
        before = [lib.arx_get_counter(c) for c in names]
        probe_rows, wide_max_bits = T.pick(emu=(4096, 3), gpu=(262144, 6))
        with U.options(lib, {
                b"groupby_partition_min_rows": 0,
                b"groupby_probe_rows": probe_rows,
                b"groupby_wide_max_bits": wide_max_bits,    # (so that the capacity bound alone cannot pick the wide plan)
        }):
            rng = rng_for("gbprobe", distinct)
            n = 9 * probe_rows + 1234
            hi = distinct if distinct else 2**31 - 1
            k = U.random_array(rng, np.int32, n, null_p=0.01, lo=-5 if distinct else -2**31, hi=hi)
            v = U.random_array(rng, np.int64, n, null_p=0.05)
            cap = T.pick(emu=1 << 21, gpu=1 << 21 if distinct else 1 << 23)     # (2.4M distinct keys need the larger table)
            P.check_groupby_sum(ctx, k, v, capacity=cap, batches=1, use_pyarrow=False)
            P.check_groupby_sum(ctx, k, v, capacity=cap, batches=2, use_pyarrow=False)   # second consume: table not empty
        probe, wide, two = (lib.arx_get_counter(c) - b for c, b in zip(names, before))
        assert probe == 3, "one sketch (round 3: one probe slice) per consume call"
        if distinct:
            assert (wide, two) == (3, 0), (probe, wide, two)     # round 4: the sketch aggregates nothing, every row runs the wide plan
        else:
            assert (wide, two) == (0, 3), (probe, wide, two)

    # ------------------------------------------------------------------ the MSD / wide sort forms
    @pytest.mark.parametrize("fused", [1, 0])
    @pytest.mark.parametrize("global_bits", [14, 4, -14])
    def test_sort_msd_hybrid_path(ctx, global_bits, fused):
        """The MSD-hybrid sort forced on (two global levels [+ the in-bucket level when the global
        bits are capped] + the windowed final ranking): full-range keys, heavy ties (bucket overflow ->
        LSD fallback), nulls (prep + MSD), descending, signed."""
        lib = ctx._lib.get_lib()
        opts = {b"sort_msd": 1, b"sort_msd_fused": fused}   # fused 1: LDS-resident bucket finish; 0: local + windowed final
        if global_bits < 0:   # the segmented form: an extra level on the top bits, then one pipeline per segment
            global_bits = -global_bits
            opts[b"sort_msd_segment_rows"] = 4096
            # beyond the segment size the wide two-level form (run_msd_sort_wide) runs first; fused = 0 switches it off so
            # that the segmented form itself stays covered
            opts[b"sort_msd_wide"] = fused
        opts[b"sort_msd_global_bits"] = global_bits
        with U.options(lib, opts):
            n = T.pick(emu=14000, gpu=6000011)   # (the emulator runs every workgroup as fibers on one core)
            rng = rng_for("msd", global_bits, fused)
            for dtype, order, placement, null_p in ((np.uint64, "ascending", "at_end", 0.0),
                                                   (np.int64, "descending", "at_start", 0.03),
                                                   *T.pick(emu=(), gpu=((np.uint64, "descending", "at_end", 0.0),))):
                a = U.random_array(rng, dtype, n, null_p=null_p, offset=3)
                a.values[a.offset:a.offset + n - 1:5] = a.values[a.offset + 1:a.offset + n:5]  # ties
                P.check_sort_indices(ctx, a, order, placement, use_pyarrow=(dtype == np.int64))
            ties = U.random_array(rng, np.uint64, n, lo=0, hi=7)       # 7 distinct keys: buckets overflow
            P.check_sort_indices(ctx, ties, "ascending", "at_end", use_pyarrow=False)
            small = U.random_array(rng, np.uint64, 300)
            P.check_sort_indices(ctx, small, "ascending", "at_end", use_pyarrow=False)

    @pytest.mark.parametrize("shift,gap2,b2max", T.pick(
        emu=[(2, 1, 12), (2, 0, 12), (0, 1, 12), (0, 0, 12), (2, 1, 0), (2, 0, 0), (0, 1, 0), (0, 0, 0)],
        gpu=[(4, 1, 12), (2, 1, 12), (4, 0, 12), (0, 1, 12), (0, 0, 12), (4, 1, 0), (0, 0, 0)]))
    def test_sort_wide_sampled_level1(ctx, shift, gap2, b2max):
        lib = ctx._lib.get_lib()
        n = T.pick(emu=300_000, gpu=6_000_011)
        failed = P.check_sort_wide_sampled(ctx, lib, rng_for("wide-sampled", shift, gap2), n, shift, gap2, b2max)
        if shift == 0 and gap2 == 0:
            assert failed == 0   # exact counts never overflow
        if shift and T.pick(emu=True, gpu=False):
            # at the emulator's size this sample misses the crafted inputs: both with the even split, at least one with the
            # few large level-1 buckets the 12-bit level 2 leaves at this size
            assert failed == 2 if b2max == 0 else failed >= 1

    # (the default (24, 16) runs in the tests around this one)
    @pytest.mark.parametrize("rpt", T.pick(emu=[(8, 24), (16, 16)], gpu=[(8, 8), (8, 24), (16, 16), (24, 24)]))
    def test_sort_wide_register_staged_tiles(ctx, rpt):
        """Level-1 / level-2 scatter tiles of 8 (LDS-resident), 16 and 24 (register-staged) rows per thread: ragged last
        tiles, level-2 tiles that end inside a round of the LDS buffer, rooms that overflow (sorted / blocky inputs)."""
        lib = ctx._lib.get_lib()
        # the 256-thread bucket finish takes over whenever every bucket fits it (always, at the emulator's sizes): one case without
        with U.options(lib, {
                b"sort_msd_tiny_bucket": {16: 0, 8: 1}.get(rpt[0], 2),   # (256- / 512-thread bucket finish)
                b"sort_msd_bucket_cpt": 8 if rpt[1] == 16 else 4,   # sub-bucket counters per thread of the finish
        }):
            n, shift = T.pick(emu=(70_000, 2), gpu=(3_000_011, 4))
            P.check_sort_wide_sampled(ctx, lib, rng_for("wide-rpt", *rpt), n, shift, 1, 12, rpt=rpt, typed_keys=True)
            for n_bins in T.pick(emu=(), gpu=(2_000_003,)):   # (each forced partition is a workgroup of fibers under the emulator)
                P.check_sort_wide_many_bins(ctx, lib, rng_for("wide-rpt-bins", *rpt), n_bins, 16, 12, combos=((0, 0), (2, 1)), rpt=rpt)

    @pytest.mark.parametrize("bits,b2max", T.pick(emu=[(13, 12)], gpu=[(13, 12), (16, 12), (20, 12), (19, 11), (19, 0)]))
    def test_sort_wide_many_level2_bins(ctx, bits, b2max):
        # (each forced partition is a workgroup of fibers under the emulator: one shape, the default size mode — sampled
        #  level 1, fixed level-2 rooms; the device tier runs the rest, with the checker's own combos)
        n, kw = T.pick(emu=(30_000, {"combos": ((2, 1),)}), gpu=(2_500_003, {}))
        P.check_sort_wide_many_bins(ctx, ctx._lib.get_lib(), rng_for("wide-bins", bits, b2max), n, bits, b2max, **kw)

    def test_null_count_bookkeeping(ctx):
        P.check_null_count_bookkeeping(ctx, rng_for("nullcount"))

    @pytest.mark.parametrize("msd", [0, 1])
    @pytest.mark.parametrize("dtype", [np.uint32, np.int32, np.float64, np.float32])
    def test_sort_32bit_and_float_keys(ctx, dtype, msd):
        """array_sort_indices on the other fixed-width key types: 32-bit integers (4 LSD passes), floats
        with NaNs as null-likes next to the nulls whatever the order, -0.0 tying with 0.0, infinities."""
        lib = ctx._lib.get_lib()
        with U.options(lib, {b"sort_msd": 1 if msd else 0}):
            rng = rng_for("sort32f", str(dtype), msd)
            n = T.pick(emu=4000, gpu=5000003)   # (emulator: fibers on one core)
            for order, placement, null_p in (("ascending", "at_end", 0.05), ("descending", "at_start", 0.05),
                                             *T.pick(emu=(), gpu=(("descending", "at_end", 0.0),))):
                a = U.random_array(rng, dtype, n, null_p=null_p, offset=2)
                v = a.values
                if np.dtype(dtype).kind == "f":
                    v[::7] = np.nan
                    v[::11] = 0.0
                    v[1::11] = -0.0
                    v[::13] = np.inf
                    v[5::13] = -np.inf
                    v[::3] = np.round(v[::3])          # ties
                else:
                    v[::3] = v[::3] % 17               # ties
                P.check_sort_indices(ctx, a, order, placement)

    @pytest.mark.parametrize("dtype", [np.float64, np.uint64, np.int32])
    def test_sort_msd_sampled_splitters(ctx, dtype):
        """The sampled-splitter form of the MSD sort forced on: skewed keys (normal floats, clustered
        integers), duplicates-heavy columns (a bucket overflows -> LSD fallback), nulls, descending."""
        lib = ctx._lib.get_lib()
        with U.options(lib, {b"sort_msd_sampled": 2}):
            rng = rng_for("sampled", str(dtype))
            n = T.pick(emu=9000, gpu=4000003)
            for order, placement, null_p in (("ascending", "at_end", 0.0), ("descending", "at_start", 0.04)):
                a = U.random_array(rng, dtype, n, null_p=null_p, offset=1)
                v = a.values
                if np.dtype(dtype).kind == "f":
                    v[::50] = np.nan
                    v[::17] = -0.0
                elif np.dtype(dtype) == np.uint64:
                    v[:] = (np.abs(rng.standard_normal(len(v))) * 1e6).astype(np.uint64) + (v % 3) * 10**12   # clustered
                else:
                    v[:] = (rng.standard_normal(len(v)) * 1000).astype(np.int32)                               # many ties
                P.check_sort_indices(ctx, a, order, placement, use_pyarrow=(order == "ascending"))
            dup = U.random_array(rng, dtype, n, lo=None if np.dtype(dtype).kind == "f" else 0, hi=None if np.dtype(dtype).kind == "f" else 3)
            if np.dtype(dtype).kind == "f":
                dup.values[:] = np.round(dup.values)
            P.check_sort_indices(ctx, dup, "ascending", "at_end", use_pyarrow=False)

    # ------------------------------------------------------------------ binary / utf8 take + filter
    @pytest.mark.parametrize("idx_dtype", [np.uint8, np.int16, np.uint32, np.int64])
    @pytest.mark.parametrize("vnull,inull", [(0.0, 0.0), (0.2, 0.0), (0.0, 0.1), (0.3, 0.3)])
    def test_binary_take(ctx, idx_dtype, vnull, inull):
        """TestTakeKernelWithString (vector_selection_test.cc): values and index nulls, all index types."""
        rng = rng_for("btake", idx_dtype, vnull, inull)
        nv = 100 if np.dtype(idx_dtype).itemsize == 1 else T.pick(emu=3000, gpu=30_000)
        v = U.random_binary(rng, nv, null_p=vnull, offset=3, tail=2, utf8=True)
        i = U.random_array(rng, idx_dtype, T.pick(emu=5000, gpu=200_003), null_p=inull, offset=1, lo=0, hi=nv - 1)
        P.check_binary_take(ctx, v, i)

    @pytest.mark.parametrize("m", T.pick(emu=[0, 1, 63, 64, 65, 4095, 4096, 4097, 8193],
                                         gpu=[0, 1, 63, 64, 65, 4095, 4096, 4097, 1_000_003]))
    def test_binary_take_lengths(ctx, m):
        rng = rng_for("btakelen", m)
        nv = T.pick(emu=500, gpu=5000)
        v = U.random_binary(rng, nv, null_p=0.1, max_len=40)
        i = U.random_array(rng, np.int32, m, null_p=0.1, lo=0, hi=nv - 1)
        P.check_binary_take(ctx, v, i)

    @pytest.mark.parametrize("sel", ["drop", "emit_null"])
    @pytest.mark.parametrize("true_p,vnull,mnull", T.pick(emu=[(0.0, 0.1, 0.0), (0.3, 0.0, 0.0), (0.5, 0.2, 0.1), (1.0, 0.1, 0.05)],
                                                          gpu=[(0.0, 0.1, 0.0), (0.1, 0.0, 0.0), (0.5, 0.2, 0.1), (1.0, 0.1, 0.05)]))
    def test_binary_filter(ctx, sel, true_p, vnull, mnull):
        """TestFilterKernelWithString / FilterRandomTest on utf8 (vector_selection_test.cc)."""
        rng = rng_for("bfilter", sel, true_p, vnull, mnull)
        n = T.pick(emu=6000, gpu=300_007)
        v = U.random_binary(rng, n, null_p=vnull, offset=5, tail=3)
        m = U.random_mask(rng, n, true_p, null_p=mnull, offset=2, tail=1)
        P.check_binary_filter(ctx, v, m, sel)

    def test_binary_take_many_tiny_values(ctx):
        """0/1-byte values: a 16 KiB output chunk spans many more rows than one LDS batch holds."""
        rng = rng_for("btaketiny")
        v = U.random_binary(rng, 4000, null_p=0.1, max_len=1, empty_p=0.5)
        i = U.random_array(rng, np.int32, T.pick(emu=70000, gpu=2000000), null_p=0.05, lo=0, hi=3999)
        P.check_binary_take(ctx, v, i)

    def test_add_and_greater_with_a_scalar_operand(ctx):
        P.check_scalar_operand_ops(ctx, rng_for("scalarops"), n=T.pick(emu=5000, gpu=300007))

    # ------------------------------------------------------------------ hash_min / hash_max on the fused table
    @pytest.mark.parametrize("skip_nulls", [True, False])
    @pytest.mark.parametrize("knull,vnull,batches,groups", T.pick(
        emu=[pytest.param(0.0, 0.0, 1, 40, id="0.0-0.0-1"), pytest.param(0.05, 0.2, 3, 40, id="0.05-0.2-3"),
             pytest.param(1.0, 0.5, 1, 40, id="1.0-0.5-1"), pytest.param(0.1, 1.0, 2, 40, id="0.1-1.0-2")],   # (40: keys in -40 .. 40)
        gpu=[(0.0, 0.0, 1, 1000), (0.02, 0.2, 3, 100_000), (1.0, 0.5, 1, 10), (0.1, 1.0, 2, 50)]))
    def test_groupby_min_max(ctx, skip_nulls, knull, vnull, batches, groups):
        """GroupedMinMaxImpl (hash_aggregate.cc:330-419): extrema at the int64 edges, null keys as one
        group, groups whose values are all null, several consume calls."""
        rng = rng_for("gbminmax", skip_nulls, knull, vnull, batches)
        n = T.pick(emu=4000, gpu=400_003)
        k = U.random_array(rng, np.int32, n, null_p=knull, offset=2, lo=-groups, hi=groups)
        v = U.random_array(rng, np.int64, n, null_p=vnull, offset=1)
        v.values[5:9] = [2**63 - 1, -2**63, 0, -1]
        P.check_groupby_min_max(ctx, k, v, skip_nulls, batches=batches, use_pyarrow=(groups <= 1000))

    @pytest.mark.parametrize("skip_nulls,min_count,knull,vnull,batches", [(True, 1, 0.0, 0.0, 1), (False, 1, 0.05, 0.2, 3),
                                                                            (True, 0, 0.1, 1.0, 2), (True, 3, 0.02, 0.5, 1)])
    def test_groupby_mean_int64(ctx, skip_nulls, min_count, knull, vnull, batches):
        """hash_mean(int64) (GroupedMeanImpl: doubles summed in row order) = (double)sum / count bit for bit while every
        partial sum is an exact integer; all-null groups, min_count = 0 (0 / 0 = NaN), !skip_nulls."""
        rng = rng_for("gmean", skip_nulls, min_count, knull, vnull, batches)
        n = T.pick(emu=6000, gpu=2000000)
        k = U.random_array(rng, np.int32, n, null_p=knull, offset=2, lo=-40, hi=40)
        v = U.random_array(rng, np.int64, n, null_p=vnull, offset=1, lo=-2**31, hi=2**31)
        P.check_groupby_mean(ctx, k, v, skip_nulls, min_count, batches=batches)

    def test_groupby_mean_declines_where_the_reference_is_order_dependent(ctx):
        """Values near 2^62: the reference's double partial sums are rounded differently for different row orders,
        so there is nothing to be bit-exact with — NotImplemented with the reason, never a wrong number."""
        rng = rng_for("gmean-big")
        k = U.random_array(rng, np.int32, 5000, lo=0, hi=10)
        v = U.random_array(rng, np.int64, 5000, lo=2**60, hi=2**62)
        P.check_groupby_mean(ctx, k, v, expect_decline=True)

    @pytest.mark.parametrize("in_name", list(P.NUMERIC_TYPES))
    def test_cast_every_numeric_pair(ctx, in_name):
        """CastIntegerToInteger / CastFloatingToInteger / CastIntegerToFloating / CastFloatingToFloating
        (scalar_cast_numeric.cc:46-60, 190-207, 270-279) for all 10 x 10 numeric pairs, safe and unsafe."""
        rng = rng_for("castpair", in_name)
        for out_name in P.NUMERIC_TYPES:
            if out_name != in_name:
                P.check_cast_numeric_pair(ctx, rng, in_name, out_name, n=T.pick(emu=3000, gpu=300000))

    def test_cast_at_the_type_boundaries(ctx):
        """All 100 pairs on the values at their own limits -- hi, hi + 1, lo, lo - 1, +-2^24, +-2^53, 2^31, 2^63, 2^64, NaN, inf,
        -0.0, DBL_MAX: the decision, the whole error text and the result bits, safe and unsafe (P.check_cast_boundaries)."""
        assert P.check_cast_boundaries(ctx) > 1500

    @pytest.mark.parametrize("pair", P.LONE_OFFENDER_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
    def test_cast_names_a_lone_offender_wherever_it_is(ctx, pair):
        """One failing row at the wave / block / tile / tail edges of a 4099-row array, under a null, and two of them in
        different blocks (the atomicMin over blocks), for one pair per checking path of arx_cast_numeric."""
        P.check_cast_lone_offender(ctx, pair)

    @pytest.mark.parametrize("dtype", ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"])
    def test_checked_arithmetic_with_one_overflowing_row(ctx, dtype):
        """add / subtract / multiply (+ _checked) with a single overflowing row at every edge position and both slice offsets,
        array x array and both scalar orders; nulls on either side hide it."""
        P.check_arith_lone_overflow(ctx, np.dtype(dtype))

    def test_add_pair_kernel_rows_and_tail(ctx):
        """Unchecked int64 / float64 add (the pair-loading add_kernel) on rows that all differ, odd length, both offsets."""
        P.check_add_pair_kernel_tail(ctx)

    @pytest.mark.parametrize("dtype", ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"])
    def test_divide_error_of_the_later_row(ctx, dtype):
        """A zero divisor and min / -1 in different blocks, in both orders: divide_checked names the later one."""
        P.check_divide_ordering(ctx, np.dtype(dtype))

    @pytest.mark.parametrize("dtype", list(P.NUMERIC_TYPES))
    def test_compare_and_arithmetic_over_the_whole_type(ctx, dtype):
        """Operands from the type's edges and its whole range (an unsigned comparison done as signed fails here)."""
        P.check_compare_whole_range(ctx, rng_for("whole-range", dtype), P.NUMERIC_TYPES[dtype])

    @pytest.mark.parametrize("key_dtype", [np.int8, np.uint16, np.uint32, np.int64, np.uint64])
    def test_groupby_sum_other_key_and_value_types(ctx, key_dtype):
        rng = rng_for("gbtyped", str(key_dtype))
        for value_dtype in (np.int8, np.int32, np.uint32, np.uint64, np.int64):
            P.check_groupby_sum_typed(ctx, rng, key_dtype, value_dtype, n=T.pick(emu=4000, gpu=400000))

    def test_groupby_declines_what_it_cannot_reproduce(ctx):
        """64-bit keys beyond the int32 range (the device table holds 32-bit keys) and floating-point sums (row-order
        double accumulation in the reference) are NotImplemented with the reason — never a wrong answer."""
        amd = ctx
        op = amd.compute.GroupBySum(64)
        with pytest.raises(NotImplementedError, match="beyond the int32 range"):
            op.consume(amd.Array.from_numpy(np.array([1, 2**40], dtype=np.int64)), amd.Array.from_numpy(np.array([1, 2], dtype=np.int64)))
        op = amd.compute.GroupBySum(64)
        with pytest.raises(NotImplementedError, match="row order"):
            op.consume(amd.Array.from_numpy(np.array([1, 2], dtype=np.int32)), amd.Array.from_numpy(np.array([1.0, 2.0])))

    @pytest.mark.parametrize("dtype", [np.bool_, np.int8, np.uint16, np.int32, np.uint64, np.int64, np.float32, np.float64])
    def test_indices_nonzero(ctx, dtype):
        """IndicesNonZero (kernels/vector_selection.cc:352): uint64 positions of the valid, non-zero elements vs pyarrow."""
        import pyarrow as pa
        import pyarrow.compute as pc

        rng = rng_for("nonzero", str(dtype))
        for n in (0, 5, 70000, T.pick(emu=100001, gpu=3000001)):
            x = rng.integers(0, 3, n).astype(dtype) if dtype != np.bool_ else rng.random(n) < 0.3
            valid = rng.random(n) > 0.1
            got = ctx.compute.indices_nonzero(ctx.Array.from_numpy(x, valid if n else None))
            want = pc.indices_nonzero(pa.array(x, mask=(~valid) if n else None))
            assert got.type.name == "uint64" and np.array_equal(got.to_numpy()[0], want.to_numpy()), (dtype, n)

    @pytest.mark.parametrize("dtype", [np.int64, np.uint64, np.int32, np.uint32, np.float64, np.float32])
    def test_golden_sort_and_sum_only_replay(ctx, dtype):
        """The reference's own known-answer tests for the two sharded paths (vector_sort_test.cc:640-724,
        acero/hash_aggregate_test.cc:839-883; tests/golden/reference_vectors.json) replayed on the kernels."""
        import json
        import os

        gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.json")))
        assert P.replay_golden_sort(ctx, gold, dtype) >= 20
        P.replay_golden_sum_only(ctx, gold)

    @pytest.mark.parametrize("run_end_type", ["int16", "int32", "int64"])
    def test_filter_with_a_run_end_encoded_mask(ctx, run_end_type):
        """array_filter(values, run_end_encoded<boolean>) (vector_selection_filter_internal.cc:1090): sliced masks, null run
        values, DROP and EMIT_NULL, vs the reference (pyarrow)."""
        import pyarrow as pa
        import pyarrow.compute as pc

        amd = ctx
        rng = rng_for("reemask", run_end_type)
        ret = {"int16": pa.int16(), "int32": pa.int32(), "int64": pa.int64()}[run_end_type]
        for n in T.pick(emu=(1, 63, 64, 1000, 20000), gpu=(1, 64, 20000, 3000001)):
            if run_end_type == "int16" and n > 30000:
                continue
            lens = rng.integers(1, 200, max(8, n // 50))
            ends = np.cumsum(lens)
            ends = ends[ends < n + 300]
            if len(ends) == 0 or ends[-1] < n + 7:
                ends = np.append(ends, n + 7)
            rv = pa.array(rng.random(len(ends)) < 0.4, mask=rng.random(len(ends)) < 0.2)
            ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends.astype(ret.to_pandas_dtype())), rv).slice(5, n)
            vals = pa.array(rng.integers(-2**62, 2**62, n), mask=rng.random(n) < 0.1)
            for sel in ("drop", "emit_null"):
                want = pc.filter(vals, ree, null_selection_behavior=sel)
                got = amd.compute.filter(amd.Array.from_pyarrow(vals), amd.array.RunEndEncoded.from_pyarrow(ree), sel)
                assert got.to_pyarrow().equals(want), (run_end_type, n, sel)

    @pytest.mark.parametrize("null_p,offset", T.pick(emu=[(0.0, 0), (0.05, 3)], gpu=[(0.0, 0), (0.05, 3), (1.0, 1)]))
    def test_unique_and_value_counts(ctx, null_p, offset):
        """UniqueAction / ValueCountsAction (vector_hash.cc): first-appearance order from the fused table."""
        rng = rng_for("unique", null_p, offset)
        n, span = T.pick(emu=(3000, 200), gpu=(500003, 60000))
        a = U.random_array(rng, np.int32, n, null_p=null_p, offset=offset, tail=2, lo=-span, hi=span)
        P.check_unique_and_value_counts(ctx, a)
        P.check_unique_and_value_counts(ctx, U.random_array(rng, np.int32, 0))
        for one in T.pick(emu=(), gpu=(1,)):    # (every sort launch costs seconds under the emulator)
            P.check_unique_and_value_counts(ctx, U.random_array(rng, np.int32, one, null_p=null_p))

    @pytest.mark.parametrize("lnull,rnull,loff,roff", [(0.0, 0.0, 0, 0), (0.2, 0.0, 3, 0), (0.0, 0.3, 0, 65), (0.3, 0.3, 7, 13), (1.0, 0.5, 1, 2)])
    def test_kleene_and_or_invert(ctx, lnull, rnull, loff, roff):
        """KleeneAndOp / KleeneOrOp / InvertOp (scalar_boolean.cc): the full truth table incl. nulls,
        sliced operands with different bit offsets."""
        rng = rng_for("kleene", lnull, rnull, loff, roff)
        n = T.pick(emu=5000, gpu=1000003)
        left = U.random_mask(rng, n, 0.5, null_p=lnull, offset=loff, tail=3)
        right = U.random_mask(rng, n, 0.4, null_p=rnull, offset=roff, tail=5)
        P.check_kleene_and_invert(ctx, left, right)
        P.check_kleene_and_invert(ctx, U.random_mask(rng, 0, 0.5), U.random_mask(rng, 0, 0.5))

    def test_compare_family(ctx):
        """Equal ... LessEqual (scalar_compare.cc:38-64): int64 and float64 incl. NaN / signed zeros / infinities."""
        P.check_compare_family(ctx, rng_for("cmpfamily"), n=T.pick(emu=3000, gpu=300007))

    def test_subtract_multiply_and_checked_arithmetic(ctx):
        """Subtract / Multiply / *Checked (base_arithmetic_internal.h): wrap-around vs "overflow" on valid slots only."""
        P.check_arithmetic(ctx, rng_for("arith"), n=T.pick(emu=3000, gpu=300007))

    def test_integer_casts(ctx):
        """CastIntegerToInteger (scalar_cast_numeric.cc:46-54) + IntegersInRange's first-offender message."""
        n = T.pick(emu=4000, gpu=400003)
        P.check_integer_casts(ctx, rng_for("intcast"), n=n)
        P.check_cast_i64_f64(ctx, rng_for("i64f64"), n=n)

    @pytest.mark.parametrize("null_p,offset", [(0.0, 0), (0.07, 3)])
    def test_dictionary_encode(ctx, null_p, offset):
        """DictEncodeAction (vector_hash.cc:173-270): MASK and ENCODE null handling, first-appearance dictionary."""
        rng = rng_for("dictenc", null_p, offset)
        n, span = T.pick(emu=(2500, 150), gpu=(500003, 40000))
        a = U.random_array(rng, np.int32, n, null_p=null_p, offset=offset, tail=2, lo=-span, hi=span)
        P.check_dictionary_encode(ctx, a)
        P.check_dictionary_encode(ctx, U.random_array(rng, np.int32, 0))

    def test_scalar_aggregates_int64(ctx):
        """SumImpl / CountImpl / MinMaxImpl (aggregate_basic.inc.cc): wrap-around sum, options, batches."""
        P.check_scalar_aggregates(ctx, rng_for("scalaragg"), n=T.pick(emu=6000, gpu=1000003))

    @pytest.mark.parametrize("idx_dtype", [np.uint8, np.int32, np.int64])
    @pytest.mark.parametrize("vnull,inull,voff", [(0.0, 0.0, 0), (0.2, 0.1, 5), (1.0, 0.5, 67)])
    def test_boolean_values_take_and_filter(ctx, idx_dtype, vnull, inull, voff):
        """filter / take on BOOLEAN values (1-bit Gather, gather_internal.h; PrimitiveFilter's bit-width-1 case)."""
        rng = rng_for("booltake", str(idx_dtype), vnull, inull, voff)
        n = T.pick(emu=5000, gpu=500003)
        nv = 200 if np.dtype(idx_dtype).itemsize == 1 else n
        v = U.random_mask(rng, nv, 0.5, null_p=vnull, offset=voff, tail=3)
        i = U.random_array(rng, idx_dtype, n, null_p=inull, offset=1, lo=0, hi=nv - 1)
        m = U.random_mask(rng, nv, 0.3, null_p=0.05, offset=2)
        P.check_boolean_take_and_filter(ctx, v, i, m)

    @pytest.mark.parametrize("kind", ["int64", "int8", "bool", "utf8", "binary_nonull"])
    def test_concat_arrays(ctx, kind):
        """Concatenate (array/concatenate.cc): sliced chunks with and without validity, empty chunks, bit offsets
        that are not multiples of 8 / 64."""
        rng = rng_for("concat", kind)
        n3, n5 = T.pick(emu=(130, 300), gpu=(130001, 300000))
        specs = [(77, 0.2, 3), (0, 0.0, 0), (1, 0.0, 0), (n3, 0.0, 65), (64, 1.0, 7), (n5, 0.1, 0), (5, 0.5, 1)]
        if kind == "bool":
            chunks = [U.random_mask(rng, n, 0.5, null_p=p, offset=o, tail=2) for n, p, o in specs]
        elif kind in ("utf8", "binary_nonull"):
            chunks = [U.random_binary(rng, n, null_p=0.0 if kind == "binary_nonull" else p, offset=o, tail=2, utf8=kind == "utf8")
                      for n, p, o in specs]
        else:
            chunks = [U.random_array(rng, np.dtype(kind).type, n, null_p=p, offset=o, tail=2) for n, p, o in specs]
        P.check_concat_arrays(ctx, chunks)
        P.check_concat_arrays(ctx, chunks[1:2])            # one empty chunk
        P.check_concat_arrays(ctx, [chunks[3]])            # a single sliced chunk without nulls

    @pytest.mark.parametrize("null_placement", ["at_end", "at_start"])
    def test_order_by_several_keys(ctx, null_placement):
        """OrderByNode::DoFinish (acero/order_by_node.cc:100-108) with two and three sort keys of mixed direction and per-key
        null placement (few distinct values per key so that every later key and the input order decide ties), a float key
        with NaNs, payload columns riding along."""
        rng = rng_for("orderby", null_placement)
        sizes = T.pick(emu=[(300, 3), (0, 0), (157, 0), (41, 5)], gpu=[(32_768, 3), (0, 0), (32_768, 0), (20_001, 5)])
        span0, span1 = T.pick(emu=(3, 4), gpu=(30, 40))

        def col(make):
            return [make(n, o) for n, o in sizes]

        def fkey(n, o):
            a = U.random_array(rng, np.float64, n, null_p=0.1, offset=o, tail=1)
            a.values[:] = np.round(a.values * 2) / 2
            a.values[rng.random(len(a.values)) < 0.1] = np.nan
            return a

        k0 = col(lambda n, o: U.random_array(rng, np.int32, n, null_p=0.1, offset=o, tail=1, lo=-span0, hi=span0))
        k1 = col(lambda n, o: U.random_array(rng, np.int64, n, null_p=0.1, offset=o, tail=1, lo=0, hi=span1))
        k2 = col(fkey)
        payload = col(lambda n, o: U.random_array(rng, np.int64, n, null_p=0.2, offset=o, tail=1))
        strs = col(lambda n, o: U.random_binary(rng, n, null_p=0.1, offset=o, tail=1, utf8=True))
        flags = col(lambda n, o: U.random_mask(rng, n, 0.5, null_p=0.1, offset=o, tail=1))
        cols = [k0, k1, k2, payload, strs, flags]
        two_keys, three_keys = [(0, "ascending"), (1, "descending")], [(2, "descending"), (0, "descending"), (1, "ascending")]
        # (every sort launch costs seconds under the emulator: there the two placements share the key sets between them)
        for keys in T.pick(emu={"at_end": [two_keys, [(1, "ascending")]], "at_start": [three_keys]}[null_placement],
                           gpu=[two_keys, three_keys]):
            P.check_order_by(ctx, cols, keys, null_placement)
        other = "at_start" if null_placement == "at_end" else "at_end"
        P.check_order_by(ctx, cols, [(0, "descending"), (2, "ascending")], [null_placement, other])     # per-key placement

    def test_divide_and_divide_checked(ctx):
        """Divide / DivideChecked (base_arithmetic_internal.h:366-424): truncating int64 division, zero divisors, INT64_MIN / -1,
        IEEE doubles, the last failing valid slot names the error, nulls hide failures."""
        P.check_divide(ctx, rng_for("divide"), n=T.pick(emu=3000, gpu=300007))

    @pytest.mark.parametrize("dtype", ["int8", "uint8", "int16", "uint16", "int32", "uint32", "uint64", "float32"])
    def test_divide_on_the_other_numeric_types(ctx, dtype):
        """arx_divide_numeric: the same Call bodies per element type (min / -1 of the type's own width, unsigned types fail
        only on a zero divisor — DivideWithOverflowGeneric, util/int_util_overflow.h:124-138)."""
        P.check_divide(ctx, rng_for("divide-" + dtype), n=T.pick(emu=1500, gpu=200003), dtypes=(np.dtype(dtype),))

    # ------------------------------------------------------------------ the device Grouper (csrc/grouper.hip)
    @pytest.mark.parametrize("section,combos", [("grouper_numeric_key", None), ("grouper_floating_point_key", None),
                                                ("grouper_multiple_int_keys", T.pick(emu=40, gpu=60))])
    def test_reference_grouper_golden_vectors(ctx, section, combos):
        """grouper_test.cc's own expectations (exact ids in first-appearance order, uniques, Lookup nulls) on the device
        Grouper; the three-column case samples the type combinations (every width pair still occurs)."""
        import json
        import os

        gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_vectors.json")))
        assert P.replay_golden_grouper(gold, section, P.device_grouper_factory(ctx), combos) > 0

    @pytest.mark.parametrize("dtypes,n,card,null_p,batches", T.pick(
        emu=[((np.int64,), 5000, 700, 0.05, 1), ((np.int64,), 5000, 4999, 0.0, 3), ((np.uint64,), 3000, 5, 0.3, 2),
             ((np.int32, np.int32), 6000, 900, 0.1, 2), ((np.int64, np.int64), 4000, 300, 0.1, 1),
             ((np.int8, np.int16, np.int32, np.int64), 3000, 2500, 0.05, 4), ((np.float64, np.uint8), 2000, 50, 0.2, 1),
             ((np.int16,), 0, 1, 0.0, 1), ((np.uint8,) * 8, 2000, 100, 0.1, 2),
             # rows wider than one 16-byte table: the chain of tables (level s keys = id of level s-1 ++ the next columns;
             # on the device these run in test_gpu_group_keys.py)
             ((np.int64, np.int64, np.int64), 4000, 600, 0.1, 2), ((np.int64,) * 5, 3000, 2900, 0.05, 3),
             ((np.uint8,) * 20, 2500, 40, 0.2, 2), ((np.int32, np.int64, np.int16, np.float64, np.int8, np.int64), 3000, 30, 0.3, 1),
             ((np.int64, np.int64, np.int32), 0, 1, 0.0, 1)],
        gpu=[((np.int64,), 2_000_000, 300_000, 0.05, 1), ((np.int64,), 1_000_000, 999_999, 0.0, 3),
             ((np.uint64,), 3_000_000, 5, 0.3, 2), ((np.int32, np.int32), 2_000_000, 900, 0.1, 2),
             ((np.int64, np.int64), 1_000_000, 200_000, 0.1, 1), ((np.int8, np.int16, np.int32, np.int64), 500_000, 400_000, 0.05, 4),
             ((np.float64, np.uint8), 300_000, 50, 0.2, 1), ((np.int16,), 0, 1, 0.0, 1), ((np.uint8,) * 8, 400_000, 100, 0.1, 2)]))
    def test_grouper_ids_uniques_lookup(ctx, dtypes, n, card, null_p, batches):
        P.check_grouper(ctx, rng_for("grouper", len(dtypes), n, card, batches), dtypes, n, card, null_p, batches)

    @pytest.mark.parametrize("dtypes,n,card,null_p", T.pick(
        emu=[((np.int64,), 6000, 500, 0.05), ((np.int32, np.int32), 6000, 800, 0.1), ((np.int64, np.int16), 4000, 3500, 0.0),
             ((np.int64, np.int64, np.int64), 4000, 12, 0.1)],
        # (device sizes: the row-by-row checker is what takes the time here)
        gpu=[((np.int64,), 600_000, 200_000, 0.05), ((np.int32, np.int32), 150_000, 800, 0.1),
             ((np.int64, np.int16), 250_000, 200_000, 0.0)]))
    def test_group_by_wide_and_multiple_keys(ctx, dtypes, n, card, null_p):
        P.check_group_by_keys(ctx, rng_for("group_by_keys", len(dtypes), n, card), dtypes, n, card, null_p)

    @pytest.mark.parametrize("dtypes,n,m,idx_dtype", T.pick(
        emu=[((np.int64, np.int32, np.float64), 5000, 3000, np.uint32),
             ((np.int8, np.int16, np.int64, np.uint64, np.float32), 777, 2000, np.int64),
             ((np.int64,) * 17, 300, 500, np.uint16),        # more than one group of 16 columns
             ((np.int32, np.int64), 1000, 0, np.int32), ((np.int64, np.int64), 64, 64, np.uint8)],
        gpu=[((np.int64, np.int32, np.float64), 3_000_000, 1_000_003, np.uint32),
             ((np.int8, np.int16, np.int64, np.uint64, np.float32), 77_777, 2_000_000, np.int64),
             ((np.int64,) * 17, 30_000, 500_000, np.uint16),
             ((np.int32, np.int64), 1000, 0, np.int32), ((np.int64, np.int64), 64, 64, np.uint8)]))
    def test_take_record_batch_in_one_launch(ctx, dtypes, n, m, idx_dtype):
        P.check_take_record_batch(ctx, rng_for("take-rb", len(dtypes), n, m), dtypes, n, m, idx_dtype)

    def test_take_record_batch_without_nulls_has_no_bitmaps(ctx):
        rng = rng_for("take-rb-nonull")
        n, m = T.pick(emu=(4000, 4096), gpu=(400_000, 1 << 20))
        P.check_take_record_batch(ctx, rng, (np.int64, np.int32), n, m, np.uint32, value_null_p=0.0, index_null_p=0.0,
                                  offsets=False)

    @pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64,
                                       np.float32, np.float64])
    def test_compare_and_arithmetic_on_every_numeric_type(ctx, dtype):
        P.check_numeric_compare_arith(ctx, rng_for("numeric-ops", np.dtype(dtype).name), dtype, n=T.pick(emu=3000, gpu=300007))

    @pytest.mark.parametrize("wide", [0, 1])
    def test_sort_keys_with_a_shared_prefix(ctx, wide):
        lib = ctx._lib.get_lib()
        n, light = T.pick(emu=(9000 if wide else 5000, not wide), gpu=(2000003, False))
        P.check_sort_limited_range(ctx, lib, rng_for("sort-prefix", wide), n, wide, light=light)

    def test_compare_on_temporal_columns(ctx):
        P.check_temporal_compare(ctx, rng_for("temporal-compare"), n=T.pick(emu=3000, gpu=700003))

    def test_copy_segments_any_alignment(ctx):
        P.check_copy_segments(ctx, rng_for("copyseg"), T.pick(emu=1, gpu=40))

    @pytest.mark.parametrize("n,num_groups,null_p", T.pick(emu=[(4000, 37, 0.2), (2000, 5, 0.0), (300, 1, 1.0)],
                                                           gpu=[(2_000_000, 300_000, 0.2), (1_000_000, 5, 0.0), (300, 1, 1.0)]))
    def test_hash_minmax_and_count_dense_kernels(ctx, n, num_groups, null_p):
        P.check_hash_minmax_count_kernels(ctx, rng_for("hmmc", n, num_groups), n=n, num_groups=num_groups, null_p=null_p)

    @pytest.mark.parametrize("dtype,n,num_groups,null_p", T.pick(
        emu=[(np.float64, 4000, 37, 0.2), (np.float32, 2000, 5, 0.0), (np.float64, 300, 1, 1.0)],
        gpu=[(np.float64, 2_000_000, 300_000, 0.2), (np.float32, 1_000_000, 5, 0.0), (np.float64, 300, 1, 1.0)]))
    def test_hash_minmax_float_dense_kernels(ctx, dtype, n, num_groups, null_p):
        P.check_hash_minmax_float_kernels(ctx, rng_for("hmmf", n, num_groups), dtype=dtype, n=n, num_groups=num_groups, null_p=null_p)

    def test_float_sum_is_the_references_bit_for_bit_and_float_min_max(ctx):
        P.check_sum_float(ctx, rng_for("fsum"), T.pick(emu=[0, 1, 15, 16, 17, 63, 64, 65, 1000, 4097, 16385, 40001],
                                                       gpu=[0, 1, 17, 4097, 32768, 32769, 1_000_003, 16_777_216 + 12345]))

    def test_coalesce_of_two_operands_is_fill_null(ctx):
        P.check_coalesce2(ctx, rng_for("coalesce2"), n=T.pick(emu=3000, gpu=1_000_003))

    def test_take_of_rows_of_any_width_and_of_lists_with_fixed_width_values(ctx):
        """fixed_size_list / list / large_list selection where the nested values are fixed-width and free of nulls
        (FSLTakeExec -> FixedWidthTakeExec; ListSelectionImpl): arx_take_rows and arx_(large_)list_take_data."""
        n, m = T.pick(emu=(700, 600), gpu=(300_000, 250_000))
        P.check_take_rows(ctx, rng_for("takerows"), n=n, m=m)
        P.check_list_take(ctx, rng_for("listtake"), n=n, m=m)

    def test_grouped_float_sum_is_the_references_row_order_sum(ctx):
        """hash_sum / hash_mean of float32 / float64 values over dense group ids: the reference's row-order double accumulation
        per group, bit for bit (stable sort by group id + one walker per group)."""
        n, groups = T.pick(emu=(3000, (1, 7, 300)), gpu=(300_000, (1, 7, 300, 100_000)))
        P.check_hash_sum_float(ctx, rng_for("hashfsum"), n=n, groups=groups)

    def test_grouped_decimal128_sum(ctx):
        """hash_sum / hash_min / hash_max of decimal128 values over dense group ids: 128-bit sums modulo 2^128 kept with two atomics
        per row; extrema in signed 128-bit order by one owner per group over the rows sorted by group id."""
        n, groups = T.pick(emu=(3000, (1, 13, 400)), gpu=(60_000, (1, 13, 4000)))
        P.check_hash_sum_dec128(ctx, rng_for("hashdec"), n=n, groups=groups)
        P.check_hash_minmax_dec128(ctx, rng_for("hashdecmm"), n=n, groups=groups)
        P.check_reduce_dec128(ctx, rng_for("reducedec"), sizes=T.pick(emu=(0, 1, 63, 64, 65, 5000), gpu=(0, 1, 65, 70_001, 3_000_017)))

    def test_buffer_copy(ctx):
        P.check_buffer_copy(ctx, rng_for("bufcopy"), T.pick(emu=1, gpu=40))

    def test_bytes_to_bitmap(ctx):
        P.check_bytes_to_bitmap(ctx, rng_for("bytes-to-bitmap"), scale=T.pick(emu=1, gpu=30))

    def test_groupby_key_range(ctx):
        P.check_groupby_key_range(ctx, rng_for("key-range"), scale=T.pick(emu=1, gpu=50))

    def test_hash_any_all_dense_kernels(ctx):
        P.check_hash_any_all_kernels(ctx, rng_for("hash-bool"), **T.pick(emu={}, gpu={"n": 600_000, "num_groups": 5000}))

    def test_bitmap_copy_segments(ctx):
        P.check_bitmap_copy_segments(ctx, rng_for("bitseg"), T.pick(emu=1, gpu=20))

    def test_hash_product_group_edge_rows_and_dec128_split(ctx):
        """The C-ABI entry points behind hash_product / hash_first / hash_last / hash_one and the decimal128 sort keys against the
        oracle's restatements of GroupedProductImpl, GroupedFirstLastImpl and GroupedOneImpl."""
        n, groups = T.pick(emu=(3000, (1, 7, 300)), gpu=(200_000, (1, 7, 300, 50_000)))
        P.check_hash_product_and_edge_rows(ctx, rng_for("hashprod"), n=n, groups=groups)

    def test_group_moments_variance_stddev_skew_kurtosis(ctx):
        """hash_variance / hash_stddev / hash_skew / hash_kurtosis: the two-pass moments kernels against the oracle's restatement
        of GroupedStatisticImpl (kernels/hash_aggregate_numeric.cc:457-843); the device tier at the checker's own sizes."""
        P.check_group_moments(ctx, rng_for("moments"), **T.pick(emu={"n": 3000, "groups": (1, 7, 300)}, gpu={}))

    def test_rank(ctx):
        """Round 6 (f3): rank / rank_quantile = arx_sort_indices + arx_rank against the oracle's restatement of vector_rank.cc and the
        known answers of the reference's TestRank."""
        P.check_rank(ctx, rng_for, **T.pick(emu={"light": True}, gpu={"scale": 10}))

    def test_select_k_and_partition_nth(ctx):
        """Round 6 (f3): select_k_unstable / partition_nth_indices on the sort skeleton — the promised properties."""
        P.check_select_k_partition_nth(ctx, rng_for, **T.pick(emu={"light": True}, gpu={"scale": 10}))

    def test_sort_boolean_keys(ctx):
        """Round 6 (f3): boolean sort keys — the counting sort as three GetTakeIndices."""
        P.check_sort_boolean_keys(ctx, rng_for, scale=T.pick(emu=1, gpu=100))

    # ------------------------------------------------------------------ every compaction form the dispatch can choose
    @pytest.mark.parametrize("sel", ["drop", "emit_null"])
    @pytest.mark.parametrize("cell", FORM_CELLS, ids=_form_id)
    def test_filter_every_compaction_form(ctx, cell, sel):
        """arx_filter_count -> arx_filter_exec at the C ABI, one (width, kernel form, null selection) cell per test: the
        checker asserts with arx_filter_compact_form that the case runs the form it names before it launches, then
        compares every output byte and validity bit with numpy (P.filter_form_cases: lengths 1 .. 266 241, selectivities
        0 .. 1, four null densities, mask bit offsets 0 / 1 / 63, outputs 0 / 1 / 2048/W - 1 elements past a 2 KiB line)."""
        width, form = cell
        for kw in P.filter_form_cases(width, form, sel):
            P.check_filter_form(ctx, width, form, sel, **kw)

    def test_filter_32_byte_values_have_no_sweep_form(ctx):
        P.check_filter_w32_sweep_is_refused(ctx)

    @pytest.mark.parametrize("sel", ["drop", "emit_null"])
    @pytest.mark.parametrize("cell", ROW_NUMBER_CELLS, ids=_form_id)
    def test_mask_to_indices_every_form(ctx, cell, sel):
        """arx_mask_to_indices called directly, 2- and 4-byte row numbers under filter_sparse 1 (gather) and 0 (sweep, both
        batch forms).  Under the sweep, selectivity 0.3 keeps a tile's row numbers inside the LDS ring (each lane walks its
        own word), 1.0 does not (the 4096-row sweep)."""
        width, form = cell
        lengths = [1, 63, 4095, 4096, 4097, 3 * 4096 + 5] + ([65535] if width == 2 else [262144 + 4097])
        cases = [(n, 0.3) for n in lengths] + [(n, p) for n in lengths[-2:] for p in (0.0, 0.02, 1.0)]
        for i, (n, p) in enumerate(cases):
            P.check_mask_to_indices_form(ctx, width, form, sel, n, moff=(1, 63, 0)[i % 3], true_p=p,
                                         mnull=(0.3, 0.0, 0.05, 1.0)[i % 4] if n < 4096 or p != 0.3 else 0.3,
                                         disp=(1, P.kFlushBytes // width - 1, 0)[(i // 2) % 3])

    def test_mask_to_indices_8_byte_row_numbers(ctx):
        """index_width 8: the gather form with DROP, refused (nothing written) under filter_sparse = 0 and for EMIT_NULL."""
        for i, (n, p) in enumerate([(1, 0.3), (63, 0.3), (4097, 0.3), (3 * 4096 + 5, 1.0), (262144 + 4097, 0.3), (262144 + 4097, 0.02)]):
            P.check_mask_to_indices_form(ctx, 8, P.COMPACT_GATHER, "drop", n, moff=(1, 63, 0)[i % 3], true_p=p,
                                         mnull=(0.3, 0.0)[i % 2], disp=(1, P.kFlushBytes // 8 - 1, 0)[i % 3])
        P.check_mask_to_indices_width8_refusals(ctx)

    @pytest.mark.parametrize("invert", [0, 1])
    def test_bitmap_to_indices(ctx, invert):
        """Positions of the set / clear bits; lengths that are no multiple of 64: inverted bits past the end must not appear.
        Clear bits at 70 % (the sweep) and, on the multi-tile lengths, at 10 % (each lane walks its own word)."""
        for n in (1, 64, 65, 4097, 262144 + 4097):
            for off in (0, 1, 63):
                P.check_bitmap_to_indices(ctx, n, off, invert)
        for n in (4097, 262144 + 4097):
            P.check_bitmap_to_indices(ctx, n, 63, invert, true_p=0.9)
            P.check_bitmap_to_indices(ctx, n, 1, invert, true_p=0.0)
            P.check_bitmap_to_indices(ctx, n, 1, invert, true_p=1.0)

    @pytest.mark.parametrize("width", [1, 2, 4, 8, 16])
    def test_expand_by_mask(ctx, width):
        for i, n in enumerate((1, 64, 65, 4097, 262144 + 4097)):
            P.check_expand_by_mask(ctx, width, n, (1, 63, 0)[i % 3], 0.0)
            P.check_expand_by_mask(ctx, width, n, (63, 0, 1)[i % 3], 0.2)

    def test_every_compaction_form_cell_was_asserted(ctx):
        """Runs the 63-row case of every cell (so that this test stands alone), then reads the checker's own tally: every
        (kind, width, form, null selection) cell has cases whose arx_filter_compact_form assertion held.  Prints the tally:
        after a run of the whole file it holds the counts of the whole matrix."""
        for sel in ("drop", "emit_null"):
            for width, form in FORM_CELLS:
                P.check_filter_form(ctx, width, form, sel, 63, moff=1, mnull=0.3)
            for width, form in ROW_NUMBER_CELLS:
                P.check_mask_to_indices_form(ctx, width, form, sel, 63, moff=1, mnull=0.3)
        P.check_mask_to_indices_form(ctx, 8, P.COMPACT_GATHER, "drop", 63)
        for invert in (0, 1):
            P.check_bitmap_to_indices(ctx, 65, 1, invert)
        cells = [("values", w, P.COMPACT_FORM_NAMES[f], s) for w, f in FORM_CELLS for s in ("drop", "emit_null")]
        cells += [("row_numbers", w, P.COMPACT_FORM_NAMES[f], s) for w, f in ROW_NUMBER_CELLS for s in ("drop", "emit_null")]
        cells += [("row_numbers", 8, "gather", "drop"), ("bit_positions", 4, "gather", "drop")]
        for key in sorted(P.FORM_HITS):
            print("compaction form cases", *key, P.FORM_HITS[key])
        assert [c for c in cells if P.FORM_HITS.get(c, 0) == 0] == []
        assert any(k[0] == "bit_positions_inverted" and k[2].startswith("sweep") for k in P.FORM_HITS)
        assert not [k for k in P.FORM_HITS if k[1] == 32 and k[2] != "gather"]

    return {name: fn for name, fn in locals().items() if name.startswith("test_")}
