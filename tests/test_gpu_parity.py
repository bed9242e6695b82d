"""Parity tests proper: the HIP kernels on a real MI355X through arrow_amd.compute -> C ABI,
against the C oracle (bit-exact) and the reference's own build (pyarrow) on the same seeded
inputs.  Run with `pytest -m gpu` on the GPU box."""
import numpy as np
import pytest

from oracle import oracle as O

from . import parity_cases as P
from . import util as U

pytestmark = pytest.mark.gpu


def rng_for(*key):
    return np.random.default_rng([U.kRandomSeed, *[abs(hash(str(k))) % (1 << 31) for k in key]])


# ------------------------------------------------------------------ filter
@pytest.mark.parametrize("sel", ["drop", "emit_null"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 262144, 262145, 1_000_003])
def test_filter_int64_lengths(gpu_ctx, n, sel):
    rng = rng_for("f64len", n, sel)
    v = U.random_array(rng, np.int64, n, null_p=0.1)
    m = U.random_mask(rng, n, 0.3, null_p=0.05)
    P.check_filter(gpu_ctx, v, m, sel)


@pytest.mark.parametrize("sel", ["drop", "emit_null"])
@pytest.mark.parametrize("true_p", [0.0, 0.1, 0.5, 0.999, 1.0])
@pytest.mark.parametrize("vnull,mnull", [(0.0, 0.0), (0.01, 0.0), (0.1, 0.05), (0.999, 0.5), (1.0, 1.0)])
def test_filter_random_grid(gpu_ctx, true_p, vnull, mnull, sel):
    """FilterRandomTest's grid (vector_selection_test.cc:2241-2260) at 300k rows."""
    rng = rng_for("fprob", true_p, vnull, mnull, sel)
    n = 300_007
    v = U.random_array(rng, np.int64, n, null_p=vnull)
    m = U.random_mask(rng, n, true_p, null_p=mnull)
    P.check_filter(gpu_ctx, v, m, sel)


@pytest.mark.parametrize("sel", ["drop", "emit_null"])
@pytest.mark.parametrize("voff,moff", [(1, 0), (0, 3), (7, 13), (64, 65), (3, 4099), (100001, 77)])
def test_filter_offsets(gpu_ctx, voff, moff, sel):
    rng = rng_for("foff", voff, moff, sel)
    n = 500_000
    v = U.random_array(rng, np.int64, n, null_p=0.2, offset=voff, tail=5)
    m = U.random_mask(rng, n, 0.4, null_p=0.1, offset=moff, tail=9)
    P.check_filter(gpu_ctx, v, m, sel)


@pytest.mark.parametrize("dtype", [np.int8, np.uint16, np.int32, np.float32, np.float64, np.uint64])
@pytest.mark.parametrize("sel", ["drop", "emit_null"])
def test_filter_widths(gpu_ctx, dtype, sel):
    rng = rng_for("fw", dtype, sel)
    n = 400_003
    v = U.random_array(rng, dtype, n, null_p=0.1, offset=3)
    m = U.random_mask(rng, n, 0.5, null_p=0.05, offset=1)
    P.check_filter(gpu_ctx, v, m, sel)


def test_filter_tuning_variants_agree(gpu_ctx):
    lib = gpu_ctx._lib.get_lib()
    rng = rng_for("fvariants")
    v = U.random_array(rng, np.int64, 2_000_003, null_p=0.1, offset=2)
    m = U.random_mask(rng, 2_000_003, 0.1, null_p=0.05)
    with U.options(lib, {b"filter_batch": 1, b"filter_pipe": 0}):
        for batch in (1, 4):
            for pipe in (0, 1):
                assert lib.arx_set_option(b"filter_batch", batch) == 0
                assert lib.arx_set_option(b"filter_pipe", pipe) == 0
                for sel in ("drop", "emit_null"):
                    P.check_filter(gpu_ctx, v, m, sel, use_pyarrow=False)
        # int64 under the automatic choice runs the gather form, which reads neither knob: the forms the knobs do select
        # are the aligned sweeps, of a narrow type above 25 % and of int64 with the gather form switched off
        for dtype, offset, sparse in ((np.int32, 8, -1), (np.int64, 2, 0)):
            v = U.random_array(rng, dtype, 9000, null_p=0.1, offset=offset)
            m = U.random_mask(rng, 9000, 0.5, null_p=0.05)
            dv = v.to_device(gpu_ctx)
            with U.options(lib, {b"filter_sparse": sparse}):
                for batch in (1, 4):
                    for pipe in (0, 1):
                        assert lib.arx_set_option(b"filter_batch", batch) == 0
                        assert lib.arx_set_option(b"filter_pipe", pipe) == 0
                        for sel in ("drop", "emit_null"):
                            want = P.COMPACT_SWEEP_PIPELINED if (batch, pipe) == (4, 1) else P.COMPACT_SWEEP_PLAIN
                            assert P.compact_form_of_filter(gpu_ctx, dv, m, sel) == want, (dtype, batch, pipe, sel)
                            P.check_filter(gpu_ctx, v, m, sel, use_pyarrow=False)


def test_filter_10m_rows_config1(gpu_ctx):
    """BASELINE config 1 shape: 10M-row int64, 50 % selectivity."""
    rng = rng_for("cfg1")
    n = 10_000_000
    v = U.random_array(rng, np.int64, n)
    m = U.random_mask(rng, n, 0.5)
    out = P.check_filter(gpu_ctx, v, m, "drop")
    assert out.validity is None and out.null_count == 0


def test_filter_length_mismatch_is_invalid(gpu_ctx):
    v = U.HostArray(np.array([7, 8, 9], dtype=np.int64), None, 0, 3).to_device(gpu_ctx)
    m = U.HostArray(np.zeros(0, dtype=bool), None, 0, 0).to_device(gpu_ctx)
    for sel in ("drop", "emit_null"):
        with pytest.raises(gpu_ctx.ArrowInvalid):
            gpu_ctx.compute.filter(v, m, sel)


# ------------------------------------------------------------------ GetTakeIndices
@pytest.mark.parametrize("sel", ["drop", "emit_null"])
@pytest.mark.parametrize("n,off", [(0, 0), (1, 0), (100, 5), (65535, 0), (65536, 3), (3_000_001, 1)])
def test_mask_to_indices(gpu_ctx, n, off, sel):
    rng = rng_for("m2i", n, off, sel)
    m = U.random_mask(rng, n, 0.2, null_p=0.05, offset=off, tail=3)
    P.check_mask_to_indices(gpu_ctx, m, sel)


def test_record_batch_filter_is_take_of_indices(gpu_ctx):
    amd = gpu_ctx
    rng = rng_for("rb")
    n = 1_000_000
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
def test_take_index_types(gpu_ctx, idx_dtype):
    rng = rng_for("tk", idx_dtype)
    small = np.dtype(idx_dtype).itemsize == 1
    nv = 100 if small else (30_000 if np.dtype(idx_dtype).itemsize == 2 else 1_000_000)
    v = U.random_array(rng, np.int64, nv, null_p=0.1, offset=3)
    i = U.random_array(rng, idx_dtype, 300_001, null_p=0.1, offset=5, lo=0, hi=nv - 1)
    P.check_take(gpu_ctx, v, i)


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.float32, np.float64])
@pytest.mark.parametrize("vnull,inull", [(0.0, 0.0), (0.1, 0.0), (0.0, 0.3), (1.0, 0.0), (0.5, 1.0)])
def test_take_widths_and_nulls(gpu_ctx, dtype, vnull, inull):
    rng = rng_for("tkw", dtype, vnull, inull)
    v = U.random_array(rng, dtype, 300_000, null_p=vnull)
    i = U.random_array(rng, np.int32, 150_001, null_p=inull, lo=0, hi=299_999)
    P.check_take(gpu_ctx, v, i)


def test_take_monotonic_indices_from_filter(gpu_ctx):
    """The Filter+Take benchmark shape: indices = GetTakeIndices(mask) (monotonic uint32)."""
    amd = gpu_ctx
    rng = rng_for("tkmono")
    n = 5_000_000
    v = U.random_array(rng, np.int64, n, null_p=0.1)
    m = U.random_mask(rng, n, 0.1)
    idx = amd.compute.get_take_indices(m.to_device(amd))
    iv, _ = idx.to_numpy()
    P.check_take(gpu_ctx, v, U.HostArray(iv, None, 0, len(iv)), boundscheck=False)


def test_take_empty_and_no_boundscheck(gpu_ctx):
    rng = rng_for("tke")
    v = U.random_array(rng, np.int64, 50)
    P.check_take(gpu_ctx, v, U.HostArray(np.zeros(0, dtype=np.int32), None, 0, 0))
    i = U.random_array(rng, np.uint32, 70_000, lo=0, hi=49)
    P.check_take(gpu_ctx, v, i, boundscheck=False)


@pytest.mark.parametrize("bad", [9, -1])
def test_take_out_of_bounds(gpu_ctx, bad):
    v = U.HostArray(np.arange(5, dtype=np.int64), None, 0, 5)
    idx = np.array([0, bad, 0, 77], dtype=np.int64)
    P.check_take_out_of_bounds(gpu_ctx, v, U.HostArray(idx, None, 0, 4))


def test_take_out_of_bounds_first_offender_large(gpu_ctx):
    rng = rng_for("oob")
    idx = rng.integers(0, 1000, size=2_000_000).astype(np.int32)
    idx[1_234_567] = 1000
    idx[1_900_000] = -7
    v = U.HostArray(np.arange(1000, dtype=np.int64), None, 0, 1000)
    P.check_take_out_of_bounds(gpu_ctx, v, U.HostArray(idx, None, 0, len(idx)))


def test_take_null_index_is_not_bounds_checked(gpu_ctx):
    v = U.HostArray(np.arange(5, dtype=np.int64), None, 0, 5)
    idx = U.HostArray(np.array([1, 99, 2], dtype=np.int32), np.array([True, False, True]), 0, 3)
    out = P.check_take(gpu_ctx, v, idx)
    assert out.to_pylist() == [1, None, 2]


# ------------------------------------------------------------------ cast / compare / add
def _cast_inputs(rng, n):
    x = rng.standard_normal(n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e39, -1e39, 3.4028235677973366e38,
                        1e-40, -1e-46, 1.0000000596046448, 1.00000017881393433, 2.0 ** -126, 2.0 ** -150])
    x[: min(len(special), n)] = special[: min(len(special), n)]
    x[rng.integers(0, n, size=n // 20)] *= 1e40
    x[rng.integers(0, n, size=n // 20)] *= 1e-42
    return x


@pytest.mark.parametrize("n,off", [(0, 0), (1, 0), (13, 1), (2048, 0), (2049, 3), (4_000_001, 2)])
def test_cast_f64_f32(gpu_ctx, n, off):
    rng = rng_for("cast", n, off)
    x = _cast_inputs(rng, n + off + 2) if n else np.zeros(off + 2)
    valid = rng.random(len(x)) > 0.1 if n % 2 else None
    P.check_cast_f64_f32(gpu_ctx, U.HostArray(x, valid, off, n))


def test_cast_f64_f32_ties_to_even_exhaustive_mantissa_tail(gpu_ctx):
    """Every 29-bit tail pattern class around a float32 rounding boundary: RNE ties."""
    base = np.float64(1.0).view(np.uint64) if False else np.array([1.0]).view(np.uint64)[0]
    tails = np.arange(0, 1 << 20, dtype=np.uint64) << np.uint64(9)
    bits = (base + tails).astype(np.uint64)
    x = bits.view(np.float64)
    P.check_cast_f64_f32(gpu_ctx, U.HostArray(x.copy(), None, 0, len(x)))


@pytest.mark.parametrize("n,off", [(1, 0), (64, 0), (127, 1), (513, 0), (3_000_001, 5)])
def test_greater_f64_array_array(gpu_ctx, n, off):
    rng = rng_for("gt", n, off)
    a = U.random_array(rng, np.float64, n, null_p=0.1, offset=off)
    b = U.random_array(rng, np.float64, n, null_p=0.1 if n % 2 else 0.0, offset=2 * off)
    a.values[rng.integers(0, len(a.values), 5)] = np.nan
    k = min(len(a.values), len(b.values))
    b.values[:k:7] = a.values[:k:7]
    P.check_greater_f64(gpu_ctx, a, b)


def test_greater_scalar_forms_and_i64(gpu_ctx):
    rng = rng_for("gts")
    a = U.random_array(rng, np.float64, 1_000_000, null_p=0.1, offset=1)
    P.check_greater_f64(gpu_ctx, a, 0.25)
    P.check_greater_f64(gpu_ctx, -0.5, a)
    P.check_greater_f64(gpu_ctx, a, float("nan"))
    x = U.random_array(rng, np.int64, 777_777, lo=-5, hi=5)
    y = U.random_array(rng, np.int64, 777_777, lo=-5, hi=5)
    P.check_greater_f64(gpu_ctx, x, y)


def test_add(gpu_ctx):
    rng = rng_for("add")
    x = U.random_array(rng, np.int64, 3_000_001, null_p=0.1, offset=1)
    y = U.random_array(rng, np.int64, 3_000_001, offset=3)
    P.check_add(gpu_ctx, x, y)
    a = U.random_array(rng, np.float64, 1_000_000, null_p=0.1)
    b = U.random_array(rng, np.float64, 1_000_000, null_p=0.1)
    P.check_add(gpu_ctx, a, b)


# ------------------------------------------------------------------ sort
@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("placement", ["at_end", "at_start"])
def test_sort_small_range_with_ties_and_nulls(gpu_ctx, order, placement):
    rng = rng_for("sort1", order, placement)
    a = U.random_array(rng, np.uint64, 200_003, null_p=0.2, offset=3, lo=0, hi=7)
    P.check_sort_indices(gpu_ctx, a, order, placement)


@pytest.mark.parametrize("dtype", [np.uint64, np.int64])
@pytest.mark.parametrize("n", [1, 2, 255, 4096, 4097, 1_000_003])
def test_sort_full_range(gpu_ctx, dtype, n):
    rng = rng_for("sort2", dtype, n)
    a = U.random_array(rng, dtype, n)
    P.check_sort_indices(gpu_ctx, a, "ascending" if n % 2 else "descending", "at_end")


def test_sort_multi_chunk(gpu_ctx):
    """> 2048 tiles so that a chunk holds several tiles (cursor carry between tiles)."""
    rng = rng_for("sort3")
    n = 4096 * 2048 * 2 + 12345
    a = U.random_array(rng, np.uint64, n, null_p=0.01)
    P.check_sort_indices(gpu_ctx, a, "ascending", "at_end", use_pyarrow=False)


def test_sort_all_null_and_empty(gpu_ctx):
    a = U.HostArray(np.arange(10, dtype=np.uint64), np.zeros(10, dtype=bool), 0, 10)
    P.check_sort_indices(gpu_ctx, a)
    P.check_sort_indices(gpu_ctx, U.HostArray(np.zeros(0, dtype=np.uint64), None, 0, 0))


# ------------------------------------------------------------------ group-by
@pytest.mark.parametrize("skip_nulls,min_count", [(True, 1), (False, 1), (True, 0), (True, 3), (False, 0)])
def test_groupby_sum_options(gpu_ctx, skip_nulls, min_count):
    rng = rng_for("gb", skip_nulls, min_count)
    k = U.random_array(rng, np.int32, 300_000, null_p=0.05, offset=1, lo=-20, hi=20)
    v = U.random_array(rng, np.int64, 300_000, null_p=0.2, offset=2)
    P.check_groupby_sum(gpu_ctx, k, v, skip_nulls, min_count, batches=3)


def test_groupby_sum_wraparound_many_groups(gpu_ctx):
    rng = rng_for("gbwrap")
    n = 2_000_000
    k = U.random_array(rng, np.int32, n, lo=0, hi=200_000)
    v = U.random_array(rng, np.int64, n)
    P.check_groupby_sum(gpu_ctx, k, v, capacity=1 << 19)


def test_groupby_sum_golden_sum_only(gpu_ctx):
    keys = [1, 1, 2, 3, None, 1, 2, 2, None, 3]
    vals = [10, None, None, 1, 30, 5, None, 20, 40, None]
    k = U.HostArray(np.array([0 if x is None else x for x in keys], dtype=np.int32),
                    np.array([x is not None for x in keys]), 0, len(keys))
    v = U.HostArray(np.array([0 if x is None else x for x in vals], dtype=np.int64),
                    np.array([x is not None for x in vals]), 0, len(vals))
    got = P.check_groupby_sum(gpu_ctx, k, v)
    assert got == [(0, 1, 15), (0, 2, 20), (0, 3, 1), (1, 0, 70)]


def test_groupby_table_overflow_is_reported(gpu_ctx):
    amd = gpu_ctx
    k = amd.Array.from_numpy(np.arange(100, dtype=np.int32))
    v = amd.Array.from_numpy(np.ones(100, dtype=np.int64))
    op = amd.compute.GroupBySum(16, k.device)
    op.consume(k, v)
    with pytest.raises(amd.ArrowInvalid, match="full"):
        op.num_groups()


# ------------------------------------------------------------------ size-independent properties
def test_large_filter_properties(gpu_ctx):
    """2^28 rows (beyond the oracle's comfortable range): count == popcount, output is the
    subsequence (checked via a checksum of selected rows), take(indices) == filter."""
    import torch

    amd = gpu_ctx
    n = 1 << 28
    g = torch.Generator(device="cuda").manual_seed(1234)
    vals = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device="cuda", generator=g)
    sel = torch.rand(n, device="cuda", generator=g) < 0.1
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")
    bits = (sel.view(-1, 8).to(torch.uint8) * w).sum(dim=1, dtype=torch.uint8)
    values = amd.Array(amd.array.int64, n, [None, vals.view(torch.uint8)], 0, 0)
    mask = amd.Array(amd.array.bool_, n, [None, bits], 0, 0)
    out = amd.compute.filter(values, mask)
    s = int(sel.sum())
    assert out.length == s
    got = out.data[: s * 8].view(torch.int64)
    want = vals[sel]
    assert torch.equal(got, want)
    idx = amd.compute.get_take_indices(mask)
    assert idx.length == s and idx.type.name == "uint32"
    want_idx = torch.nonzero(sel).view(-1).to(torch.int64)
    assert torch.equal(idx.data[: s * 4].view(torch.int32).to(torch.int64) & 0xFFFFFFFF, want_idx)
    tk = amd.compute.take(values, idx, boundscheck=False)
    assert torch.equal(tk.data[: s * 8].view(torch.int64), want)


@pytest.mark.parametrize("skip_nulls,min_count", [(True, 1), (False, 1), (True, 0), (True, 40), (False, 0)])
def test_hash_sum_kernel_vtable(gpu_ctx, skip_nulls, min_count):
    """hash_sum(int64, uint32) through its HashAggregateKernel vtable: resize / consume (arrays,
    slices, broadcast + null scalars) / merge via group_id_mapping / finalize
    (hash_aggregate_numeric.cc:61-152; driven like groupby_aggregate_node.cc:210-337)."""
    P.check_hash_sum_kernel(gpu_ctx, rng_for("hsk", skip_nulls, min_count), n=400000, num_groups=5003,
                            skip_nulls=skip_nulls, min_count=min_count)


@pytest.mark.parametrize("num_groups,n", [(100, 2_000_000), (100_000, 4_000_000), (10_000_000, 8_000_000)])
def test_hash_sum_kernel_partitioned_by_group_id(gpu_ctx, num_groups, n):
    """The scratch form of the vtable consume (arx_hash_sum_i64_consume_ws) forced on: rows partitioned by the top bits
    of the dense group id, LDS aggregation, one flush per partition — no partition level (<= 2048 ids), one level,
    two levels; null values, hot groups, several consumes into the same state.  Same results as the per-row form."""
    lib = gpu_ctx._lib.get_lib()
    with U.options(lib, {b"groupby_partition_min_rows": 0}):
        P.check_hash_sum_kernel(gpu_ctx, rng_for("hskp", num_groups), n=n, num_groups=num_groups, null_p=0.1,
                                use_pyarrow=False)


def test_hash_sum_kernel_no_nulls_has_no_bitmap(gpu_ctx):
    P.check_hash_sum_kernel(gpu_ctx, rng_for("hsk0"), n=200000, num_groups=11, null_p=0.0)


@pytest.mark.parametrize("mode", [0, 1])
def test_filter_forced_sweep_and_sparse_forms(gpu_ctx, mode):
    """filter_sparse = 0 forces the sweeping compaction, 1 the gather form, for EVERY selectivity,
    null density, offset, width and length class: both must be bit-exact (auto picks by S/N)."""
    lib = gpu_ctx._lib.get_lib()
    with U.options(lib, {b"filter_sparse": mode}):
        for n in (1, 63, 64, 65, 4095, 4096, 4097, 1000003):
            for sel in ("drop", "emit_null"):
                rng = rng_for("fform", n, sel)
                v = U.random_array(rng, np.int64, n, null_p=0.1, offset=n % 5)
                m = U.random_mask(rng, n, 0.3, null_p=0.05, offset=n % 3)
                P.check_filter(gpu_ctx, v, m, sel, use_pyarrow=False)
        for true_p in (0.0, 0.02, 0.5, 1.0):
            for vnull, mnull in ((0.0, 0.0), (0.2, 0.0), (0.0, 0.3), (1.0, 1.0)):
                for sel in ("drop", "emit_null"):
                    rng = rng_for("fform2", true_p, vnull, mnull, sel)
                    v = U.random_array(rng, np.int64, 20000, null_p=vnull, offset=7)
                    m = U.random_mask(rng, 20000, true_p, null_p=mnull, offset=13)
                    P.check_filter(gpu_ctx, v, m, sel, use_pyarrow=False)
        for dtype in (np.int8, np.uint16, np.float32, np.float64):
            rng = rng_for("fform3", str(dtype))
            v = U.random_array(rng, dtype, 12345, null_p=0.1, offset=3)
            m = U.random_mask(rng, 12345, 0.15, null_p=0.05, offset=1)
            P.check_filter(gpu_ctx, v, m, "emit_null", use_pyarrow=False)


@pytest.mark.parametrize("bits", [0, 1, 5, 9, 11])
def test_groupby_partitioned_path(gpu_ctx, bits):
    """The radix-partitioned consume (hist -> scatter level 1 [-> level 2] -> LDS aggregate -> flush)
    forced on, for one-level (bits <= 8) and two-level plans, with null keys / null values /
    wrap-around, several consume calls, and keys that overflow one partition's LDS table."""
    lib = gpu_ctx._lib.get_lib()
    with U.options(lib, {b"groupby_partition_min_rows": 0, b"groupby_partition_bits": bits}):
        rng = rng_for("gbp", bits)
        n = 3000003
        k = U.random_array(rng, np.int32, n, null_p=0.02, offset=3, lo=-2**31, hi=2**31 - 1)
        k.values[: n // 2] = k.values[: n // 2] % 1777          # many repeats + distinct tail
        v = U.random_array(rng, np.int64, n, null_p=0.1, offset=1)
        P.check_groupby_sum(gpu_ctx, k, v, skip_nulls=(bits % 2 == 1), min_count=1, batches=2,
                            use_pyarrow=(bits == 9))
        # no nulls at all (the HAS_NULLS = false kernels)
        k2 = U.random_array(rng, np.int32, n, lo=0, hi=50000)
        v2 = U.random_array(rng, np.int64, n)
        P.check_groupby_sum(gpu_ctx, k2, v2, use_pyarrow=False)


@pytest.mark.parametrize("order,placement", [("ascending", "at_end"), ("descending", "at_start")])
def test_sharded_sort_single_rank_pieces(gpu_ctx, order, placement):
    """The device pieces of the multi-GPU sort (splitter histogram, stable partition by
    destination, null-row positions) on one rank: the result must equal the plain sort."""
    from arrow_amd import parallel

    rng = rng_for("shsort", order, placement)
    n = 1_500_001
    a = U.random_array(rng, np.uint64, n, null_p=0.03, offset=5)
    a.values[a.offset:a.offset + n:4] %= 1000
    rows, start = parallel.sharded_sort_indices(a.to_device(gpu_ctx), order, placement)
    want = O.sort_indices_64(np.ascontiguousarray(a.values), a.valid_bitmap(), a.offset, n,
                             descending=(order == "descending"), nulls_at_start=(placement == "at_start"))
    assert start == 0
    assert (rows.cpu().numpy().astype(np.uint64) == want).all()


@pytest.mark.parametrize("l1_global,agg_chunk,bits", [(0, 1 << 16, 9), (1, 1 << 12, 9), (0, 1 << 20, 5), (1, 1 << 18, 11)])
def test_groupby_partition_knobs(gpu_ctx, l1_global, agg_chunk, bits):
    """Tuning knobs of the partitioned consume never change results: level 1 with chunked exact offsets vs global
    cursors, the rows per LDS-aggregate work unit (how often a partition's groups are flushed)."""
    lib = gpu_ctx._lib.get_lib()
    opts = {b"groupby_partition_min_rows": 0, b"groupby_partition_bits": bits, b"groupby_l1_global": l1_global,
            b"groupby_agg_chunk_rows": agg_chunk}
    with U.options(lib, opts):
        rng = rng_for("gbpknobs", l1_global, agg_chunk, bits)
        n = 3000000
        k = U.random_array(rng, np.int32, n, null_p=0.02, offset=3, lo=-2**31, hi=2**31 - 1)
        k.values[: n // 2] = k.values[: n // 2] % 1777
        v = U.random_array(rng, np.int64, n, null_p=0.1, offset=1)
        P.check_groupby_sum(gpu_ctx, k, v, skip_nulls=True, min_count=1, batches=2, use_pyarrow=False)
        k2 = U.random_array(rng, np.int32, n, lo=0, hi=50000)
        v2 = U.random_array(rng, np.int64, n)
        P.check_groupby_sum(gpu_ctx, k2, v2, use_pyarrow=False)


@pytest.mark.parametrize("bits", [1, 4, 8, 11])
def test_groupby_wide_one_level_form(gpu_ctx, bits):
    """The wide one-level plan forced on (groupby_wide = 2): ONE flat scatter of register-held 24576-row tiles into
    2^bits bins of 12-byte records + 8192-slot LDS tables; null keys / null values / wrap-around, several consume
    calls, partial last tiles, more groups than the LDS tables hold (rows spill to the HBM table, still exact)."""
    lib = gpu_ctx._lib.get_lib()
    opts = {b"groupby_partition_min_rows": 0, b"groupby_wide": 2, b"groupby_partition_bits": bits,
            b"groupby_wide_agg_chunk_rows": 1 << (14 + bits % 3)}
    wide0 = lib.arx_get_counter(b"groupby_slices_wide")
    with U.options(lib, opts):
        rng = rng_for("gbwide", bits)
        n = 3000000
        k = U.random_array(rng, np.int32, n, null_p=0.02, offset=3, lo=-2**31, hi=2**31 - 1)
        k.values[: n // 2] = k.values[: n // 2] % 1777          # many repeats + distinct tail
        v = U.random_array(rng, np.int64, n, null_p=0.1, offset=1)
        P.check_groupby_sum(gpu_ctx, k, v, skip_nulls=(bits % 2 == 1), min_count=1, batches=2, use_pyarrow=(bits == 4))
        k2 = U.random_array(rng, np.int32, n + 4097, lo=0, hi=9000000)      # no nulls: the HAS_NULLS = false kernels
        v2 = U.random_array(rng, np.int64, n + 4097)
        P.check_groupby_sum(gpu_ctx, k2, v2, use_pyarrow=False)
        assert lib.arx_get_counter(b"groupby_slices_wide") >= wide0 + 3, "the wide plan did not run"


@pytest.mark.parametrize("stripe", [0, 276])
@pytest.mark.parametrize("hot", [False, True])
def test_groupby_wide_form_without_histogram(gpu_ctx, hot, stripe):
    """The wide plan with fixed rooms instead of a histogram pass: evenly spread keys fit their rooms (no overflow);
    a few hot keys outgrow one room — the slice is redone with counted partitions (null rows are not consumed twice)
    and the call's later slices stay on the counted plan.  Results exact either way — and whether the rooms lie one after
    the other or in stripes of `stripe` records (groupby_stripe)."""
    lib = gpu_ctx._lib.get_lib()
    opts = {b"groupby_partition_min_rows": 0, b"groupby_wide": 2, b"groupby_partition_bits": 11, b"groupby_wide_room_min_mean": 16, b"groupby_stripe": stripe,
            b"groupby_wide_max_slice_rows": 2457600}
    names = (b"groupby_slices_rooms", b"groupby_rooms_overflows")
    before = [lib.arx_get_counter(c) for c in names]
    with U.options(lib, opts):
        rng = rng_for("gbrooms", hot)
        n = 3200000
        k = U.random_array(rng, np.int32, n, null_p=0.02, lo=-2**31, hi=2**31 - 1)
        if hot:
            k.values[n // 3:] = 7            # two thirds of the rows in ONE group: its partition outgrows its room
        v = U.random_array(rng, np.int64, n, null_p=0.1)
        P.check_groupby_sum(gpu_ctx, k, v, skip_nulls=False, min_count=2, batches=1, use_pyarrow=not hot)
    rooms, overflows = (lib.arx_get_counter(c) - b for c, b in zip(names, before))
    assert rooms >= 1, "the plan without a histogram did not run"
    assert (overflows >= 1) == hot, (rooms, overflows)
    if hot:
        assert rooms == 1, "after an overflow the call stays on the counted plan"


@pytest.mark.parametrize("distinct", [50000, 0])
def test_groupby_probe_slice_selects_the_plan(gpu_ctx, distinct):
    """A capacity that only bounds the group count from above (two-level plan) + enough rows: a HyperLogLog sketch of
    the first groupby_probe_rows keys estimates the distinct keys; few of them, seen often -> the rows run the wide plan, keys
    that do not repeat -> the two-level plan.  Same groups either way."""
    lib = gpu_ctx._lib.get_lib()
    names = (b"groupby_slices_probe", b"groupby_slices_wide", b"groupby_slices_two_level")
    before = [lib.arx_get_counter(c) for c in names]
    with U.options(lib, {
            b"groupby_partition_min_rows": 0,
            b"groupby_probe_rows": 262144,
            b"groupby_wide_max_bits": 6,    # (so that the capacity bound alone cannot pick the wide plan)
    }):
        rng = rng_for("gbprobe", distinct)
        n = 9 * 262144 + 1234
        hi = distinct if distinct else 2**31 - 1
        k = U.random_array(rng, np.int32, n, null_p=0.01, lo=-5 if distinct else -2**31, hi=hi)
        v = U.random_array(rng, np.int64, n, null_p=0.05)
        cap = 1 << 21 if distinct else 1 << 23     # (2.4M distinct keys need the larger table)
        P.check_groupby_sum(gpu_ctx, k, v, capacity=cap, batches=1, use_pyarrow=False)
        P.check_groupby_sum(gpu_ctx, k, v, capacity=cap, batches=2, use_pyarrow=False)   # second consume: table not empty
    probe, wide, two = (lib.arx_get_counter(c) - b for c, b in zip(names, before))
    assert probe == 3, "one sketch (round 3: one probe slice) per consume call"
    if distinct:
        assert (wide, two) == (3, 0), (probe, wide, two)     # round 4: the sketch aggregates nothing, every row runs the wide plan
    else:
        assert (wide, two) == (0, 3), (probe, wide, two)


@pytest.mark.parametrize("wide,bits,parts,keys_hi", [(1, -1, 8, 300_000), (2, 8, 5, 300_000), (1, 0, 2, 1500), (1, 9, 64, 2_000_000)])
def test_groupby_consume_partials(gpu_ctx, wide, bits, parts, keys_hi):
    """The sharded group-by's local pass without the local table (arx_groupby_sum_i64_consume_partials) on the device: the
    planner's own choice for 3 M rows, the wide form forced, the unpartitioned aggregate, a two-level plan with more groups
    than its LDS tables hold; owners, sums, counts, the receivers' merges and the too-small-region status are checked by
    check_groupby_consume_partials."""
    lib = gpu_ctx._lib.get_lib()
    # (room_min_mean 1 << 14 where the wide form is not forced: a value this case runs with, not a restore)
    opts = {b"groupby_wide": wide, b"groupby_partition_bits": bits, b"groupby_wide_room_min_mean": 16 if wide == 2 else 1 << 14}
    with U.options(lib, opts):
        rng = rng_for("gbemit", wide, bits, parts)
        n = 3_000_000
        k = U.random_array(rng, np.int32, n, lo=0, hi=keys_hi, offset=3)
        v = U.random_array(rng, np.int64, n, offset=1)
        records = P.check_groupby_consume_partials(gpu_ctx, k, v, parts, capacity=1 << 23)
        assert records >= keys_hi * (1 - np.exp(-n / keys_hi)) * 0.99      # (at least the distinct keys)


def test_groupby_virtual_ranks_on_one_gpu(gpu_ctx):
    """The multi-GPU hash_sum data path with P = 4 virtual ranks on one device: per-rank local
    aggregate -> partials exported as records grouped by hash(key) % P -> exchange (slicing stands in
    for the all-to-all) -> merge -> finalize; the union must be the oracle's result and every key
    must be owned by exactly one rank."""
    import torch

    from arrow_amd import parallel

    amd = gpu_ctx
    P_, n = 4, 600_000
    rng = rng_for("vranks")
    shards = []
    for r in range(P_):
        k = U.random_array(rng, np.int32, n + 1000 * r, null_p=0.01, offset=r, lo=-40000, hi=40000)
        v = U.random_array(rng, np.int64, n + 1000 * r, null_p=0.1, offset=1)
        shards.append((k, v))
    parts, counts = [], []
    for k, v in shards:
        local = amd.compute.GroupBySum(1 << 18, k.to_device(amd).device)
        local.consume(k.to_device(amd), v.to_device(amd))
        records, cnt = parallel.export_partitioned(local, P_)      # 24-byte records, destination-major
        parts.append(records)
        counts.append([int(x) for x in cnt.cpu().tolist()])
        assert records.numel() == parallel.RECORD_BYTES * sum(counts[-1]) == parallel.RECORD_BYTES * local.num_groups()
    got = {}
    for dst in range(P_):
        owned = amd.compute.GroupBySum(1 << 18, parts[0].device)
        for src in range(P_):
            lo = sum(counts[src][:dst]) * parallel.RECORD_BYTES
            hi = lo + counts[src][dst] * parallel.RECORD_BYTES
            parallel.merge_records(owned, parts[src][lo:hi])
        gk, gkv, gs, gvalid = owned.finalize()
        for key, kv, s, ok in zip(gk.cpu().tolist(), gkv.cpu().tolist(), gs.cpu().tolist(), gvalid.cpu().tolist()):
            ident = (bool(kv), key if kv else 0)
            assert ident not in got, f"key {ident} owned by two virtual ranks"
            got[ident] = s if ok else None
    keys = np.concatenate([k.values[k.offset:k.offset + k.length] for k, _ in shards])
    kval = np.concatenate([np.ones(k.length, bool) if k.valid is None else k.valid[k.offset:k.offset + k.length] for k, _ in shards])
    vals = np.concatenate([v.values[v.offset:v.offset + v.length] for _, v in shards])
    vval = np.concatenate([np.ones(v.length, bool) if v.valid is None else v.valid[v.offset:v.offset + v.length] for _, v in shards])
    w = O.groupby_sum_i64(keys, O.pack_bits(kval), 0, vals, O.pack_bits(vval), 0, len(keys))
    want = {(bool(kv), int(k) if kv else 0): (int(s) if ok else None)
            for k, kv, s, ok in zip(w["keys"], w["key_is_valid"], w["sums"], w["valid"])}
    assert got == want


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("global_bits", [14, 4, -14])
def test_sort_msd_hybrid_path(gpu_ctx, global_bits, fused):
    """The MSD-hybrid sort forced on (two global levels [+ the in-bucket level when the global
    bits are capped] + the windowed final ranking): full-range keys, heavy ties (bucket overflow ->
    LSD fallback), nulls (prep + MSD), descending, signed."""
    lib = gpu_ctx._lib.get_lib()
    opts = {b"sort_msd": 1, b"sort_msd_fused": fused}   # fused 1: LDS-resident bucket finish; 0: local + windowed final
    if global_bits < 0:   # the segmented form: an extra level on the top bits, then one pipeline per segment
        global_bits = -global_bits
        opts[b"sort_msd_segment_rows"] = 4096
        # beyond the segment size the wide two-level form (run_msd_sort_wide) runs first; fused = 0 switches it off so
        # that the segmented form itself stays covered
        opts[b"sort_msd_wide"] = fused
    opts[b"sort_msd_global_bits"] = global_bits
    with U.options(lib, opts):
        n = 6000011
        rng = rng_for("msd", global_bits, fused)
        for dtype, order, placement, null_p in ((np.uint64, "ascending", "at_end", 0.0),
                                               (np.int64, "descending", "at_start", 0.03),
                                               (np.uint64, "descending", "at_end", 0.0)):
            a = U.random_array(rng, dtype, n, null_p=null_p, offset=3)
            a.values[a.offset:a.offset + n - 1:5] = a.values[a.offset + 1:a.offset + n:5]  # ties
            P.check_sort_indices(gpu_ctx, a, order, placement, use_pyarrow=(dtype == np.int64))
        ties = U.random_array(rng, np.uint64, n, lo=0, hi=7)       # 7 distinct keys: buckets overflow
        P.check_sort_indices(gpu_ctx, ties, "ascending", "at_end", use_pyarrow=False)
        small = U.random_array(rng, np.uint64, 300)
        P.check_sort_indices(gpu_ctx, small, "ascending", "at_end", use_pyarrow=False)


@pytest.mark.parametrize("shift,gap2,b2max", [(4, 1, 12), (2, 1, 12), (4, 0, 12), (0, 1, 12), (0, 0, 12), (4, 1, 0),
                                              (0, 0, 0)])
def test_sort_wide_sampled_level1(gpu_ctx, shift, gap2, b2max):
    lib = gpu_ctx._lib.get_lib()
    failed = P.check_sort_wide_sampled(gpu_ctx, lib, rng_for("wide-sampled", shift, gap2), 6_000_011, shift, gap2,
                                       b2max)
    if shift == 0 and gap2 == 0:
        assert failed == 0   # exact counts never overflow


@pytest.mark.parametrize("rpt", [(8, 8), (8, 24), (16, 16), (24, 24)])
def test_sort_wide_register_staged_tiles(gpu_ctx, rpt):
    """Level-1 / level-2 scatter tiles of 8 (LDS-resident), 16 and 24 (register-staged) rows per thread."""
    lib = gpu_ctx._lib.get_lib()
    with U.options(lib, {
            b"sort_msd_tiny_bucket": {16: 0, 8: 1}.get(rpt[0], 2),   # (256- / 512-thread bucket finish)
            b"sort_msd_bucket_cpt": 8 if rpt[1] == 16 else 4,   # sub-bucket counters per thread of the finish
    }):
        P.check_sort_wide_sampled(gpu_ctx, lib, rng_for("wide-rpt", *rpt), 3_000_011, 4, 1, 12, rpt=rpt, typed_keys=True)
        P.check_sort_wide_many_bins(gpu_ctx, lib, rng_for("wide-rpt-bins", *rpt), 2_000_003, 16, 12, combos=((0, 0), (2, 1)), rpt=rpt)


@pytest.mark.parametrize("n,bits,gap2,shift,rpt,b2max,wc,prefetch,l2w", [(3_000_011, 0, 1, 4, (24, 16), 11, 256, 1, 1), (3_000_003, 14, 0, 2, (8, 8), 11, 0, 1, 2),
                                                                         (2_000_003, 8, 1, 0, (16, 24), 11, 7, 0, 0), (4_000_003, 0, 1, 4, (24, 16), 4, 48, 1, 1),
                                                                         (3_000_003, 18, 1, 4, (24, 16), 9, 24, 1, 3), (3_000_003, 18, 1, 4, (24, 16), 9, 24, 0, 1),
                                                                         (3_000_003, 14, 0, 0, (8, 16), 5, 32, 1, 2), (3_000_003, 20, 1, 4, (24, 16), 11, 32, 1, 1)])
def test_sort_wide_rec8_words(gpu_ctx, n, bits, gap2, shift, rpt, b2max, wc, prefetch, l2w):
    """8-byte {key bits, row id} words through the wide form (the form the 2e9-row bench runs): ties below the word,
    duplicates, the tie budget, fall-backs; level 1 tile at a time and write-combined (2 to 512 bins — 9 + 9 bits is the
    2e9-row split's level 1); counters prove which form ran."""
    P.check_sort_wide_rec8(gpu_ctx, gpu_ctx._lib.get_lib(), rng_for("wide-rec8", n, bits), n, bits=bits, gap2=gap2, shift=shift, rpt=rpt,
                           b2max=b2max, wc=wc, prefetch=prefetch, l2w=l2w)


@pytest.mark.parametrize("bits,b2max", [(13, 12), (16, 12), (20, 12), (19, 11), (19, 0)])
def test_sort_wide_many_level2_bins(gpu_ctx, bits, b2max):
    P.check_sort_wide_many_bins(gpu_ctx, gpu_ctx._lib.get_lib(), rng_for("wide-bins", bits, b2max), 2_500_003, bits,
                                b2max)


def test_null_count_bookkeeping(gpu_ctx):
    P.check_null_count_bookkeeping(gpu_ctx, rng_for("nullcount"))


@pytest.mark.parametrize("msd", [0, 1])
@pytest.mark.parametrize("dtype", [np.uint32, np.int32, np.float64, np.float32])
def test_sort_32bit_and_float_keys(gpu_ctx, dtype, msd):
    """array_sort_indices on the other fixed-width key types: 32-bit integers (4 LSD passes), floats
    with NaNs as null-likes next to the nulls whatever the order, -0.0 tying with 0.0, infinities."""
    lib = gpu_ctx._lib.get_lib()
    with U.options(lib, {b"sort_msd": 1 if msd else 0}):
        rng = rng_for("sort32f", str(dtype), msd)
        n = 5000003
        for order, placement, null_p in (("ascending", "at_end", 0.05), ("descending", "at_start", 0.05),
                                         ("descending", "at_end", 0.0)):
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
            P.check_sort_indices(gpu_ctx, a, order, placement)


def test_sort_virtual_ranks_on_one_gpu(gpu_ctx):
    """The multi-GPU sort_indices data path with P = 4 virtual ranks on one device: splitter
    histogram (summed over the shards), stable partition by destination on every shard, the
    exchange emulated by slicing (receive buffers concatenated in source-rank order), local stable
    sort + gather.  The concatenation over ranks must be the oracle's argsort of the whole array."""
    import ctypes as C

    import torch

    amd = gpu_ctx
    lib = amd._lib.get_lib()
    from arrow_amd.array import alloc, current_stream

    P_, bits = 4, 12
    rng = rng_for("vsort")
    shards = [U.random_array(rng, np.uint64, 300_000 + 7_001 * r, null_p=0.02, offset=r + 1) for r in range(P_)]
    for a in shards:
        a.values[a.offset:a.offset + a.length:3] %= 50          # ties across shards
    dev = [a.to_device(amd) for a in shards]
    stream = current_stream(dev[0].device)
    offsets = np.cumsum([0] + [a.length for a in shards])
    hist = torch.zeros(1 << bits, dtype=torch.int64, device=dev[0].device)
    for d in dev:
        sp = d.span()
        amd._lib.check(lib.arx_sort_key_histogram(C.byref(sp), 0, 0, bits, hist.data_ptr(), stream))
    cum = torch.cumsum(hist, 0).cpu().numpy()
    total = int(cum[-1])
    split = [int(np.searchsorted(cum, (total * p + P_ - 1) // P_) + 1) for p in range(1, P_)]
    split_arr = (C.c_uint32 * len(split))(*split)
    sent = []   # per source: (keys, global rows, counts)
    for r, d in enumerate(dev):
        n = d.length
        ws = alloc(lib.arx_sort_indices_workspace_bytes(n) + 256, d.device)
        ws_ptr = (ws.data_ptr() + 255) & ~255
        keys = torch.empty(n, dtype=torch.int64, device=d.device)
        rows = torch.empty(n, dtype=torch.int32, device=d.device)
        counts = torch.zeros(P_, dtype=torch.int64, device=d.device)
        nv = C.c_int64(0)
        sp = d.span()
        amd._lib.check(lib.arx_sort_partition_by_bins(C.byref(sp), 0, 0, bits, split_arr, P_, ws_ptr,
                                                      ws.numel() - (ws_ptr - ws.data_ptr()), keys.data_ptr(),
                                                      rows.data_ptr(), counts.data_ptr(), C.byref(nv), stream))
        torch.cuda.synchronize()
        sent.append((keys[: nv.value], rows[: nv.value].to(torch.int64) + int(offsets[r]), counts.cpu().tolist()))
    out = []
    for dst in range(P_):
        ks, gs = [], []
        for keys, grows, counts in sent:       # source-rank order
            lo = sum(counts[:dst])
            ks.append(keys[lo: lo + counts[dst]])
            gs.append(grows[lo: lo + counts[dst]])
        k, g = torch.cat(ks).contiguous(), torch.cat(gs).contiguous()
        karr = amd.Array(amd.array.uint64, k.numel(), [None, k.view(torch.uint8)], 0, 0)
        perm = amd.compute.sort_indices(karr).data[: k.numel() * 8].view(torch.int64)
        out.append(g[perm])
        assert k.numel() > total // (2 * P_), "splitters should balance the virtual ranks"
    got = torch.cat(out).cpu().numpy().astype(np.uint64)
    vals = np.concatenate([a.values[a.offset:a.offset + a.length] for a in shards])
    valid = np.concatenate([np.ones(a.length, bool) if a.valid is None else a.valid[a.offset:a.offset + a.length] for a in shards])
    want = O.sort_indices_64(np.ascontiguousarray(vals), O.pack_bits(valid), 0, len(vals))
    n_valid = int(valid.sum())
    assert (got == want[:n_valid]).all()        # nulls travel separately (row numbers only)


@pytest.mark.parametrize("small_bucket,final_rows_log2,seg_rows,v2", [(0, 4, 1 << 27, 1), (1, 1, 1 << 27, 1), (1, 3, 1 << 20, 0),
                                                                     (0, 1, 1 << 27, 0), (1, 2, 1 << 19, 1)])
def test_sort_msd_bucket_variants_on_gpu(gpu_ctx, small_bucket, final_rows_log2, seg_rows, v2):
    """Tuning knobs of the MSD sort never change results on the device either: both LDS bucket finishes
    (msd_bucket_kernel / msd_bucket2_kernel: one LDS-atomic pass, up to 4096 sub-buckets), 1024- vs 512-thread
    form, sub-bucket size, segmented form."""
    lib = gpu_ctx._lib.get_lib()
    opts = {b"sort_msd": 1, b"sort_msd_small_bucket": small_bucket, b"sort_msd_final_rows_log2": final_rows_log2,
            b"sort_msd_segment_rows": seg_rows, b"sort_msd_bucket_v2": v2, b"sort_msd_wide": v2}
    with U.options(lib, opts):
        rng = rng_for("msdknobs-gpu", small_bucket, final_rows_log2, seg_rows, v2)
        n = 5_000_011
        a = U.random_array(rng, np.uint64, n, null_p=0.02, offset=1)
        a.values[a.offset:a.offset + n - 1:7] = a.values[a.offset + 1:a.offset + n:7]  # ties
        P.check_sort_indices(gpu_ctx, a, "descending", "at_start", use_pyarrow=False)
        b = U.random_array(rng, np.int64, n, offset=0)
        P.check_sort_indices(gpu_ctx, b, "ascending", "at_end", use_pyarrow=False)


@pytest.mark.parametrize("placement,window", [("at_end", None), ("at_start", None),
                                              ("at_end", (1_700_000_000_000_000, 86_400_000_000)),
                                              ("at_start", (-40_000, 100_000))])
def test_sort_records_virtual_ranks_on_one_gpu(gpu_ctx, placement, window):
    """The ONE-buffer exchange of the sharded sort with P = 3 virtual ranks: arx_sort_partition_records packs
    {transformed key, local row} records destination-major with the shard's null rows in the last / first rank's
    block; slicing stands in for the all-to-all(v); arx_sort_unpack_records rebuilds keys + global rows in source
    order; local stable sort + gather.  Concatenated over ranks = the oracle's argsort, nulls included.
    window: every key inside [lo, lo + span) (timestamps, ids) — the splitter bins come from arx_sort_key_range's
    window and every virtual rank must still get its share."""
    import ctypes as C

    import torch

    amd = gpu_ctx
    lib = amd._lib.get_lib()
    from arrow_amd import parallel
    from arrow_amd.array import alloc, current_stream

    P_, bits = 3, 12
    nulls_first = placement == "at_start"
    target = 0 if nulls_first else P_ - 1
    rng = rng_for("vsortrec", placement)
    shards = [U.random_array(rng, np.int64, 200_000 + 5_003 * r, null_p=0.03 if r != 1 else 0.0, offset=r + 2) for r in range(P_)]
    for a in shards:
        a.values[a.offset:a.offset + a.length:3] %= 50
        if window is not None:   # ties across the shards that do not pile up in one bin
            v = a.values[a.offset:a.offset + a.length]
            v[:] = (v.astype(np.uint64) % np.uint64(window[1])).astype(np.int64) + np.int64(window[0])
            v[::3] = shards[0].values[shards[0].offset:shards[0].offset + len(v[::3])]
    dev = [a.to_device(amd) for a in shards]
    device = dev[0].device
    stream = current_stream(device)
    offsets = [int(x) for x in np.cumsum([0] + [a.length for a in shards])]
    hist = torch.zeros(1 << bits, dtype=torch.int64, device=device)
    win = None
    if window is not None:
        rng_t = torch.zeros(2, dtype=torch.int64, device=device)   # atomicMax across the shards = the MAX all-reduce
        for d in dev:
            sp = d.span()
            amd._lib.check(lib.arx_sort_key_range(C.byref(sp), 1, 1, rng_t.data_ptr(), stream))
        inv_min, kmax = [int(x) & (2**64 - 1) for x in rng_t.cpu().tolist()]
        kmin = ~inv_min & (2**64 - 1)
        tk = np.concatenate([(~(a.values[a.offset:a.offset + a.length].view(np.uint64) ^ np.uint64(1 << 63)))
                             [np.ones(a.length, bool) if a.valid is None else a.valid[a.offset:a.offset + a.length]]
                             for a in shards])              # descending int64: transformed key = ~(key ^ sign)
        assert (kmin, kmax) == (int(tk.min()), int(tk.max()))
        win = amd._lib.ArxSortKeyWindow(kmin, 64 - (kmax - kmin).bit_length(), 0)
    for d in dev:
        sp = d.span()
        amd._lib.check(lib.arx_sort_key_histogram_window(C.byref(sp), 1, 1, bits, C.byref(win) if win else None,
                                                         hist.data_ptr(), stream))
    cum = torch.cumsum(hist, 0).cpu().numpy()
    total = int(cum[-1])
    split = [int(np.searchsorted(cum, (total * p + P_ - 1) // P_) + 1) for p in range(1, P_)]
    split_arr = (C.c_uint32 * len(split))(*split)
    sent = []
    for r, d in enumerate(dev):
        n = d.length
        ws = alloc(lib.arx_sort_indices_workspace_bytes(n) + 256, device)
        ws_ptr = (ws.data_ptr() + 255) & ~255
        rec = torch.empty(n * parallel.SORT_RECORD_BYTES, dtype=torch.uint8, device=device)
        counts = torch.zeros(P_, dtype=torch.int64, device=device)
        nv = C.c_int64(0)
        sp = d.span()
        amd._lib.check(lib.arx_sort_partition_records_window(
            C.byref(sp), 1, 1, 0 if nulls_first else 1, bits, C.byref(win) if win else None, split_arr, P_, ws_ptr,
            ws.numel() - (ws_ptr - ws.data_ptr()), rec.data_ptr(), counts.data_ptr(), C.byref(nv), stream))
        torch.cuda.synchronize()
        sent.append((rec, counts.cpu().tolist(), nv.value, n - nv.value))
    out = []
    for dst in range(P_):
        blocks, meta = [], []
        for src, (rec, counts, nv, nnull) in enumerate(sent):
            send = [counts[p] + (nnull if p == target else 0) for p in range(P_)]
            lo = sum(send[:dst]) * parallel.SORT_RECORD_BYTES
            blocks.append(rec[lo: lo + send[dst] * parallel.SORT_RECORD_BYTES])
            meta.append([counts[dst], nnull if dst == target else 0, offsets[src]])
        got = torch.cat(blocks).contiguous()
        mv, mn = sum(m[0] for m in meta), sum(m[1] for m in meta)
        meta_t = torch.tensor(meta, dtype=torch.int64).to(device)
        keys = torch.empty(max(mv, 1), dtype=torch.int64, device=device)
        grows = torch.empty(max(mv, 1), dtype=torch.int64, device=device)
        nrows = torch.empty(max(mn, 1), dtype=torch.int64, device=device)
        amd._lib.check(lib.arx_sort_unpack_records(got.data_ptr(), mv + mn, meta_t.data_ptr(), P_, int(nulls_first),
                                                   keys.data_ptr(), grows.data_ptr(), nrows.data_ptr(), stream))
        karr = amd.Array(amd.array.uint64, mv, [None, keys.view(torch.uint8)], 0, 0)
        perm = amd.compute.sort_indices(karr).data[: mv * 8].view(torch.int64)
        piece = grows[:mv][perm]
        out.append(torch.cat([nrows[:mn], piece]) if nulls_first else torch.cat([piece, nrows[:mn]]))
    if window is not None:
        assert min(int(o.numel()) for o in out) > sum(a.length for a in shards) // (2 * P_), "every rank gets its share"
    got = torch.cat(out).cpu().numpy().astype(np.uint64)
    vals = np.concatenate([a.values[a.offset:a.offset + a.length] for a in shards])
    valid = np.concatenate([np.ones(a.length, bool) if a.valid is None else a.valid[a.offset:a.offset + a.length] for a in shards])
    want = O.sort_indices_64(np.ascontiguousarray(vals), O.pack_bits(valid), 0, len(vals), descending=True,
                             nulls_at_start=nulls_first)
    assert (got == want).all()


@pytest.mark.parametrize("dtype", [np.float64, np.uint64, np.int32])
def test_sort_msd_sampled_splitters(gpu_ctx, dtype):
    """The sampled-splitter form of the MSD sort forced on: skewed keys (normal floats, clustered
    integers), duplicates-heavy columns (a bucket overflows -> LSD fallback), nulls, descending."""
    lib = gpu_ctx._lib.get_lib()
    with U.options(lib, {b"sort_msd_sampled": 2}):
        rng = rng_for("sampled", str(dtype))
        n = 4000003
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
            P.check_sort_indices(gpu_ctx, a, order, placement, use_pyarrow=(order == "ascending"))
        dup = U.random_array(rng, dtype, n, lo=None if np.dtype(dtype).kind == "f" else 0, hi=None if np.dtype(dtype).kind == "f" else 3)
        if np.dtype(dtype).kind == "f":
            dup.values[:] = np.round(dup.values)
        P.check_sort_indices(gpu_ctx, dup, "ascending", "at_end", use_pyarrow=False)


# ------------------------------------------------------------------ binary / utf8 take + filter
@pytest.mark.parametrize("idx_dtype", [np.uint8, np.int16, np.uint32, np.int64])
@pytest.mark.parametrize("vnull,inull", [(0.0, 0.0), (0.2, 0.0), (0.0, 0.1), (0.3, 0.3)])
def test_binary_take(gpu_ctx, idx_dtype, vnull, inull):
    rng = rng_for("btake", idx_dtype, vnull, inull)
    nv = 100 if np.dtype(idx_dtype).itemsize == 1 else 30_000
    v = U.random_binary(rng, nv, null_p=vnull, offset=3, tail=2, utf8=True)
    i = U.random_array(rng, idx_dtype, 200_003, null_p=inull, offset=1, lo=0, hi=nv - 1)
    P.check_binary_take(gpu_ctx, v, i)


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 4095, 4096, 4097, 1_000_003])
def test_binary_take_lengths(gpu_ctx, m):
    rng = rng_for("btakelen", m)
    v = U.random_binary(rng, 5000, null_p=0.1, max_len=40)
    i = U.random_array(rng, np.int32, m, null_p=0.1, lo=0, hi=4999)
    P.check_binary_take(gpu_ctx, v, i)


def test_binary_take_edges(gpu_ctx):
    rng = rng_for("btakeedge")
    i = U.random_array(rng, np.int32, 20_000, lo=0, hi=63)
    out = P.check_binary_take(gpu_ctx, U.random_binary(rng, 64, null_p=1.0), i)
    assert out.null_count == 20_000
    P.check_binary_take(gpu_ctx, U.random_binary(rng, 64, empty_p=1.0), i)
    P.check_binary_take(gpu_ctx, U.random_binary(rng, 64, max_len=2000, empty_p=0.0), i)   # long values
    v = U.random_binary(rng, 10)
    idx = U.HostArray(np.array([0, 3, 10, 2], dtype=np.int32), None, 0, 4)
    with pytest.raises(gpu_ctx.ArrowIndexError, match="Index 10 out of bounds"):
        gpu_ctx.compute.take(v.to_device(gpu_ctx), idx.to_device(gpu_ctx))


def test_binary_take_offset_overflow(gpu_ctx):
    """2^20 copies of a 4 KiB value do not fit int32 offsets: an error, as in the reference
    (the offset builder of the var-binary take overflows)."""
    rng = rng_for("btakeovf")
    v = U.random_binary(rng, 4, max_len=4096, empty_p=0.0)
    v.offsets[:] = np.arange(len(v.offsets), dtype=np.int32) * 1024   # every value 1 KiB
    v.data = np.zeros(int(v.offsets[-1]), np.uint8)
    i = U.HostArray(np.zeros(1 << 22, np.int32), None, 0, 1 << 22)    # 4 GiB of output
    with pytest.raises(gpu_ctx.ArrowInvalid, match="overflow"):
        gpu_ctx.compute.take(v.to_device(gpu_ctx), i.to_device(gpu_ctx))


@pytest.mark.parametrize("sel", ["drop", "emit_null"])
@pytest.mark.parametrize("true_p,vnull,mnull", [(0.0, 0.1, 0.0), (0.1, 0.0, 0.0), (0.5, 0.2, 0.1), (1.0, 0.1, 0.05)])
def test_binary_filter(gpu_ctx, sel, true_p, vnull, mnull):
    rng = rng_for("bfilter", sel, true_p, vnull, mnull)
    n = 300_007
    v = U.random_binary(rng, n, null_p=vnull, offset=5, tail=3)
    m = U.random_mask(rng, n, true_p, null_p=mnull, offset=2, tail=1)
    P.check_binary_filter(gpu_ctx, v, m, sel)


def test_binary_take_many_tiny_values(gpu_ctx):
    """0/1-byte values: a 16 KiB output chunk spans many more rows than one LDS batch holds."""
    rng = rng_for("btaketiny")
    v = U.random_binary(rng, 4000, null_p=0.1, max_len=1, empty_p=0.5)
    i = U.random_array(rng, np.int32, 2000000, null_p=0.05, lo=0, hi=3999)
    P.check_binary_take(gpu_ctx, v, i)


def test_add_and_greater_with_a_scalar_operand(gpu_ctx):
    P.check_scalar_operand_ops(gpu_ctx, rng_for("scalarops"), n=300007)


# ------------------------------------------------------------------ hash_min / hash_max on the fused table
@pytest.mark.parametrize("skip_nulls", [True, False])
@pytest.mark.parametrize("knull,vnull,batches,groups", [(0.0, 0.0, 1, 1000), (0.02, 0.2, 3, 100_000), (1.0, 0.5, 1, 10),
                                                        (0.1, 1.0, 2, 50)])
def test_groupby_min_max(gpu_ctx, skip_nulls, knull, vnull, batches, groups):
    rng = rng_for("gbminmax", skip_nulls, knull, vnull, batches)
    n = 400_003
    k = U.random_array(rng, np.int32, n, null_p=knull, offset=2, lo=-groups, hi=groups)
    v = U.random_array(rng, np.int64, n, null_p=vnull, offset=1)
    v.values[5:9] = [2**63 - 1, -2**63, 0, -1]
    P.check_groupby_min_max(gpu_ctx, k, v, skip_nulls, batches=batches, use_pyarrow=(groups <= 1000))


@pytest.mark.parametrize("skip_nulls,min_count,knull,vnull,batches", [(True, 1, 0.0, 0.0, 1), (False, 1, 0.05, 0.2, 3),
                                                                        (True, 0, 0.1, 1.0, 2), (True, 3, 0.02, 0.5, 1)])
def test_groupby_mean_int64(gpu_ctx, skip_nulls, min_count, knull, vnull, batches):
    """hash_mean(int64) (GroupedMeanImpl: doubles summed in row order) = (double)sum / count bit for bit while every
    partial sum is an exact integer; all-null groups, min_count = 0 (0 / 0 = NaN), !skip_nulls."""
    rng = rng_for("gmean", skip_nulls, min_count, knull, vnull, batches)
    n = 2000000
    k = U.random_array(rng, np.int32, n, null_p=knull, offset=2, lo=-40, hi=40)
    v = U.random_array(rng, np.int64, n, null_p=vnull, offset=1, lo=-2**31, hi=2**31)
    P.check_groupby_mean(gpu_ctx, k, v, skip_nulls, min_count, batches=batches)


def test_groupby_mean_declines_where_the_reference_is_order_dependent(gpu_ctx):
    """Values near 2^62: the reference's double partial sums are rounded differently for different row orders,
    so there is nothing to be bit-exact with — NotImplemented with the reason, never a wrong number."""
    rng = rng_for("gmean-big")
    k = U.random_array(rng, np.int32, 5000, lo=0, hi=10)
    v = U.random_array(rng, np.int64, 5000, lo=2**60, hi=2**62)
    P.check_groupby_mean(gpu_ctx, k, v, expect_decline=True)


@pytest.mark.parametrize("in_name", list(P.NUMERIC_TYPES))
def test_cast_every_numeric_pair(gpu_ctx, in_name):
    """CastIntegerToInteger / CastFloatingToInteger / CastIntegerToFloating / CastFloatingToFloating
    (scalar_cast_numeric.cc:46-60, 190-207, 270-279) for all 10 x 10 numeric pairs, safe and unsafe."""
    rng = rng_for("castpair", in_name)
    for out_name in P.NUMERIC_TYPES:
        if out_name != in_name:
            P.check_cast_numeric_pair(gpu_ctx, rng, in_name, out_name, n=300000)


def test_cast_at_the_type_boundaries(gpu_ctx):
    """All 100 pairs on the values at their own limits -- hi, hi + 1, lo, lo - 1, +-2^24, +-2^53, 2^31, 2^63, 2^64, NaN, inf,
    -0.0, DBL_MAX: the decision, the whole error text and the result bits, safe and unsafe (P.check_cast_boundaries)."""
    assert P.check_cast_boundaries(gpu_ctx) > 1500


@pytest.mark.parametrize("pair", P.LONE_OFFENDER_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_cast_names_a_lone_offender_wherever_it_is(gpu_ctx, pair):
    """One failing row at the wave / block / tile / tail edges of a 4099-row array, under a null, and two of them in
    different blocks (the atomicMin over blocks), for one pair per checking path of arx_cast_numeric."""
    P.check_cast_lone_offender(gpu_ctx, pair)


@pytest.mark.parametrize("dtype", ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"])
def test_checked_arithmetic_with_one_overflowing_row(gpu_ctx, dtype):
    """add / subtract / multiply (+ _checked) with a single overflowing row at every edge position and both slice offsets,
    array x array and both scalar orders; nulls on either side hide it."""
    P.check_arith_lone_overflow(gpu_ctx, np.dtype(dtype))


def test_add_pair_kernel_rows_and_tail(gpu_ctx):
    """Unchecked int64 / float64 add (the pair-loading add_kernel) on rows that all differ, odd length, both offsets."""
    P.check_add_pair_kernel_tail(gpu_ctx)


@pytest.mark.parametrize("dtype", ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"])
def test_divide_error_of_the_later_row(gpu_ctx, dtype):
    """A zero divisor and min / -1 in different blocks, in both orders: divide_checked names the later one."""
    P.check_divide_ordering(gpu_ctx, np.dtype(dtype))


@pytest.mark.parametrize("dtype", list(P.NUMERIC_TYPES))
def test_compare_and_arithmetic_over_the_whole_type(gpu_ctx, dtype):
    """Operands from the type's edges and its whole range (an unsigned comparison done as signed fails here)."""
    P.check_compare_whole_range(gpu_ctx, rng_for("whole-range", dtype), P.NUMERIC_TYPES[dtype])


@pytest.mark.parametrize("key_dtype", [np.int8, np.uint16, np.uint32, np.int64, np.uint64])
def test_groupby_sum_other_key_and_value_types(gpu_ctx, key_dtype):
    rng = rng_for("gbtyped", str(key_dtype))
    for value_dtype in (np.int8, np.int32, np.uint32, np.uint64, np.int64):
        P.check_groupby_sum_typed(gpu_ctx, rng, key_dtype, value_dtype, n=400000)


def test_groupby_declines_what_it_cannot_reproduce(gpu_ctx):
    """64-bit keys beyond the int32 range (the device table holds 32-bit keys) and floating-point sums (row-order
    double accumulation in the reference) are NotImplemented with the reason — never a wrong answer."""
    amd = gpu_ctx
    op = amd.compute.GroupBySum(64)
    with pytest.raises(NotImplementedError, match="beyond the int32 range"):
        op.consume(amd.Array.from_numpy(np.array([1, 2**40], dtype=np.int64)), amd.Array.from_numpy(np.array([1, 2], dtype=np.int64)))
    op = amd.compute.GroupBySum(64)
    with pytest.raises(NotImplementedError, match="row order"):
        op.consume(amd.Array.from_numpy(np.array([1, 2], dtype=np.int32)), amd.Array.from_numpy(np.array([1.0, 2.0])))


@pytest.mark.parametrize("dtype", [np.bool_, np.int8, np.uint16, np.int32, np.uint64, np.int64, np.float32, np.float64])
def test_indices_nonzero(gpu_ctx, dtype):
    """IndicesNonZero (kernels/vector_selection.cc:352): uint64 positions of the valid, non-zero elements vs pyarrow."""
    import pyarrow as pa
    import pyarrow.compute as pc

    rng = rng_for("nonzero", str(dtype))
    for n in (0, 5, 70000, 3000001):
        x = rng.integers(0, 3, n).astype(dtype) if dtype != np.bool_ else rng.random(n) < 0.3
        valid = rng.random(n) > 0.1
        got = gpu_ctx.compute.indices_nonzero(gpu_ctx.Array.from_numpy(x, valid if n else None))
        want = pc.indices_nonzero(pa.array(x, mask=(~valid) if n else None))
        assert got.type.name == "uint64" and np.array_equal(got.to_numpy()[0], want.to_numpy()), (dtype, n)


@pytest.mark.parametrize("dtype", [np.int64, np.uint64, np.int32, np.uint32, np.float64, np.float32])
def test_golden_sort_and_sum_only_replay(gpu_ctx, dtype):
    """The reference's own known-answer tests for the two sharded paths (vector_sort_test.cc:640-724,
    acero/hash_aggregate_test.cc:839-883; tests/golden/reference_vectors.json) replayed on the kernels."""
    import json
    import os

    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.json")))
    assert P.replay_golden_sort(gpu_ctx, gold, dtype) >= 20
    P.replay_golden_sum_only(gpu_ctx, gold)


@pytest.mark.parametrize("run_end_type", ["int16", "int32", "int64"])
def test_filter_with_a_run_end_encoded_mask(gpu_ctx, run_end_type):
    """array_filter(values, run_end_encoded<boolean>) (vector_selection_filter_internal.cc:1090): sliced masks, null run
    values, DROP and EMIT_NULL, vs the reference (pyarrow)."""
    import pyarrow as pa
    import pyarrow.compute as pc

    amd = gpu_ctx
    rng = rng_for("reemask", run_end_type)
    ret = {"int16": pa.int16(), "int32": pa.int32(), "int64": pa.int64()}[run_end_type]
    for n in (1, 64, 20000, 3_000_001):
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


def test_groupby_min_max_next_to_sum_and_merge(gpu_ctx):
    amd = gpu_ctx
    rng = rng_for("gbminmaxsum")
    k = U.random_array(rng, np.int32, 300_000, null_p=0.02, lo=0, hi=5000)
    v = U.random_array(rng, np.int64, 300_000, null_p=0.1, lo=-10**9, hi=10**9)
    P.check_groupby_min_max(amd, k, v, True, batches=2, with_sum=True)
    dk, dv = k.to_device(amd), v.to_device(amd)
    a, b = amd.compute.GroupBySum(1 << 14, dk.device), amd.compute.GroupBySum(1 << 14, dk.device)
    a.consume_min_max(dk.slice(0, 170_000), dv.slice(0, 170_000))
    b.consume_min_max(dk.slice(170_000), dv.slice(170_000))
    a.merge_min_max(b.export_min_max())
    gk, gkv, gmin, gmax, gvalid = (x.cpu().numpy() for x in a.finalize_min_max())
    w = O.groupby_minmax_i64(k.values, k.valid_bitmap(), 0, v.values, v.valid_bitmap(), 0, 300_000, True)
    key = lambda r: (r[0] is None, r[0] or 0)  # noqa: E731
    got = sorted(((int(x) if y else None, (int(c), int(d)) if e else None) for x, y, c, d, e in zip(gk, gkv, gmin, gmax, gvalid)), key=key)
    want = sorted(((int(x) if y else None, (int(c), int(d)) if e else None)
                   for x, y, c, d, e in zip(w["keys"], w["key_is_valid"], w["mins"], w["maxs"], w["valid"])), key=key)
    assert got == want


@pytest.mark.parametrize("null_p,offset", [(0.0, 0), (0.05, 3), (1.0, 1)])
def test_unique_and_value_counts(gpu_ctx, null_p, offset):
    """UniqueAction / ValueCountsAction (vector_hash.cc): first-appearance order from the fused table."""
    rng = rng_for("unique", null_p, offset)
    a = U.random_array(rng, np.int32, 500003, null_p=null_p, offset=offset, tail=2, lo=-60000, hi=60000)
    P.check_unique_and_value_counts(gpu_ctx, a)
    P.check_unique_and_value_counts(gpu_ctx, U.random_array(rng, np.int32, 0))
    P.check_unique_and_value_counts(gpu_ctx, U.random_array(rng, np.int32, 1, null_p=null_p))


@pytest.mark.parametrize("lnull,rnull,loff,roff", [(0.0, 0.0, 0, 0), (0.2, 0.0, 3, 0), (0.0, 0.3, 0, 65), (0.3, 0.3, 7, 13), (1.0, 0.5, 1, 2)])
def test_kleene_and_or_invert(gpu_ctx, lnull, rnull, loff, roff):
    """KleeneAndOp / KleeneOrOp / InvertOp (scalar_boolean.cc): the full truth table incl. nulls,
    sliced operands with different bit offsets."""
    rng = rng_for("kleene", lnull, rnull, loff, roff)
    left = U.random_mask(rng, 1000003, 0.5, null_p=lnull, offset=loff, tail=3)
    right = U.random_mask(rng, 1000003, 0.4, null_p=rnull, offset=roff, tail=5)
    P.check_kleene_and_invert(gpu_ctx, left, right)
    P.check_kleene_and_invert(gpu_ctx, U.random_mask(rng, 0, 0.5), U.random_mask(rng, 0, 0.5))


def test_compare_family(gpu_ctx):
    """Equal ... LessEqual (scalar_compare.cc:38-64): int64 and float64 incl. NaN / signed zeros / infinities."""
    P.check_compare_family(gpu_ctx, rng_for("cmpfamily"), n=300007)


def test_subtract_multiply_and_checked_arithmetic(gpu_ctx):
    """Subtract / Multiply / *Checked (base_arithmetic_internal.h): wrap-around vs "overflow" on valid slots only."""
    P.check_arithmetic(gpu_ctx, rng_for("arith"), n=300007)


def test_integer_casts(gpu_ctx):
    """CastIntegerToInteger (scalar_cast_numeric.cc:46-54) + IntegersInRange's first-offender message."""
    P.check_integer_casts(gpu_ctx, rng_for("intcast"), n=400003)
    P.check_cast_i64_f64(gpu_ctx, rng_for("i64f64"), n=400003)


@pytest.mark.parametrize("null_p,offset", [(0.0, 0), (0.07, 3)])
def test_dictionary_encode(gpu_ctx, null_p, offset):
    """DictEncodeAction (vector_hash.cc:173-270): MASK and ENCODE null handling, first-appearance dictionary."""
    rng = rng_for("dictenc", null_p, offset)
    a = U.random_array(rng, np.int32, 500003, null_p=null_p, offset=offset, tail=2, lo=-40000, hi=40000)
    P.check_dictionary_encode(gpu_ctx, a)
    P.check_dictionary_encode(gpu_ctx, U.random_array(rng, np.int32, 0))


# ------------------------------------------------------------------ boolean values, scalar aggregates, divide, concatenate, order_by
@pytest.mark.parametrize("idx_dtype", [np.uint8, np.int32, np.int64])
@pytest.mark.parametrize("vnull,inull,voff", [(0.0, 0.0, 0), (0.2, 0.1, 5), (1.0, 0.5, 67)])
def test_boolean_values_take_and_filter(gpu_ctx, idx_dtype, vnull, inull, voff):
    """filter / take on BOOLEAN values (1-bit Gather, gather_internal.h; PrimitiveFilter's bit-width-1 case)."""
    rng = rng_for("booltake", str(idx_dtype), vnull, inull, voff)
    nv = 200 if np.dtype(idx_dtype).itemsize == 1 else 500003
    v = U.random_mask(rng, nv, 0.5, null_p=vnull, offset=voff, tail=3)
    i = U.random_array(rng, idx_dtype, 500003, null_p=inull, offset=1, lo=0, hi=nv - 1)
    m = U.random_mask(rng, nv, 0.3, null_p=0.05, offset=2)
    P.check_boolean_take_and_filter(gpu_ctx, v, i, m)


def test_scalar_aggregates_int64(gpu_ctx):
    """SumImpl / CountImpl / MinMaxImpl (aggregate_basic.inc.cc): wrap-around sum, options, batches."""
    P.check_scalar_aggregates(gpu_ctx, rng_for("scalaragg"), n=1000003)


def test_divide_and_divide_checked(gpu_ctx):
    """Divide / DivideChecked (base_arithmetic_internal.h:366-424) through the C ABI against the oracle and pyarrow."""
    P.check_divide(gpu_ctx, rng_for("divide"), n=300_007)


@pytest.mark.parametrize("dtype", ["int8", "uint8", "int16", "uint16", "int32", "uint32", "uint64", "float32"])
def test_divide_on_the_other_numeric_types(gpu_ctx, dtype):
    """arx_divide_numeric through the C ABI against the oracle and pyarrow, one element type at a time."""
    P.check_divide(gpu_ctx, rng_for("divide-" + dtype), n=200_003, dtypes=(np.dtype(dtype),))


@pytest.mark.parametrize("kind", ["int64", "int8", "bool", "utf8", "binary_nonull"])
def test_concat_arrays(gpu_ctx, kind):
    """Concatenate (array/concatenate.cc): sliced chunks glued at arbitrary bit positions, empty chunks."""
    rng = rng_for("concat", kind)
    specs = [(77, 0.2, 3), (0, 0.0, 0), (1, 0.0, 0), (130_001, 0.0, 65), (64, 1.0, 7), (300_000, 0.1, 0), (5, 0.5, 1)]
    if kind == "bool":
        chunks = [U.random_mask(rng, n, 0.5, null_p=p, offset=o, tail=2) for n, p, o in specs]
    elif kind in ("utf8", "binary_nonull"):
        chunks = [U.random_binary(rng, n, null_p=0.0 if kind == "binary_nonull" else p, offset=o, tail=2, utf8=kind == "utf8")
                  for n, p, o in specs]
    else:
        chunks = [U.random_array(rng, np.dtype(kind).type, n, null_p=p, offset=o, tail=2) for n, p, o in specs]
    P.check_concat_arrays(gpu_ctx, chunks)
    P.check_concat_arrays(gpu_ctx, chunks[1:2])
    P.check_concat_arrays(gpu_ctx, [chunks[3]])


@pytest.mark.parametrize("null_placement", ["at_end", "at_start"])
def test_order_by_several_keys(gpu_ctx, null_placement):
    """OrderByNode::DoFinish (acero/order_by_node.cc:100-108) with up to three keys of mixed direction and
    per-key null placement; few distinct values per key, NaNs in the float key, payload columns ride along."""
    rng = rng_for("orderby", null_placement)
    sizes = [(32_768, 3), (0, 0), (32_768, 0), (20_001, 5)]

    def col(make):
        return [make(n, o) for n, o in sizes]

    def fkey(n, o):
        a = U.random_array(rng, np.float64, n, null_p=0.1, offset=o, tail=1)
        a.values[:] = np.round(a.values * 2) / 2
        a.values[rng.random(len(a.values)) < 0.1] = np.nan
        return a

    k0 = col(lambda n, o: U.random_array(rng, np.int32, n, null_p=0.1, offset=o, tail=1, lo=-30, hi=30))
    k1 = col(lambda n, o: U.random_array(rng, np.int64, n, null_p=0.1, offset=o, tail=1, lo=0, hi=40))
    k2 = col(fkey)
    payload = col(lambda n, o: U.random_array(rng, np.int64, n, null_p=0.2, offset=o, tail=1))
    strs = col(lambda n, o: U.random_binary(rng, n, null_p=0.1, offset=o, tail=1, utf8=True))
    flags = col(lambda n, o: U.random_mask(rng, n, 0.5, null_p=0.1, offset=o, tail=1))
    cols = [k0, k1, k2, payload, strs, flags]
    P.check_order_by(gpu_ctx, cols, [(0, "ascending"), (1, "descending")], null_placement)
    P.check_order_by(gpu_ctx, cols, [(2, "descending"), (0, "descending"), (1, "ascending")], null_placement)
    other = "at_start" if null_placement == "at_end" else "at_end"
    P.check_order_by(gpu_ctx, cols, [(0, "descending"), (2, "ascending")], [null_placement, other])


# The device Grouper (csrc/grouper.hip): round 2 left these tests opt-in after two GPU calls that coincided with lost
# boxes; round 3 ran every one of them on gfx950 in its own process under a wall-clock kill (scripts/gpu_r03_grouper.sh,
# profiles/r03_d_grouper_gpu_tests.txt: 13 of 13 green, no hang) and they are part of the default `-m gpu` run again.
@pytest.mark.parametrize("section,combos", [("grouper_numeric_key", None), ("grouper_floating_point_key", None),
                                            ("grouper_multiple_int_keys", 60)])
def test_reference_grouper_golden_vectors(gpu_ctx, section, combos):
    """grouper_test.cc's own expectations (exact ids in first-appearance order, uniques, Lookup nulls) on the device
    Grouper."""
    import json
    import os

    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_vectors.json")))
    assert P.replay_golden_grouper(gold, section, P.device_grouper_factory(gpu_ctx), combos) > 0


@pytest.mark.parametrize("dtypes,n,card,null_p,batches", [
    ((np.int64,), 2_000_000, 300_000, 0.05, 1), ((np.int64,), 1_000_000, 999_999, 0.0, 3),
    ((np.uint64,), 3_000_000, 5, 0.3, 2), ((np.int32, np.int32), 2_000_000, 900, 0.1, 2),
    ((np.int64, np.int64), 1_000_000, 200_000, 0.1, 1), ((np.int8, np.int16, np.int32, np.int64), 500_000, 400_000, 0.05, 4),
    ((np.float64, np.uint8), 300_000, 50, 0.2, 1), ((np.int16,), 0, 1, 0.0, 1), ((np.uint8,) * 8, 400_000, 100, 0.1, 2)])
def test_grouper_ids_uniques_lookup(gpu_ctx, dtypes, n, card, null_p, batches):
    P.check_grouper(gpu_ctx, rng_for("grouper", len(dtypes), n, card, batches), dtypes, n, card, null_p, batches)


def test_grouper_hot_keys_and_overflow(gpu_ctx):
    """Every row hits one of 3 keys while they are being inserted (the pending-list path), and a table that is too
    small fails the call instead of corrupting ids."""
    P.check_grouper(gpu_ctx, rng_for("grouper-hot"), (np.int64, np.int64), 4_000_000, 3, 0.0, 1, max_groups=16)
    from arrow_amd.array import int64

    g = gpu_ctx.compute.Grouper([int64], 1000)
    with pytest.raises(ValueError, match="more than 1000 distinct key rows"):
        g.consume([gpu_ctx.Array.from_numpy(np.arange(100_000, dtype=np.int64))])


@pytest.mark.parametrize("dtypes,n,card,null_p", [((np.int64,), 600_000, 200_000, 0.05),      # (sizes: the row-by-row checker
                                                  ((np.int32, np.int32), 150_000, 800, 0.1),    #  is what takes the time here)
                                                  ((np.int64, np.int16), 250_000, 200_000, 0.0)])
def test_group_by_wide_and_multiple_keys(gpu_ctx, dtypes, n, card, null_p):
    P.check_group_by_keys(gpu_ctx, rng_for("group_by_keys", len(dtypes), n, card), dtypes, n, card, null_p)


@pytest.mark.parametrize("dtypes,n,m,idx_dtype", [
    ((np.int64, np.int32, np.float64), 3_000_000, 1_000_003, np.uint32),
    ((np.int8, np.int16, np.int64, np.uint64, np.float32), 77_777, 2_000_000, np.int64),
    ((np.int64,) * 17, 30_000, 500_000, np.uint16),
    ((np.int32, np.int64), 1000, 0, np.int32), ((np.int64, np.int64), 64, 64, np.uint8)])
def test_take_record_batch_in_one_launch(gpu_ctx, dtypes, n, m, idx_dtype):
    P.check_take_record_batch(gpu_ctx, rng_for("take-rb", len(dtypes), n, m), dtypes, n, m, idx_dtype)


def test_take_record_batch_without_nulls_has_no_bitmaps(gpu_ctx):
    rng = rng_for("take-rb-nonull")
    P.check_take_record_batch(gpu_ctx, rng, (np.int64, np.int32), 400_000, 1 << 20, np.uint32, value_null_p=0.0,
                              index_null_p=0.0, offsets=False)


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64,
                                   np.float32, np.float64])
def test_compare_and_arithmetic_on_every_numeric_type(gpu_ctx, dtype):
    P.check_numeric_compare_arith(gpu_ctx, rng_for("numeric-ops", np.dtype(dtype).name), dtype, n=300007)


@pytest.mark.parametrize("wide", [0, 1])
def test_sort_keys_with_a_shared_prefix(gpu_ctx, wide):
    lib = gpu_ctx._lib.get_lib()
    P.check_sort_limited_range(gpu_ctx, lib, rng_for("sort-prefix", wide), 2000003, wide)


def test_compare_on_temporal_columns(gpu_ctx):
    P.check_temporal_compare(gpu_ctx, rng_for("temporal-compare"), n=700003)


def test_copy_segments_any_alignment(gpu_ctx):
    P.check_copy_segments(gpu_ctx, rng_for("copyseg"), 40)


@pytest.mark.parametrize("n,num_groups,null_p", [(2000000, 300000, 0.2), (1000000, 5, 0.0), (300, 1, 1.0)])
def test_hash_minmax_and_count_dense_kernels(gpu_ctx, n, num_groups, null_p):
    P.check_hash_minmax_count_kernels(gpu_ctx, rng_for("hmmc", n, num_groups), n=n, num_groups=num_groups, null_p=null_p)


@pytest.mark.parametrize("dtype,n,num_groups,null_p", [(np.float64, 2000000, 300000, 0.2), (np.float32, 1000000, 5, 0.0), (np.float64, 300, 1, 1.0)])
def test_hash_minmax_float_dense_kernels(gpu_ctx, dtype, n, num_groups, null_p):
    P.check_hash_minmax_float_kernels(gpu_ctx, rng_for("hmmf", n, num_groups), dtype=dtype, n=n, num_groups=num_groups, null_p=null_p)


def test_float_sum_is_the_references_bit_for_bit_and_float_min_max(gpu_ctx):
    P.check_sum_float(gpu_ctx, rng_for("fsum"), [0, 1, 17, 4097, 32768, 32769, 1000003, 16777216 + 12345])


def test_coalesce_of_two_operands_is_fill_null(gpu_ctx):
    P.check_coalesce2(gpu_ctx, rng_for("coalesce2"), n=1000003)


def test_take_of_rows_of_any_width_and_of_lists_with_fixed_width_values(gpu_ctx):
    """fixed_size_list / list / large_list selection where the nested values are fixed-width and free of nulls
    (FSLTakeExec -> FixedWidthTakeExec; ListSelectionImpl): arx_take_rows and arx_(large_)list_take_data."""
    P.check_take_rows(gpu_ctx, rng_for("takerows"), n=300000, m=250000)
    P.check_list_take(gpu_ctx, rng_for("listtake"), n=300000, m=250000)


def test_grouped_float_sum_is_the_references_row_order_sum(gpu_ctx):
    """hash_sum / hash_mean of float32 / float64 values over dense group ids: the reference's row-order double accumulation
    per group, bit for bit (stable sort by group id + one walker per group)."""
    P.check_hash_sum_float(gpu_ctx, rng_for("hashfsum"), n=300000, groups=(1, 7, 300, 100000))


def test_grouped_decimal128_sum(gpu_ctx):
    """hash_sum / hash_min / hash_max of decimal128 values over dense group ids: 128-bit sums modulo 2^128 kept with two atomics
    per row; extrema in signed 128-bit order by one owner per group over the rows sorted by group id."""
    P.check_hash_sum_dec128(gpu_ctx, rng_for("hashdec"), n=60000, groups=(1, 13, 4000))
    P.check_hash_minmax_dec128(gpu_ctx, rng_for("hashdecmm"), n=60000, groups=(1, 13, 4000))
    P.check_reduce_dec128(gpu_ctx, rng_for("reducedec"), sizes=(0, 1, 65, 70001, 3000017))


def test_buffer_copy(gpu_ctx):
    P.check_buffer_copy(gpu_ctx, rng_for("bufcopy"), 40)


def test_bytes_to_bitmap(gpu_ctx):
    P.check_bytes_to_bitmap(gpu_ctx, rng_for("bytes-to-bitmap"), scale=30)


def test_groupby_key_range(gpu_ctx):
    P.check_groupby_key_range(gpu_ctx, rng_for("key-range"), scale=50)


@pytest.mark.parametrize("n", [100_003, 6_000_011, 150_000_001])
def test_sort_records(gpu_ctx, n):
    """Round 6: arx_sort_records on gfx950 — the LSD fallback, the MSD hybrid (> 4M records) and the wide form (> 2^27)."""
    P.check_sort_records(gpu_ctx, rng_for("sort-records", n), n)


def test_groupby_range_state(gpu_ctx):
    """Round 6: the range-partitioned state through its C ABI on gfx950, 20x the emulated tier's rows, the 12288-wide partitions."""
    P.check_groupby_range_state(gpu_ctx, rng_for, scale=20)


def test_groupby_lines_plan(gpu_ctx):
    """Round 6: the dense-range lines plan (write-combined whole-line scatter + direct-indexed LDS aggregate) on gfx950:
    every case of the emulated tier at 20x the rows, plus the 12288- and 8192-wide partitions."""
    P.check_groupby_lines_plan(gpu_ctx, rng_for, scale=20, wide_width=True)


def test_hash_any_all_dense_kernels(gpu_ctx):
    P.check_hash_any_all_kernels(gpu_ctx, rng_for("hash-bool"), n=600_000, num_groups=5000)


def test_bitmap_copy_segments(gpu_ctx):
    P.check_bitmap_copy_segments(gpu_ctx, rng_for("bitseg"), 20)


@pytest.mark.gpu
def test_hash_product_group_edge_rows_and_dec128_split(gpu_ctx):
    """The C-ABI entry points behind hash_product / hash_first / hash_last / hash_one and the decimal128 sort keys against the
    oracle's restatements of GroupedProductImpl, GroupedFirstLastImpl and GroupedOneImpl."""
    P.check_hash_product_and_edge_rows(gpu_ctx, rng_for("hashprod"), n=200000, groups=(1, 7, 300, 50000))



def test_group_moments_variance_stddev_skew_kurtosis(gpu_ctx):
    """hash_variance / hash_stddev / hash_skew / hash_kurtosis: the two-pass moments kernels against the oracle's restatement
    of GroupedStatisticImpl (kernels/hash_aggregate_numeric.cc:457-843)."""
    P.check_group_moments(gpu_ctx, rng_for("moments"))

def test_rank(gpu_ctx):
    """Round 6 (f3): rank / rank_quantile = arx_sort_indices + arx_rank against the oracle's restatement of vector_rank.cc and the
    known answers of the reference's TestRank."""
    P.check_rank(gpu_ctx, rng_for, scale=10)


def test_select_k_and_partition_nth(gpu_ctx):
    """Round 6 (f3): select_k_unstable / partition_nth_indices on the sort skeleton — the promised properties."""
    P.check_select_k_partition_nth(gpu_ctx, rng_for, scale=10)


def test_sort_boolean_keys(gpu_ctx):
    """Round 6 (f3): boolean sort keys — the counting sort as three GetTakeIndices."""
    P.check_sort_boolean_keys(gpu_ctx, rng_for, scale=100)


# ------------------------------------------------------------------ every compaction form the dispatch can choose
FORM_CELLS = [(w, f) for w in (1, 2, 4, 8, 16) for f in (P.COMPACT_GATHER, P.COMPACT_SWEEP_PIPELINED, P.COMPACT_SWEEP_PLAIN,
                                                         P.COMPACT_SWEEP_UNALIGNED)] + [(32, P.COMPACT_GATHER)]
ROW_NUMBER_CELLS = [(2, P.COMPACT_GATHER), (2, P.COMPACT_SWEEP_PIPELINED), (2, P.COMPACT_SWEEP_PLAIN),
                    (4, P.COMPACT_GATHER), (4, P.COMPACT_SWEEP_PIPELINED), (4, P.COMPACT_SWEEP_PLAIN)]


def _form_id(cell):
    return f"W{cell[0]}-{P.COMPACT_FORM_NAMES[cell[1]]}"


@pytest.mark.parametrize("sel", ["drop", "emit_null"])
@pytest.mark.parametrize("cell", FORM_CELLS, ids=_form_id)
def test_filter_every_compaction_form(gpu_ctx, cell, sel):
    """arx_filter_count -> arx_filter_exec at the C ABI, one (width, kernel form, null selection) cell per test: the
    checker asserts with arx_filter_compact_form that the case runs the form it names before it launches, then
    compares every output byte and validity bit with numpy (P.filter_form_cases: lengths 1 .. 266 241, selectivities
    0 .. 1, four null densities, mask bit offsets 0 / 1 / 63, outputs 0 / 1 / 2048/W - 1 elements past a 2 KiB line)."""
    width, form = cell
    for kw in P.filter_form_cases(width, form, sel):
        P.check_filter_form(gpu_ctx, width, form, sel, **kw)


def test_filter_32_byte_values_have_no_sweep_form(gpu_ctx):
    P.check_filter_w32_sweep_is_refused(gpu_ctx)


@pytest.mark.parametrize("sel", ["drop", "emit_null"])
@pytest.mark.parametrize("cell", ROW_NUMBER_CELLS, ids=_form_id)
def test_mask_to_indices_every_form(gpu_ctx, cell, sel):
    """arx_mask_to_indices called directly, 2- and 4-byte row numbers under filter_sparse 1 (gather) and 0 (sweep, both
    batch forms).  Under the sweep, selectivity 0.3 keeps a tile's row numbers inside the LDS ring (each lane walks its
    own word), 1.0 does not (the 4096-row sweep)."""
    width, form = cell
    lengths = [1, 63, 4095, 4096, 4097, 3 * 4096 + 5] + ([65535] if width == 2 else [262144 + 4097])
    cases = [(n, 0.3) for n in lengths] + [(n, p) for n in lengths[-2:] for p in (0.0, 0.02, 1.0)]
    for i, (n, p) in enumerate(cases):
        P.check_mask_to_indices_form(gpu_ctx, width, form, sel, n, moff=(1, 63, 0)[i % 3], true_p=p,
                                     mnull=(0.3, 0.0, 0.05, 1.0)[i % 4] if n < 4096 or p != 0.3 else 0.3,
                                     disp=(1, P.kFlushBytes // width - 1, 0)[(i // 2) % 3])


def test_mask_to_indices_8_byte_row_numbers(gpu_ctx):
    """index_width 8: the gather form with DROP, refused (nothing written) under filter_sparse = 0 and for EMIT_NULL."""
    for i, (n, p) in enumerate([(1, 0.3), (63, 0.3), (4097, 0.3), (3 * 4096 + 5, 1.0), (262144 + 4097, 0.3), (262144 + 4097, 0.02)]):
        P.check_mask_to_indices_form(gpu_ctx, 8, P.COMPACT_GATHER, "drop", n, moff=(1, 63, 0)[i % 3], true_p=p,
                                     mnull=(0.3, 0.0)[i % 2], disp=(1, P.kFlushBytes // 8 - 1, 0)[i % 3])
    P.check_mask_to_indices_width8_refusals(gpu_ctx)


@pytest.mark.parametrize("invert", [0, 1])
def test_bitmap_to_indices(gpu_ctx, invert):
    """Positions of the set / clear bits; lengths that are no multiple of 64: inverted bits past the end must not appear.
    Clear bits at 70 % (the sweep) and, on the multi-tile lengths, at 10 % (each lane walks its own word)."""
    for n in (1, 64, 65, 4097, 262144 + 4097):
        for off in (0, 1, 63):
            P.check_bitmap_to_indices(gpu_ctx, n, off, invert)
    for n in (4097, 262144 + 4097):
        P.check_bitmap_to_indices(gpu_ctx, n, 63, invert, true_p=0.9)
        P.check_bitmap_to_indices(gpu_ctx, n, 1, invert, true_p=0.0)
        P.check_bitmap_to_indices(gpu_ctx, n, 1, invert, true_p=1.0)


@pytest.mark.parametrize("width", [1, 2, 4, 8, 16])
def test_expand_by_mask(gpu_ctx, width):
    for i, n in enumerate((1, 64, 65, 4097, 262144 + 4097)):
        P.check_expand_by_mask(gpu_ctx, width, n, (1, 63, 0)[i % 3], 0.0)
        P.check_expand_by_mask(gpu_ctx, width, n, (63, 0, 1)[i % 3], 0.2)


def test_every_compaction_form_cell_was_asserted(gpu_ctx):
    """Runs the 63-row case of every cell (so that this test stands alone), then reads the checker's own tally: every
    (kind, width, form, null selection) cell has cases whose arx_filter_compact_form assertion held.  Prints the tally:
    after a run of the whole file it holds the counts of the whole matrix."""
    for sel in ("drop", "emit_null"):
        for width, form in FORM_CELLS:
            P.check_filter_form(gpu_ctx, width, form, sel, 63, moff=1, mnull=0.3)
        for width, form in ROW_NUMBER_CELLS:
            P.check_mask_to_indices_form(gpu_ctx, width, form, sel, 63, moff=1, mnull=0.3)
    P.check_mask_to_indices_form(gpu_ctx, 8, P.COMPACT_GATHER, "drop", 63)
    for invert in (0, 1):
        P.check_bitmap_to_indices(gpu_ctx, 65, 1, invert)
    cells = [("values", w, P.COMPACT_FORM_NAMES[f], s) for w, f in FORM_CELLS for s in ("drop", "emit_null")]
    cells += [("row_numbers", w, P.COMPACT_FORM_NAMES[f], s) for w, f in ROW_NUMBER_CELLS for s in ("drop", "emit_null")]
    cells += [("row_numbers", 8, "gather", "drop"), ("bit_positions", 4, "gather", "drop")]
    for key in sorted(P.FORM_HITS):
        print("compaction form cases", *key, P.FORM_HITS[key])
    assert [c for c in cells if P.FORM_HITS.get(c, 0) == 0] == []
    assert any(k[0] == "bit_positions_inverted" and k[2].startswith("sweep") for k in P.FORM_HITS)
    assert not [k for k in P.FORM_HITS if k[1] == 32 and k[2] != "gather"]
