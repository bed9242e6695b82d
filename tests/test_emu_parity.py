"""Kernel-logic parity on the CPU: the *unchanged* kernel sources of arrow_amd/csrc compiled for
the host against tests/emu/hip_emu.h (a fiber-based SIMT emulator) and driven through the same
arrow_amd.compute -> C ABI path as on the GPU.  These are not GPU compute calls and not a CPU
fallback of the product: the emulated library is built and loaded by the tests only.
Sizes are small (the emulator context-switches at every wave collective).

The cases both tiers run are written once, in parity_tiers.define: this file runs them at the emulator's sizes and adds,
below them, the cases only this tier has."""
import numpy as np
import pytest

from . import parity_cases as P
from . import util as U
from .parity_tiers import EMU, check_min_max_merge_of_two_states, define, rng_for

pytestmark = pytest.mark.emu


@pytest.fixture
def ctx(emu_ctx):
    return emu_ctx


_shared = define(EMU)
test_filter_int64_probabilities = _shared.pop("test_filter_random_grid")             # (this tier's names for the two)
test_filter_dense_and_batch_variants = _shared.pop("test_filter_tuning_variants_agree")
globals().update(_shared)


# ------------------------------------------------------------------ this tier only
def test_filter_no_nulls_has_no_validity(emu_ctx):
    # the device tier asserts the same on its 10M-row benchmark shape (test_filter_10m_rows_config1)
    rng = rng_for("fnn")
    v = U.random_array(rng, np.int64, 5000)
    m = U.random_mask(rng, 5000, 0.5)
    out = P.check_filter(emu_ctx, v, m, "drop")
    assert out.validity is None and out.null_count == 0


# same name as the device tier's, another case: knob sets per row here (and a key that counts them), sizes alone there
@pytest.mark.parametrize("n,options", [(0, ()), (1, ()), (9000, ()), (30000, ((b"sort_msd", 1),)),
                                       (30000, ((b"sort_msd", 1), (b"sort_msd_sampled", 2))),
                                       (40000, ((b"sort_msd", 1), (b"sort_msd_segment_rows", 4096), (b"sort_msd_wide", 1), (b"sort_msd_wide_bits", 8))),
                                       (40000, ((b"sort_msd", 1), (b"sort_msd_segment_rows", 4096), (b"sort_msd_wide", 1), (b"sort_msd_wide_bits", 8),
                                                (b"sort_records_in_place", 0)))])
def test_sort_records(emu_ctx, n, options):
    """Round 6: arx_sort_records (the receiver of the sharded sort's records form) — LSD fallback, MSD hybrid, sampled
    splitters, the wide form on 12-byte records."""
    P.check_sort_records(emu_ctx, rng_for("sort-records", n, len(options)), n, options)


# same name as the device tier's, another case: emulator-only knob grid (wc_form, wc_min_rows) and a key of its own
@pytest.mark.parametrize("n,bits,gap2,shift,rpt,b2max,wc,prefetch,l2w,wc_form", [
    (120_000, 0, 1, 0, (24, 16), 11, 256, 1, 1, 2), (40_000, 12, 0, 2, (8, 8), 11, 0, 1, 2, 2),
    (40_000, 6, 1, 2, (16, 24), 11, 1, 0, 0, 2), (120_000, 10, 1, 2, (24, 16), 4, 3, 1, 3, 2),
    (120_000, 10, 1, 2, (24, 16), 4, 2, 0, 1, 1), (160_000, 12, 0, 0, (8, 16), 3, 2, 1, 2, 2),
    (60_000, 12, 1, 2, (24, 16), 11, 4, 1, 3, 2)])    # (round 5's rank-and-stage level 1 at 160 000 rows: the GPU tier)
def test_sort_wide_rec8_words(emu_ctx, n, bits, gap2, shift, rpt, b2max, wc, prefetch, l2w, wc_form):
    """8-byte {key bits, row id} words through the wide form: ties below the word, duplicates, the tie budget, fall-backs;
    level 1 tile at a time and write-combined — round 6's append kernel (wc_form 2) and round 5's rank-and-stage kernel
    (2 to 512 bins, sampled and exact rooms, chunks of 4 / 2 / 1 lines, counted and fixed level-2 buckets)."""
    P.check_sort_wide_rec8(emu_ctx, emu_ctx._lib.get_lib(), rng_for("wide-rec8", bits, gap2), n, bits=bits, gap2=gap2, shift=shift,
                           rpt=rpt, b2max=b2max, wc=wc, prefetch=prefetch, l2w=l2w, wc_form=wc_form, wc_min_rows=1 << 13)


# same name as the device tier's, another case: every plan forced at emulator sizes, plus the shards that are declined
@pytest.mark.parametrize("wide,bits,parts", [(0, 0, 2), (0, 1, 3), (0, 5, 8), (0, 9, 4), (2, 4, 8), (2, 8, 5), (2, 6, 64)])
def test_groupby_consume_partials(emu_ctx, wide, bits, parts):
    """The sharded group-by's local pass without the local table (arx_groupby_sum_i64_consume_partials), on every plan of
    the partitioned consume: the unpartitioned aggregate, one- and two-level plans, the wide form with rooms and counted;
    several work units per partition (a key in several records), more groups than the LDS tables hold (rows that leave as
    records of their own), regions too small (ARX_CAPACITY_ERROR); shards with nulls or too small are declined."""
    lib = emu_ctx._lib.get_lib()
    opts = {b"groupby_partition_min_rows": 0, b"groupby_wide": wide or 1, b"groupby_partition_bits": bits,
            b"groupby_agg_chunk_rows": 1 << 12, b"groupby_wide_agg_chunk_rows": 1 << 14, b"groupby_wide_room_min_mean": 16}
    with U.options(lib, opts):
        rng = rng_for("gbemit", wide, bits, parts)
        n = 40000
        k = U.random_array(rng, np.int32, n, lo=-2**31, hi=2**31 - 1)
        k.values[: n // 2] = k.values[: n // 2] % 1777          # many repeats + a distinct tail
        v = U.random_array(rng, np.int64, n, offset=1)
        records = P.check_groupby_consume_partials(emu_ctx, k, v, parts)
        assert records >= 1777 + n // 2 - 64
        k2 = U.random_array(rng, np.int32, n + 4097, lo=0, hi=50000, offset=5)
        v2 = U.random_array(rng, np.int64, n + 4097)
        P.check_groupby_consume_partials(emu_ctx, k2, v2, parts)
        # declined: nulls, and a shard below the partitioned consume's row threshold
        kn = U.random_array(rng, np.int32, n, null_p=0.01, lo=0, hi=100)
        from arrow_amd import parallel
        assert parallel.consume_partials_regions(kn.to_device(emu_ctx), v.to_device(emu_ctx), 1 << 12, parts) is None
        # (a forced value the case needs, a threshold above the rows of this shard, not a restore: options() above puts the knob back)
        assert lib.arx_set_option(b"groupby_partition_min_rows", 1 << 17) == 0
        assert parallel.consume_partials(k.to_device(emu_ctx), v.to_device(emu_ctx), 1 << 12, parts) == (None, None)
        # more records than the regions hold (every row its own group and a capacity that promises few groups: the rows that
        # find no place in an LDS table leave as records of their own): declined, the caller goes through the table
        assert lib.arx_set_option(b"groupby_partition_min_rows", 0) == 0
        big = 400_000 if bits == 0 else 0
        if big:
            kd = U.random_array(rng, np.int32, big, lo=-2**31, hi=2**31 - 1)
            vd = U.random_array(rng, np.int64, big)
            assert parallel.consume_partials(kd.to_device(emu_ctx), vd.to_device(emu_ctx), 1 << 12, parts) == (None, None)
            P.check_groupby_sum(emu_ctx, kd, vd, capacity=1 << 20, use_pyarrow=False)       # (the table path still serves it)
        k16 = U.random_array(rng, np.int16, n, lo=0, hi=100)      # other key types: through the table (its casts)
        assert lib.arx_set_option(b"groupby_partition_min_rows", 0) == 0
        assert parallel.consume_partials_regions(k16.to_device(emu_ctx), v.to_device(emu_ctx), 1 << 12, parts) is None


# the device tier's test_binary_take_edges draws its indices first and adds 2000-byte values: another input, one test there
def test_binary_take_empty_values_and_all_null(emu_ctx):
    rng = rng_for("btakeedge")
    v = U.random_binary(rng, 64, null_p=1.0)
    i = U.random_array(rng, np.int32, 200, lo=0, hi=63)
    out = P.check_binary_take(emu_ctx, v, i)
    assert out.null_count == 200
    v = U.random_binary(rng, 64, empty_p=1.0)      # only empty strings: zero data bytes
    P.check_binary_take(emu_ctx, v, i)


def test_binary_take_out_of_bounds(emu_ctx):
    # (part of test_binary_take_edges on the device tier)
    rng = rng_for("btakeoob")
    v = U.random_binary(rng, 10)
    idx = U.HostArray(np.array([0, 3, 10, 2], dtype=np.int32), None, 0, 4)
    with pytest.raises(emu_ctx.ArrowIndexError, match="Index 10 out of bounds"):
        emu_ctx.compute.take(v.to_device(emu_ctx), idx.to_device(emu_ctx))


# emulator-only knob grid: the segment fan-out at 2048-row segments (the device tier has its own grid at 5M rows)
@pytest.mark.parametrize("small_bucket,final_rows_log2,seg_min_bits,v2", [(0, 4, 1, 1), (1, 2, 1, 1), (1, 3, 5, 0), (0, 1, 1, 0)])
def test_sort_msd_bucket_variants_and_segment_fanout(emu_ctx, small_bucket, final_rows_log2, seg_min_bits, v2):
    """Tuning knobs of the MSD sort never change results: the 1024- vs 512-thread bucket kernel, the
    sub-bucket size and the fan-out of the segment level (segmented form forced on)."""
    lib = emu_ctx._lib.get_lib()
    opts = {b"sort_msd": 1, b"sort_msd_small_bucket": small_bucket, b"sort_msd_final_rows_log2": final_rows_log2,
            b"sort_msd_seg_min_bits": seg_min_bits, b"sort_msd_segment_rows": 2048 if seg_min_bits > 1 else 1 << 27,
            b"sort_msd_bucket_v2": v2, b"sort_msd_wide": v2}
    with U.options(lib, opts):
        rng = rng_for("msdknobs", small_bucket, final_rows_log2, seg_min_bits, v2)
        n = 6000   # (the emulator runs a 1024-thread workgroup as 1024 fibers)
        a = U.random_array(rng, np.uint64, n, null_p=0.02, offset=1)
        a.values[a.offset:a.offset + n - 1:7] = a.values[a.offset + 1:a.offset + n:7]  # ties
        P.check_sort_indices(emu_ctx, a, "descending", "at_start", use_pyarrow=False)


# the device tier runs the two as one test on one input (test_groupby_min_max_next_to_sum_and_merge): two inputs here
def test_groupby_min_max_next_to_sum(emu_ctx):
    rng = rng_for("gbminmaxsum")
    k = U.random_array(rng, np.int32, 3000, null_p=0.02, lo=0, hi=500)
    v = U.random_array(rng, np.int64, 3000, null_p=0.1, lo=-1000, hi=1000)
    P.check_groupby_min_max(emu_ctx, k, v, True, batches=2, with_sum=True)


def test_groupby_min_max_merge_of_two_states(emu_ctx):
    """Two states over halves of the rows, merged (Merge, hash_aggregate.cc:371-399) == one state."""
    rng = rng_for("gbminmaxmerge")
    k = U.random_array(rng, np.int32, 3000, null_p=0.03, lo=-60, hi=60)
    v = U.random_array(rng, np.int64, 3000, null_p=0.15)
    check_min_max_merge_of_two_states(emu_ctx, k, v, 1700, 1024)


# the device tier's test_grouper_hot_keys_and_overflow is this at 4M rows in one batch plus an overflow of its own
def test_grouper_hot_keys_take_the_pending_path(emu_ctx):
    """9 distinct rows over 30000: while a row's slot is claimed but not yet published (the emulator's __threadfence is
    a scheduling point) the other rows of the workgroup with that key must defer, not wait and not insert twice."""
    P.check_grouper(emu_ctx, rng_for("grouper-hot"), (np.int64, np.int64), 30000, 3, 0.0, 2, max_groups=16)


# host-side refusals, checked once: on this tier
def test_grouper_declines_and_overflows(emu_ctx):
    from arrow_amd.array import int64, bool_

    with pytest.raises(NotImplementedError, match="1 to 32 key columns"):
        emu_ctx.compute.Grouper([int64] * 33, 16)
    with pytest.raises(NotImplementedError, match="keys of type bool"):
        emu_ctx.compute.Grouper([bool_], 16)
    g = emu_ctx.compute.Grouper([int64], 4)
    g.consume([emu_ctx.Array.from_numpy(np.arange(4, dtype=np.int64))])
    assert g.num_groups == 4
    with pytest.raises(ValueError, match="more than 4 distinct key rows"):
        g.consume([emu_ctx.Array.from_numpy(np.arange(10, dtype=np.int64))])


# on the device these run in test_gpu_group_keys.py
@pytest.mark.parametrize("n,null_p,offset,max_len,card", [(0, 0.0, 0, 8, 1), (3000, 0.1, 0, 30, 40), (2500, 0.0, 5, 11, 2000),
                                                         (2000, 0.3, 3, 50, 7), (1000, 1.0, 0, 5, 5), (1500, 0.1, 2, 700, 300)])
def test_binary_key_columns_and_first_rows(emu_ctx, n, null_p, offset, max_len, card):
    P.check_binary_key_columns(emu_ctx, U.random_binary_pool(rng_for("bkey", n, max_len), n, card, null_p, offset, max_len),
                               rng_for("bkey2", n))


# on the device this runs in test_gpu_group_keys.py
def test_grouper_chain_levels_and_partial_lookups(emu_ctx):
    P.check_grouper_chain(emu_ctx)
