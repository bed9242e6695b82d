"""Parity tests proper: the HIP kernels on a real MI355X through arrow_amd.compute -> C ABI,
against the C oracle (bit-exact) and the reference's own build (pyarrow) on the same seeded
inputs.  Run with `pytest -m gpu` on the GPU box.

The cases both tiers run are written once, in parity_tiers.define: this file runs them at the device's sizes and adds,
below them, the cases only this tier has."""
import numpy as np
import pytest

from oracle import oracle as O

from . import parity_cases as P
from . import util as U
from .parity_tiers import GPU, check_min_max_merge_of_two_states, define, rng_for

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx(gpu_ctx):
    return gpu_ctx


globals().update(define(GPU))


# ------------------------------------------------------------------ this tier only
def test_filter_10m_rows_config1(gpu_ctx):
    """BASELINE config 1 shape: 10M-row int64, 50 % selectivity.  (Too large for the emulator, which asserts the same on
    5000 rows: test_filter_no_nulls_has_no_validity.)"""
    rng = rng_for("cfg1")
    n = 10_000_000
    v = U.random_array(rng, np.int64, n)
    m = U.random_mask(rng, n, 0.5)
    out = P.check_filter(gpu_ctx, v, m, "drop")
    assert out.validity is None and out.null_count == 0


# too large for the emulator
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


# too large for the emulator: the offenders sit in blocks far apart
def test_take_out_of_bounds_first_offender_large(gpu_ctx):
    rng = rng_for("oob")
    idx = rng.integers(0, 1000, size=2_000_000).astype(np.int32)
    idx[1_234_567] = 1000
    idx[1_900_000] = -7
    v = U.HostArray(np.arange(1000, dtype=np.int64), None, 0, 1000)
    P.check_take_out_of_bounds(gpu_ctx, v, U.HostArray(idx, None, 0, len(idx)))


# too large for the emulator (2^20 rows)
def test_cast_f64_f32_ties_to_even_exhaustive_mantissa_tail(gpu_ctx):
    """Every 29-bit tail pattern class around a float32 rounding boundary: RNE ties."""
    base = np.float64(1.0).view(np.uint64) if False else np.array([1.0]).view(np.uint64)[0]
    tails = np.arange(0, 1 << 20, dtype=np.uint64) << np.uint64(9)
    bits = (base + tails).astype(np.uint64)
    x = bits.view(np.float64)
    P.check_cast_f64_f32(gpu_ctx, U.HostArray(x.copy(), None, 0, len(x)))


# too large for the emulator
def test_sort_multi_chunk(gpu_ctx):
    """> 2048 tiles so that a chunk holds several tiles (cursor carry between tiles)."""
    rng = rng_for("sort3")
    n = 4096 * 2048 * 2 + 12345
    a = U.random_array(rng, np.uint64, n, null_p=0.01)
    P.check_sort_indices(gpu_ctx, a, "ascending", "at_end", use_pyarrow=False)


# a contract of the table in HBM (16 slots, 100 keys), checked once: on this tier
def test_groupby_table_overflow_is_reported(gpu_ctx):
    amd = gpu_ctx
    k = amd.Array.from_numpy(np.arange(100, dtype=np.int32))
    v = amd.Array.from_numpy(np.ones(100, dtype=np.int64))
    op = amd.compute.GroupBySum(16, k.device)
    op.consume(k, v)
    with pytest.raises(amd.ArrowInvalid, match="full"):
        op.num_groups()


# ------------------------------------------------------------------ size-independent properties
# needs `torch` on `cuda` (inputs made on the device), and 2^28 rows
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


# the sharded sort's host side (arrow_amd.parallel) needs `torch` on `cuda`
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


# same name as the emulator tier's, another case: the planner's own choices at 3M rows (the emulator forces every plan)
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


# needs `torch` on `cuda`: the exchange between the virtual ranks is done on device tensors
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


# same name as the emulator tier's, another case: sizes from 2M to 4M rows and counters (the emulator runs a knob grid)
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


# needs `torch` on `cuda`: the exchange between the virtual ranks is done on device tensors
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


# device-only knob grid at 5M rows (the emulator tier has its own: test_sort_msd_bucket_variants_and_segment_fanout)
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


# needs `torch` on `cuda`: the exchange between the virtual ranks is done on device tensors
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


# the emulator tier draws other inputs for these edges and splits them in two (test_binary_take_empty_values_and_all_null,
# test_binary_take_out_of_bounds); the 2000-byte values are this tier's
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


# too large for the emulator (2^22 indices, 4 GiB of output asked for)
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


# one input for both halves (the emulator tier draws one each: test_groupby_min_max_next_to_sum, ..._merge_of_two_states)
def test_groupby_min_max_next_to_sum_and_merge(gpu_ctx):
    rng = rng_for("gbminmaxsum")
    k = U.random_array(rng, np.int32, 300_000, null_p=0.02, lo=0, hi=5000)
    v = U.random_array(rng, np.int64, 300_000, null_p=0.1, lo=-10**9, hi=10**9)
    P.check_groupby_min_max(gpu_ctx, k, v, True, batches=2, with_sum=True)
    check_min_max_merge_of_two_states(gpu_ctx, k, v, 170_000, 1 << 14)


# 4M rows in one batch and an overflow of 100 000 keys (the emulator tier: test_grouper_hot_keys_take_the_pending_path)
def test_grouper_hot_keys_and_overflow(gpu_ctx):
    """Every row hits one of 3 keys while they are being inserted (the pending-list path), and a table that is too
    small fails the call instead of corrupting ids."""
    P.check_grouper(gpu_ctx, rng_for("grouper-hot"), (np.int64, np.int64), 4_000_000, 3, 0.0, 1, max_groups=16)
    from arrow_amd.array import int64

    g = gpu_ctx.compute.Grouper([int64], 1000)
    with pytest.raises(ValueError, match="more than 1000 distinct key rows"):
        g.consume([gpu_ctx.Array.from_numpy(np.arange(100_000, dtype=np.int64))])


# same name as the emulator tier's, another case: sizes alone (the LSD fallback, > 4M and > 2^27 records), no knob sets
@pytest.mark.parametrize("n", [100_003, 6_000_011, 150_000_001])
def test_sort_records(gpu_ctx, n):
    """Round 6: arx_sort_records on gfx950 — the LSD fallback, the MSD hybrid (> 4M records) and the wide form (> 2^27)."""
    P.check_sort_records(gpu_ctx, rng_for("sort-records", n), n)
