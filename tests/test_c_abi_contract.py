"""The C ABI's argument contract (include/arrow_amd.h), exercised directly through ctypes on the
kernel sources built for the host (tests/emu): every entry point rejects NULL buffers, negative or
mismatched lengths, unsupported widths / types and short or misaligned workspaces with a status
code that mirrors arrow::StatusCode and a message in arx_last_error() — never a crash — and
zero-length inputs are accepted everywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.emu

OK, INVALID, INDEX_ERROR, NOT_IMPLEMENTED = 0, -4, -7, -10


def _span(L, data=None, validity=None, offset=0, length=0, null_count=0):
    return L.ArxSpan(None if validity is None else validity.data_ptr(), None if data is None else data.data_ptr(),
                     offset, length, null_count)


def _buf(nbytes):
    return torch.zeros(max(nbytes, 64), dtype=torch.uint8)


def _err(lib):
    lib.arx_last_error.restype = C.c_char_p
    return lib.arx_last_error().decode()


def test_filter_and_take_argument_checks(emu_ctx):
    L = emu_ctx._lib
    lib = L.get_lib()
    n = 1000
    vals, mask, ws, out = _buf(n * 8), _buf(n // 8 + 8), _buf(lib.arx_filter_workspace_bytes(n) + 64), _buf(n * 8)
    m = _span(L, mask, length=n)
    v = _span(L, vals, length=n)
    cnt = C.c_int64(0)
    assert lib.arx_filter_count(C.byref(m), 0, ws.data_ptr(), 8, C.byref(cnt), None) == INVALID      # workspace too small
    assert "workspace" in _err(lib)
    assert lib.arx_filter_count(None, 0, ws.data_ptr(), ws.numel(), C.byref(cnt), None) == INVALID
    assert lib.arx_filter_count(C.byref(m), 7, ws.data_ptr(), ws.numel(), C.byref(cnt), None) == INVALID  # bad null selection
    assert lib.arx_filter_count(C.byref(m), 0, ws.data_ptr(), ws.numel(), C.byref(cnt), None) == OK and cnt.value == 0
    assert lib.arx_filter_exec(C.byref(v), 3, C.byref(m), 0, ws.data_ptr(), 0, out.data_ptr(), None, None) in (INVALID, NOT_IMPLEMENTED)  # width 3
    short = _span(L, vals, length=n - 1)
    assert lib.arx_filter_exec(C.byref(short), 8, C.byref(m), 0, ws.data_ptr(), 0, out.data_ptr(), None, None) == INVALID
    assert "same length" in _err(lib)
    idx = _buf(40)
    i = _span(L, idx, length=10)
    assert lib.arx_take(C.byref(v), 8, C.byref(i), 99, out.data_ptr(), None, None, None) == NOT_IMPLEMENTED  # index type
    assert lib.arx_take(C.byref(v), 5, C.byref(i), 5, out.data_ptr(), None, None, None) == NOT_IMPLEMENTED   # byte width
    assert lib.arx_take(C.byref(v), 8, C.byref(i), 5, None, None, None, None) == INVALID
    tws = _buf(lib.arx_take_workspace_bytes() + 64)
    idx.view(torch.int32)[3] = 5000
    assert lib.arx_check_index_bounds(C.byref(i), 5, 1000, tws.data_ptr(), tws.numel(), None) == INDEX_ERROR
    assert _err(lib) == "Index 5000 out of bounds"
    idx.view(torch.int32)[3] = -1
    assert lib.arx_check_index_bounds(C.byref(i), 5, 1000, tws.data_ptr(), tws.numel(), None) == INDEX_ERROR
    assert _err(lib) == "Index -1 out of bounds"
    empty = _span(L, idx, length=0)
    assert lib.arx_take(C.byref(v), 8, C.byref(empty), 5, out.data_ptr(), None, None, None) == OK


def test_sort_and_groupby_argument_checks(emu_ctx):
    L = emu_ctx._lib
    lib = L.get_lib()
    n = 500
    keys, out = _buf(n * 8), _buf(n * 8)
    need = lib.arx_sort_indices_workspace_bytes(n)
    ws = _buf(need + 512)
    base = (ws.data_ptr() + 255) & ~255
    v = _span(L, keys, length=n)
    assert lib.arx_sort_indices(C.byref(v), 0, 0, 1, base, 16, out.data_ptr(), None) == INVALID          # short workspace
    assert "workspace" in _err(lib)
    assert lib.arx_sort_indices(C.byref(v), 0, 0, 1, base + 8, need, out.data_ptr(), None) == INVALID     # misaligned
    assert lib.arx_sort_indices(C.byref(v), 42, 0, 1, base, need, out.data_ptr(), None) == NOT_IMPLEMENTED  # key type
    assert lib.arx_sort_indices(C.byref(v), 0, 9, 1, base, need, out.data_ptr(), None) == INVALID          # order
    assert lib.arx_sort_indices(C.byref(v), 0, 0, 9, base, need, out.data_ptr(), None) == INVALID          # null placement
    assert lib.arx_sort_indices(C.byref(v), 0, 0, 1, base, need, None, None) == INVALID
    assert lib.arx_sort_indices(C.byref(_span(L, keys, length=0)), 0, 0, 1, base, need, out.data_ptr(), None) == OK
    cap = 64
    state = _buf(lib.arx_groupby_state_bytes(cap))
    assert lib.arx_groupby_init(state.data_ptr(), 48, None) == INVALID                                     # not a power of two
    assert lib.arx_groupby_init(None, cap, None) == INVALID
    assert lib.arx_groupby_init(state.data_ptr(), cap, None) == OK
    k32, v64 = _buf(n * 4), _buf(n * 8)
    ks, vs = _span(L, k32, length=n), _span(L, v64, length=n - 3)
    assert lib.arx_groupby_sum_i64_consume(state.data_ptr(), cap, C.byref(ks), C.byref(vs), None, 0, None) == INVALID
    assert "same length" in _err(lib)
    # more distinct keys than slots: reported, not silently dropped
    k32.view(torch.int32)[:n] = torch.arange(n, dtype=torch.int32)
    vs = _span(L, v64, length=n)
    rc = lib.arx_groupby_sum_i64_consume(state.data_ptr(), cap, C.byref(ks), C.byref(vs), None, 0, None)
    g = C.c_int64(0)
    assert rc == INVALID or lib.arx_groupby_num_groups(state.data_ptr(), C.byref(g), None) == INVALID
    assert "capacity" in _err(lib) or "full" in _err(lib)
    mm = _buf(lib.arx_groupby_minmax_bytes(cap))
    assert lib.arx_groupby_minmax_i64_consume(state.data_ptr(), None, cap, C.byref(ks), C.byref(vs), None) == INVALID
    assert lib.arx_groupby_export(state.data_ptr(), None, k32.data_ptr(), k32.data_ptr(), v64.data_ptr(), v64.data_ptr(),
                                  k32.data_ptr(), v64.data_ptr(), v64.data_ptr(), None) == INVALID   # extrema wanted, no minmax buffer
    del mm
    # grouped float sums (row order) and rows / list elements of any width
    gids, sums, cnts, seen = _buf(n * 4), _buf(64 * 8), _buf(64 * 8), _buf(64 * 4)
    fv = _span(L, v64, length=n)
    fneed = lib.arx_hash_sum_float_workspace_bytes(n)
    fws = _buf(fneed + 512)
    args = (gids.data_ptr(), n, fws.data_ptr(), fneed + 512, sums.data_ptr(), cnts.data_ptr(), seen.data_ptr(), None)
    assert lib.arx_hash_sum_float_consume(C.byref(fv), 6, 0, 0.0, *args) == INVALID                       # int64 is not a float type
    assert lib.arx_hash_sum_float_consume(C.byref(fv), 9, 0, 0.0, gids.data_ptr(), n, fws.data_ptr(), 64, sums.data_ptr(), cnts.data_ptr(),
                                          seen.data_ptr(), None) == INVALID                             # short workspace
    assert "workspace" in _err(lib)
    assert lib.arx_hash_sum_float_consume(C.byref(fv), 9, 0, 0.0, None, n, fws.data_ptr(), fneed + 512, sums.data_ptr(), cnts.data_ptr(),
                                          seen.data_ptr(), None) == INVALID
    assert lib.arx_hash_sum_float_consume(C.byref(fv), 9, 0, 0.0, gids.data_ptr(), 0, None, 0, None, None, None, None) == OK
    assert lib.arx_hash_sum_float_consume(C.byref(fv), 9, 0, 0.0, *args) == OK                             # all rows in group 0
    assert lib.arx_hash_sum_float_workspace_bytes(0) == 0
    assert lib.arx_hash_sum_f64_merge(sums.data_ptr(), cnts.data_ptr(), seen.data_ptr(), None, cnts.data_ptr(), seen.data_ptr(),
                                      gids.data_ptr(), 4, None) == INVALID
    assert lib.arx_hash_sum_f64_merge(None, None, None, None, None, None, None, 0, None) == OK
    assert lib.arx_hash_mean_f64_finalize(sums.data_ptr(), None, 4, sums.data_ptr(), None) == INVALID
    assert lib.arx_hash_mean_f64_finalize(None, None, 0, None, None) == OK


def test_scalar_kernel_argument_checks(emu_ctx):
    L = emu_ctx._lib
    lib = L.get_lib()
    a, b, out = _buf(800), _buf(800), _buf(800)
    I64, F64, F32, I32 = 6, 9, 8, 4                                                                      # ARX_NUM_*
    zf, zi = C.c_double(0.0), C.c_int64(0)
    zfp, zip_ = C.addressof(zf), C.addressof(zi)
    assert lib.arx_compare_numeric(2, F64, None, zfp, None, zfp, 100, out.data_ptr(), None) == INVALID  # scalar x scalar
    assert lib.arx_compare_numeric(77, I64, a.data_ptr(), zip_, b.data_ptr(), zip_, 100, out.data_ptr(), None) == INVALID   # unknown op
    assert lib.arx_compare_numeric(2, I64, a.data_ptr(), zip_, b.data_ptr(), zip_, 0, None, None) == OK
    assert lib.arx_arith_numeric(9, 0, I64, a.data_ptr(), zip_, None, 0, b.data_ptr(), zip_, None, 0, 100, out.data_ptr(), None,
                                 None) == INVALID                                                       # unknown op
    assert lib.arx_arith_numeric(0, 1, I64, a.data_ptr(), zip_, None, 0, b.data_ptr(), zip_, None, 0, 100, out.data_ptr(), None,
                                 None) == INVALID                                                       # checked int64, no flag
    nodata = L.ArxSpan(None, None, 0, 10, 0)
    assert lib.arx_cast_numeric(C.byref(nodata), F64, F32, 0, 0, None, 0, out.data_ptr(), None) == INVALID   # NULL input
    sp = _span(L, a, length=100)
    assert lib.arx_cast_numeric(C.byref(sp), I64, I32, 0, 0, None, 0, out.data_ptr(), None) == INVALID   # checked cast needs a workspace
    assert lib.arx_cast_numeric(C.byref(sp), I64, I32, 1, 0, None, 0, out.data_ptr(), None) == OK        # unchecked does not
    lm, rm = _span(L, a, length=100), _span(L, b, length=90)
    assert lib.arx_boolean_kleene(0, C.byref(lm), C.byref(rm), out.data_ptr(), None, None) == INVALID   # length mismatch
    rm = _span(L, b, validity=a, length=100, null_count=-1)
    assert lib.arx_boolean_kleene(0, C.byref(lm), C.byref(rm), out.data_ptr(), None, None) == INVALID   # nulls but no out validity
    assert lib.arx_boolean_kleene(5, C.byref(lm), C.byref(lm), out.data_ptr(), None, None) == INVALID
    assert lib.arx_set_option(b"no_such_option", 1) != 0
    bs = L.ArxBinarySpan(None, None, None, 0, 10, 0)
    i = _span(L, a, length=5)
    tot = C.c_int64(0)
    assert lib.arx_binary_take_offsets(C.byref(bs), C.byref(i), 5, None, 0, out.data_ptr(), None, None, C.byref(tot), None) == INVALID


def test_concatenate_and_delta_argument_checks(emu_ctx):
    L = emu_ctx._lib
    lib = L.get_lib()
    src, dst = _buf(64), _buf(64)
    assert lib.arx_bitmap_copy_at(src.data_ptr(), -1, 10, dst.data_ptr(), 0, None) == INVALID
    assert lib.arx_bitmap_copy_at(src.data_ptr(), 0, 10, None, 0, None) == INVALID
    assert lib.arx_bitmap_copy_at(src.data_ptr(), 0, 10, dst.data_ptr(), -3, None) == INVALID
    assert lib.arx_bitmap_copy_at(None, 0, 0, None, 0, None) == OK                                    # nothing to append
    assert lib.arx_bitmap_copy_at(None, 0, 70, dst.data_ptr(), 3, None) == OK                           # NULL source = all ones
    bits = np.unpackbits(dst.numpy()[:16], bitorder="little")
    assert bits[:3].sum() == 0 and bits[3:73].all() and bits[73:].sum() == 0
    assert lib.arx_binary_rebase_offsets(None, 4, 0, dst.data_ptr(), None) == INVALID
    assert lib.arx_binary_rebase_offsets(src.data_ptr(), -1, 0, dst.data_ptr(), None) == INVALID
    # DELTA_BINARY_PACKED: corrupt headers are refused by the host walk, never read past the page
    nmb, vpm, total, first, used = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_size_t(0)
    def scan(page):
        buf = np.frombuffer(page, dtype=np.uint8)
        return lib.arx_delta_scan_miniblocks(buf.ctypes.data, len(buf), 0, None, 0, C.byref(nmb), C.byref(vpm), C.byref(total),
                                             C.byref(first), C.byref(used))
    from oracle import oracle as O
    good = O.delta_binary_packed_encode(np.arange(1000) * 3)
    assert scan(good) == OK and (total.value, first.value, used.value) == (1000, 0, len(good))
    assert scan(good[: len(good) - 5]) == INVALID and "past the page" in _err(lib)                     # truncated miniblock
    assert scan(good[:2]) == INVALID                                                                  # truncated header
    assert scan(b"\x07\x04\x05\x00") == INVALID and "header" in _err(lib)                             # block size 7
    assert scan(b"\x80\x01\x00\x05\x00") == INVALID                                                   # zero miniblocks
    assert scan(b"\x80\x01\x04\x01\x02") == OK and (nmb.value, total.value, first.value) == (0, 1, 1)   # one value: no blocks
    assert lib.arx_delta_scan_miniblocks(None, 0, 0, None, 0, C.byref(nmb), C.byref(vpm), C.byref(total), C.byref(first), None) == INVALID
    out, ws = _buf(8000), _buf(lib.arx_delta_decode_workspace_bytes(1000) + 64)
    page = _buf(len(good) + 64)
    mbs = _buf(24 * 40)
    assert lib.arx_delta_decode(page.data_ptr(), mbs.data_ptr(), 32, 32, 0, 1000, 3, ws.data_ptr(), ws.numel(), out.data_ptr(), None) == INVALID  # width 3
    assert lib.arx_delta_decode(page.data_ptr() + 1, mbs.data_ptr(), 32, 32, 0, 1000, 8, ws.data_ptr(), ws.numel(), out.data_ptr(), None) == INVALID  # misaligned page
    assert lib.arx_delta_decode(page.data_ptr(), mbs.data_ptr(), 3, 32, 0, 1000, 8, ws.data_ptr(), ws.numel(), out.data_ptr(), None) == INVALID  # too few miniblocks
    assert lib.arx_delta_decode(page.data_ptr(), mbs.data_ptr(), 32, 32, 0, 1000, 8, ws.data_ptr(), 8, out.data_ptr(), None) == INVALID      # short workspace
    assert lib.arx_delta_decode(None, None, 0, 0, 0, 0, 8, None, 0, None, None) == OK                  # nothing to decode
    assert lib.arx_delta_decode(None, None, 0, 0, 42, 1, 8, ws.data_ptr(), ws.numel(), out.data_ptr(), None) == OK   # a single value: the header's
    assert out.view(torch.int64)[0].item() == 42
    # BYTE_STREAM_SPLIT
    assert lib.arx_byte_stream_split_decode(page.data_ptr(), 10, 3, out.data_ptr(), None) == NOT_IMPLEMENTED       # width 3
    assert lib.arx_byte_stream_split_decode(page.data_ptr(), -1, 4, out.data_ptr(), None) == INVALID
    assert lib.arx_byte_stream_split_decode(page.data_ptr(), 10, 8, out.data_ptr() + 4, None) == INVALID             # misaligned output
    assert lib.arx_byte_stream_split_decode(None, 10, 8, out.data_ptr(), None) == INVALID
    assert lib.arx_byte_stream_split_decode(None, 0, 8, None, None) == OK
    page[:16] = torch.arange(16, dtype=torch.uint8)
    assert lib.arx_byte_stream_split_decode(page.data_ptr(), 4, 4, out.data_ptr(), None) == OK
    assert out[:16].tolist() == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
    # DELTA_LENGTH_BYTE_ARRAY: lengths -> offsets
    lens = torch.tensor([3, 0, 5, 1], dtype=torch.int32)
    offs = torch.zeros(16, dtype=torch.int32)
    assert lib.arx_lengths_to_offsets_i32(lens.data_ptr(), 4, 10, offs.data_ptr(), ws.data_ptr(), ws.numel(), None) == OK
    assert offs[:5].tolist() == [10, 13, 13, 18, 19]
    assert lib.arx_lengths_to_offsets_i32(None, 0, 7, offs.data_ptr(), ws.data_ptr(), ws.numel(), None) == OK and offs[0].item() == 7
    assert lib.arx_lengths_to_offsets_i32(None, 4, 0, offs.data_ptr(), ws.data_ptr(), ws.numel(), None) == INVALID
    assert lib.arx_lengths_to_offsets_i32(lens.data_ptr(), 4, 0, None, ws.data_ptr(), ws.numel(), None) == INVALID
    assert lib.arx_lengths_to_offsets_i32(lens.data_ptr(), 4, 0, offs.data_ptr(), ws.data_ptr(), 0, None) == INVALID
    assert lib.arx_lengths_to_offsets_i32(lens.data_ptr(), -1, 0, offs.data_ptr(), ws.data_ptr(), ws.numel(), None) == INVALID
    # DELTA_BYTE_ARRAY: ["apple", "apply", "", "b"] then a second page ["x", "xy"]
    prefix = torch.tensor([0, 4, 0, 0, 0, 1], dtype=torch.int32)
    slen = torch.tensor([5, 1, 0, 1, 1, 1], dtype=torch.int32)
    suffix = torch.tensor(list(b"appleybxy") + [0] * 7, dtype=torch.uint8)
    first = torch.tensor([0, 4, 6], dtype=torch.int64)
    sfirst = torch.tensor([0, 7, 9], dtype=torch.int64)
    vlen = torch.zeros(6, dtype=torch.int32)
    state = torch.zeros(2, dtype=torch.int64)
    soff, ooff = torch.zeros(7, dtype=torch.int32), torch.zeros(7, dtype=torch.int32)
    assert lib.arx_delta_byte_array_lengths(prefix.data_ptr(), slen.data_ptr(), 6, first.data_ptr(), 2, vlen.data_ptr(), state.data_ptr(), None) == OK
    assert vlen.tolist() == [5, 5, 0, 1, 1, 2] and state.tolist() == [0, 14]
    assert lib.arx_lengths_to_offsets_i32(slen.data_ptr(), 6, 0, soff.data_ptr(), ws.data_ptr(), ws.numel(), None) == OK
    assert lib.arx_lengths_to_offsets_i32(vlen.data_ptr(), 6, 100, ooff.data_ptr(), ws.data_ptr(), ws.numel(), None) == OK
    data = torch.zeros(16, dtype=torch.uint8)
    assert lib.arx_delta_byte_array_expand(prefix.data_ptr(), soff.data_ptr(), suffix.data_ptr(), 9, ooff.data_ptr(), 100, first.data_ptr(),
                                           sfirst.data_ptr(), 2, data.data_ptr(), state.data_ptr(), None) == OK
    assert bytes(data[:14].tolist()) == b"appleapplybxxy" and state[0].item() == 0
    sfirst[1] = 6                                              # the first page's suffix lengths add up to 7, not 6: both pages are off
    assert lib.arx_delta_byte_array_expand(prefix.data_ptr(), soff.data_ptr(), suffix.data_ptr(), 9, ooff.data_ptr(), 100, first.data_ptr(),
                                           sfirst.data_ptr(), 2, data.data_ptr(), state.data_ptr(), None) == OK
    assert state[0].item() == 16
    prefix[4] = 1                                              # a page's first value has nothing before it
    assert lib.arx_delta_byte_array_lengths(prefix.data_ptr(), slen.data_ptr(), 6, first.data_ptr(), 2, vlen.data_ptr(), state.data_ptr(), None) == OK
    assert state[0].item() == 2
    prefix[4], prefix[1] = 0, -1
    assert lib.arx_delta_byte_array_lengths(prefix.data_ptr(), slen.data_ptr(), 6, first.data_ptr(), 2, vlen.data_ptr(), state.data_ptr(), None) == OK
    assert state[0].item() == 1
    assert lib.arx_delta_byte_array_lengths(None, None, 0, None, 0, None, state.data_ptr(), None) == OK and state.tolist() == [0, 0]
    assert lib.arx_delta_byte_array_lengths(prefix.data_ptr(), slen.data_ptr(), 6, first.data_ptr(), 2, vlen.data_ptr(), None, None) == INVALID
    assert lib.arx_delta_byte_array_lengths(prefix.data_ptr(), slen.data_ptr(), 6, None, 2, vlen.data_ptr(), state.data_ptr(), None) == INVALID
    assert lib.arx_delta_byte_array_expand(None, None, None, 0, None, 0, None, None, 0, None, None, None) == OK
    assert lib.arx_delta_byte_array_expand(prefix.data_ptr(), soff.data_ptr(), suffix.data_ptr() + 1, 8, ooff.data_ptr(), 100, first.data_ptr(),
                                           None, 2, data.data_ptr(), None, None) == INVALID                   # misaligned suffix bytes
    assert lib.arx_delta_byte_array_expand(prefix.data_ptr(), soff.data_ptr(), suffix.data_ptr(), 9, ooff.data_ptr(), 100, first.data_ptr(),
                                           sfirst.data_ptr(), 2, data.data_ptr(), None, None) == INVALID      # a check without a state word


# ---------------------------------------------------------------------------------------------------------------------
# The tuning knobs (arx_set_option / arx_get_option).  One row per knob: name, default, probes (value given, value
# stored).  The numbers are the contract: they were written down from the setters and the Knob initialisers as they
# stood before the knobs moved into tables, NOT read back from the library — a default or a range that changes in
# arrow_amd/csrc must be changed here by hand too.
I32_MAX = 2**31 - 1
GB_HARD_MAX_SLICE = (1 << 32) - (1 << 26)
BOOL = ((-1, 1), (0, 0), (1, 1), (2, 1))
TRI = ((-5, -1), (-1, -1), (0, 0), (1, 1), (7, 1))
RPT = ((-3, 8), (0, 8), (8, 8), (12, 8), (16, 16), (20, 16), (24, 24), (100, 24))
SLICE_ROWS = ((0, 4096), (4096, 4096), (5000, 4096), (98304 + 5, 98304), (1 << 30, 1 << 30), (GB_HARD_MAX_SLICE, GB_HARD_MAX_SLICE),
              (GB_HARD_MAX_SLICE + 1, GB_HARD_MAX_SLICE), (1 << 40, GB_HARD_MAX_SLICE))
ANY_INT = ((-7, -7), (-1, -1), (0, 0), (9, 9), (100, 100), (I32_MAX, I32_MAX), (2**32 + 5, 5))     # stored as given, truncated to int


def _pow2_probes(lo, hi):
    """The next power of two within 2^lo .. 2^hi: below the range, every power (each a snap point, stored as given), one
    value just above each power (stored as the next one, or as 2^hi), far above."""
    inside = tuple(p for k in range(lo, hi + 1) for p in ((1 << k, 1 << k), ((1 << k) + 1, 1 << min(k + 1, hi))))
    return ((-1, 1 << lo), (0, 1 << lo)) + inside + ((1 << 40, 1 << hi),)


KNOBS = (
    # sort.hip
    (b"sort_msd", -1, TRI),
    (b"sort_msd_min_rows", 1 << 22, ((0, 256), (256, 256), (1 << 22, 1 << 22), (I32_MAX, I32_MAX), (2**31, I32_MAX), (2**40, I32_MAX))),
    (b"sort_msd_sampled", 1, ((-1, 0), (0, 0), (1, 1), (2, 2), (3, 2))),
    (b"sort_msd_fused", 1, BOOL),
    (b"sort_msd_segment_rows", 1 << 27, ((0, 1024), (1023, 1024), (1024, 1024), (1 << 27, 1 << 27), (1 << 40, 1 << 40))),
    (b"sort_msd_final_rows_log2", 1, ((0, 1), (1, 1), (8, 8), (9, 8))),
    (b"sort_msd_small_bucket", 1, BOOL),
    (b"sort_msd_wide_sample_shift", 6, ((-1, 0), (0, 0), (6, 6), (8, 8), (9, 8))),
    (b"sort_xcd_map", 1, ((-1, 0), (0, 0), (1, 1), (7, 7), (8, 7))),
    (b"sort_msd_wide_bits", 0, ((-1, 0), (0, 0), (20, 20), (21, 20))),
    (b"sort_msd_wide_b2max", 11, ((-1, 0), (0, 0), (11, 11), (12, 12), (13, 12))),
    (b"sort_msd_wide_rpt1", 24, RPT),
    (b"sort_msd_wide_rpt2", 16, RPT),
    (b"sort_msd_tiny_bucket", 2, ((-1, 0), (0, 0), (2, 2), (3, 2))),
    (b"sort_msd_bucket_cpt", 4, ((-1, 4), (0, 4), (4, 4), (6, 4), (7, 4), (8, 8), (100, 8))),
    (b"sort_msd_prefix", 1, BOOL),
    (b"sort_msd_wide_gap2", 1, BOOL),
    (b"sort_msd_wide_rec8", 1, BOOL),
    (b"sort_msd_wide_rec8_tie_shift", 4, ((-1, 0), (0, 0), (4, 4), (40, 40), (41, 40))),
    (b"sort_msd_wide_wc", 256, ((-1, 0), (0, 0), (256, 256), (4096, 4096), (4097, 4096))),
    (b"sort_records_in_place", 1, BOOL),
    (b"sort_vary_sample_shift", 6, ((0, 1), (1, 1), (6, 6), (8, 8), (9, 8))),
    (b"sort_msd_wide_wc_typed", 1, ((-1, 1), (0, 0), (1, 1), (2, 2), (3, 1))),
    (b"sort_msd_wide_wc_form", 2, ((-1, 2), (0, 2), (1, 1), (2, 2), (3, 2))),
    (b"sort_msd_wide_wc_rows", 4, ((0, 4), (4, 4), (5, 4), (6, 6), (7, 4), (8, 8), (9, 4))),
    (b"sort_msd_wide_wc_min_rows", 1 << 17, ((0, 1), (1, 1), (1 << 17, 1 << 17), (1 << 30, 1 << 30), ((1 << 30) + 1, 1 << 30))),
    (b"sort_msd_wide_wc_prefetch", 1, BOOL),
    (b"sort_msd_wide_l2w", 3, ((-1, 0), (0, 0), (3, 3), (4, 3))),
    (b"sort_msd_wide_sample_strict", 0, BOOL),
    (b"sort_msd_wide", 1, BOOL),
    (b"sort_msd_bucket_v2", 1, BOOL),
    (b"sort_msd_seg_min_bits", 1, ((0, 1), (1, 1), (7, 7), (8, 7))),
    (b"sort_msd_global_bits", 14, ((1, 2), (2, 2), (14, 14), (15, 14))),
    (b"sort_fuse_prep", 1, BOOL),
    (b"sort_chunks", 2048, ((0, 1), (1, 1), (2048, 2048), (16384, 16384), (16385, 16384))),
    # selection.hip
    (b"filter_batch", 4, ((-1, 1), (0, 1), (1, 1), (3, 1), (4, 4), (9, 4))),
    (b"filter_pipe", 1, BOOL),
    (b"filter_sparse", -1, TRI),
    # parquet.hip
    (b"snappy_lds", -1, TRI),
    # groupby.hip
    (b"groupby_partition_min_rows", 1 << 17, ((-1, 0), (0, 0), (1 << 17, 1 << 17), (I32_MAX, I32_MAX), (2**31, I32_MAX))),
    (b"groupby_partition_bits", -1, ANY_INT),
    (b"groupby_agg_pipe", 1, BOOL),
    (b"groupby_xcd_map", 1, ((-1, 0), (0, 0), (1, 1), (7, 7), (8, 7))),
    (b"groupby_b1", -1, ANY_INT),
    (b"groupby_chunks", 2048, ((0, 1), (1, 1), (2048, 2048), (4096, 4096), (4097, 4096))),
    (b"groupby_wide_max_bits", 11, ((0, 1), (1, 1), (11, 11), (12, 11))),
    (b"groupby_wide_room_min_mean", 1 << 14, ((0, 1), (1, 1), (1 << 14, 1 << 14), (I32_MAX, I32_MAX), (2**31, I32_MAX))),
    (b"groupby_sketch", 1, BOOL),
    (b"groupby_stripe", 0, ((-4, 0), (0, 0), (1, 4), (3, 4), (4, 4), (7, 4), (68, 68), (70, 68), (1 << 20, 1 << 20), ((1 << 20) + 4, 1 << 20))),
    (b"groupby_wide_rooms", 1, BOOL),
    (b"groupby_wide", 1, ((-1, 0), (0, 0), (1, 1), (2, 2), (3, 2))),
    (b"groupby_wide_agg_chunk_rows", 1 << 21, _pow2_probes(14, 26) + ((3 << 20, 1 << 22),)),
    (b"groupby_probe_rows", 1 << 25, ((0, 4096), (4095, 4096), (4096, 4096), (1 << 25, 1 << 25), (1 << 40, 1 << 40))),
    (b"groupby_l1_global", 1, BOOL),
    (b"groupby_max_slice_rows", 1 << 30, SLICE_ROWS),
    (b"groupby_wide_max_slice_rows", GB_HARD_MAX_SLICE, SLICE_ROWS),
    (b"groupby_agg_chunk_rows", 1 << 18, _pow2_probes(12, 24) + ((3 << 17, 1 << 19),)),
    # groupby_lines.h
    (b"groupby_lines", 1, BOOL),
    (b"groupby_lines_min_rows", 1 << 22, ((-5, 1), (0, 1), (1, 1), (1 << 22, 1 << 22), (1 << 40, 1 << 40))),
    (b"groupby_lines_sample_rows", 1 << 24, ((0, 64), (63, 64), (64, 64), (1 << 24, 1 << 24), (1 << 40, 1 << 40))),
    (b"groupby_lines_range_sample_rows", 1 << 20, ((0, 64), (63, 64), (64, 64), (1 << 20, 1 << 20), (1 << 40, 1 << 40))),
    (b"groupby_lines_unit_rows", 1 << 21, ((0, 768), (767, 768), (768, 768), (1 << 21, 1 << 21), (1 << 30, 1 << 30), ((1 << 30) + 1, 1 << 30))),
    (b"groupby_lines_wgs", 0, ((-1, 0), (0, 0), (4096, 4096), (4097, 4096))),
)
COUNTERS = (b"groupby_slices_direct", b"groupby_slices_one_level", b"groupby_slices_two_level", b"groupby_slices_wide",
            b"groupby_slices_probe", b"groupby_slices_rooms", b"groupby_rooms_overflows", b"groupby_slices_lines",
            b"groupby_lines_fallbacks", b"groupby_lines_declined", b"groupby_lines_outlier_rows", b"sort_wide_runs",
            b"sort_wide_rec8_runs", b"sort_wide_rec8_ties", b"sort_wide_rec8_given_up", b"sort_wide_wc_runs",
            b"sort_wide_wc_given_up", b"set_lookup_lds_probes", b"set_lookup_global_probes")


def _check_knob_table(lib):
    import os
    import re

    from . import util as U

    names = [k[0] for k in KNOBS]
    assert len(names) == len(set(names)) == 63
    # every knob DESIGN.md 4.9 speaks of is in the table
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    sec = design[design.index("### 4.9 A/B knobs"):]
    sec = sec[:sec.index("\n### ", 4)]
    for word in re.findall(r"`((?:filter|sort|groupby|snappy)_[a-z0-9_]+)`", sec):
        assert word.encode() in names, word
    out = C.c_int64(-12345)
    for name, default, probes in KNOBS:
        # (a) the name is a knob, a misspelling of it is not — for the getter and the setter alike
        for wrong in (name + b"_", name[:-1] + b"0"):
            assert lib.arx_get_option(wrong, C.byref(out)) == INVALID and _err(lib) == "unknown option '%s'" % wrong.decode()
            assert lib.arx_set_option(wrong, 1) == INVALID and _err(lib) == "unknown option '%s'" % wrong.decode()
        # (b) untouched, it holds its default
        assert U.get_option(lib, name) == default, name
        # (c) what is stored for what is given
        assert any(given == default and stored == default for given, stored in probes), name
        with U.options(lib, {name: default}):
            for given, stored in probes:
                assert lib.arx_set_option(name, given) == OK, (name, given)
                assert U.get_option(lib, name) == stored, (name, given, stored, U.get_option(lib, name))
                # ... and for no other knob (two rows on one variable would show here)
                if stored != default:
                    moved = [other for other, d, _ in KNOBS if other != name and U.get_option(lib, other) != d]
                    assert not moved, (name, given, moved)
    assert lib.arx_get_option(None, C.byref(out)) == INVALID and lib.arx_set_option(None, 1) == INVALID
    assert lib.arx_get_option(names[0], None) == INVALID
    # (d) and every knob is back at its default
    for name, default, _ in KNOBS:
        assert U.get_option(lib, name) == default, name


def _check_counters(lib):
    for name in COUNTERS:
        assert lib.arx_get_counter(name) >= 0, name
    for wrong in (b"sort_wide_run", b"groupby_slices", b""):
        assert lib.arx_get_counter(wrong) == -1 and _err(lib) == "unknown counter '%s'" % wrong.decode()
    assert lib.arx_get_counter(None) == -1 and _err(lib) == "unknown counter '(null)'"


def test_knob_table(emu_ctx):
    _check_knob_table(emu_ctx._lib.get_lib())


def test_counter_names(emu_ctx):
    _check_counters(emu_ctx._lib.get_lib())


@pytest.mark.gpu
def test_knob_table_on_the_device_library(gpu_ctx):
    _check_knob_table(gpu_ctx._lib.get_lib())


@pytest.mark.gpu
def test_counter_names_on_the_device_library(gpu_ctx):
    _check_counters(gpu_ctx._lib.get_lib())
