"""Times the string length and slice calls (csrc/string_slice.hip) on columns generated on the device, each against a
yardstick of the library's own kernels moving the same bytes; a measured call may take its yardstick's time x 1.05.

    binary_length                                   add int32 + scalar over the same row count
    binary_slice(0, None), utf8_slice_codeunits(0, None)
                                                    an identity take of the same column (int32 indices 0 .. n - 1):
                                                    arx_binary_take_offsets + arx_binary_take_data
    utf8_length                                     arx_match_substring on its bytes path over the same column, rare pattern
    utf8_slice_codeunits(-3, None)                  the identity take + the bytes-path read (the sum of both)

binary_length runs over 2^--log2-rows rows (offsets only: no data byte is read, rows of 0 .. 7 bytes keep int32 offsets);
the others over 2^--log2-slice-rows rows of 0 .. 32 bytes (mean 16, 'a' .. 'z', no nulls): the largest power of two whose
data fits int32 offsets.  A slice is timed as its two calls together, as the take is.  Then both forms of the codepoint
walk (rows: one lane per row, waves: one wave per row) at mean row sizes 8 .. 4096 bytes over 2^--log2-sweep-bytes data
bytes: where they cross is where kWavesPathMeanRow belongs.  Median of --reps device-event timings after 3 warm-up calls.
The device results of the first 2^18 rows are checked against pyarrow.  Writes the table to --out.

    python scripts/exp_string_slice.py [--log2-rows 28] [--log2-slice-rows 26] [--log2-sweep-bytes 28] [--reps 10] [--out profiles/string_slice.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARX_NUM_INT32, ARX_ARITH_ADD, INDEX_INT32 = 4, 0, 5
BYTES, CODEPOINTS = 0, 1
NO_STOP = 2**63 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=28)
    ap.add_argument("--log2-slice-rows", type=int, default=26)
    ap.add_argument("--log2-sweep-bytes", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_slice.txt"))
    a = ap.parse_args()
    assert a.reps >= 10, "median of at least 10"
    import pyarrow as pa
    import pyarrow.compute as pc
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import current_stream

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.get_lib()
    stream = current_stream(dev)
    gen = torch.Generator(device=dev).manual_seed(59)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        times = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if i >= 3:
                times.append(e0.elapsed_time(e1))
        return float(np.median(times)), min(times), max(times)

    def ok(rc):
        assert rc == 0, lib.arx_last_error()

    def offsets_of(n, lo, hi):
        lengths = torch.randint(lo, hi + 1, (n,), dtype=torch.int64, device=dev, generator=gen)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lengths, 0, out=offsets[1:])
        nbytes = int(offsets[-1])
        assert nbytes < 2**31, "the column's data does not fit int32 offsets"
        return offsets.to(torch.int32), nbytes

    def row(label, t, nbytes, extra=""):
        ms, lo, hi = t
        emit(f"{label:<44} {ms:>9.3f} {lo:>9.3f} {hi:>9.3f} {nbytes / ms / 1e6:>9.1f} {extra}")

    def verdict(t, bound, missed, label):
        if t[0] <= bound:
            return f"within the bound {bound:.3f}"
        missed.append(f"{label} {t[0]:.3f} > {bound:.3f}")
        return f"MISSES the bound {bound:.3f}"

    emit(f"# string lengths and slices, {torch.cuda.get_device_name(0)}; no nulls; pyarrow {pa.__version__} checks the first 2^18 rows")
    emit(f"# ms: median / min / max of {a.reps} after 3 warm-up calls, device events around the C-ABI call(s); GB/s over the bytes named")
    emit(f"{'call':<44} {'ms':>9} {'min':>9} {'max':>9} {'GB/s':>9}")
    missed = []

    # ---- binary_length against add int32 + scalar
    n = 1 << a.log2_rows
    offsets, _ = offsets_of(n, 0, 7)
    out = torch.empty(n * 4 + 64, dtype=torch.uint8, device=dev)
    seven = C.c_int32(7)
    t_add = timed(lambda: ok(lib.arx_arith_numeric(ARX_ARITH_ADD, 0, ARX_NUM_INT32, offsets.data_ptr(), None, None, 0, None,
                                                   C.cast(C.pointer(seven), C.c_void_p), None, 0, n, out.data_ptr(), None, stream)))
    row(f"add int32 + scalar, 2^{a.log2_rows} rows", t_add, n * 8, "yardstick (4 + 4 bytes a row)")
    span = _lib.ArxBinarySpan(None, offsets.data_ptr(), None, 0, n, 0)
    t = timed(lambda: ok(lib.arx_string_length(C.byref(span), 4, BYTES, -1, 0, out.data_ptr(), stream)))
    row(f"binary_length, 2^{a.log2_rows} rows", t, n * 8, verdict(t, t_add[0] * 1.05, missed, "binary_length"))
    got = out[: 4 << 18].cpu().numpy().view(np.int32)
    assert (got == np.diff(offsets[: (1 << 18) + 1].cpu().numpy())).all(), "binary_length differs from the offsets' differences"
    del offsets, out
    torch.cuda.empty_cache()
    emit()

    # ---- the slices and utf8_length over rows of mean 16 bytes
    n = 1 << a.log2_slice_rows
    offsets, nbytes = offsets_of(n, 0, 32)
    data = torch.randint(97, 123, (nbytes + 64,), dtype=torch.uint8, device=dev, generator=gen)
    span = _lib.ArxBinarySpan(None, offsets.data_ptr(), data.data_ptr(), 0, n, 0)
    out_offsets = torch.empty((n + 1) * 4 + 64, dtype=torch.uint8, device=dev)
    out_data = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    out_len = torch.empty(n * 4 + 64, dtype=torch.uint8, device=dev)
    bits = torch.empty((n + 63) // 64 * 8 + 8, dtype=torch.uint8, device=dev)
    indices = torch.arange(n, dtype=torch.int32, device=dev)
    ispan = _lib.ArxSpan(None, indices.data_ptr(), 0, n, 0)
    ws_bytes = max(lib.arx_binary_take_workspace_bytes(n), lib.arx_string_slice_workspace_bytes(n, 4))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device=dev)
    pattern = torch.frombuffer(bytearray(b"wxyzwxyz"), dtype=torch.uint8).to(dev)
    total = C.c_int64(0)

    def take():
        ok(lib.arx_binary_take_offsets(C.byref(span), C.byref(ispan), INDEX_INT32, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), None,
                                       None, C.byref(total), stream))
        ok(lib.arx_binary_take_data(C.byref(span), n, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), total.value, out_data.data_ptr(), stream))

    def slice_(unit, start, stop, path=0):
        ok(lib.arx_string_slice_offsets(C.byref(span), 4, unit, start, stop, nbytes, path, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(),
                                        C.byref(total), stream))
        ok(lib.arx_string_slice_data(C.byref(span), 4, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), total.value, out_data.data_ptr(), stream))

    rows = f"2^{a.log2_slice_rows} rows of mean {nbytes / n:.1f} bytes"
    copy_bytes = 2 * nbytes + 2 * (n + 1) * 4
    t_take = timed(take)
    row(f"identity take, {rows}", t_take, copy_bytes + 4 * n, "yardstick (data and offsets in and out, indices in)")
    t_read = timed(lambda: ok(lib.arx_match_substring(C.byref(span), 4, 0, pattern.data_ptr(), 8, nbytes, 2, bits.data_ptr(), stream)))
    row(f"match_substring bytes path, {rows}", t_read, nbytes + (n + 1) * 4 + n // 8, "yardstick (data and offsets in, bits out)")
    for label, unit in (("binary_slice(0, None)", BYTES), ("utf8_slice_codeunits(0, None)", CODEPOINTS)):
        t = timed(lambda: slice_(unit, 0, NO_STOP))
        assert total.value == nbytes
        row(label, t, copy_bytes, verdict(t, t_take[0] * 1.05, missed, label))
    t = timed(lambda: ok(lib.arx_string_length(C.byref(span), 4, CODEPOINTS, nbytes, 0, out_len.data_ptr(), stream)))
    row("utf8_length", t, nbytes + (n + 1) * 4 + n * 4, verdict(t, t_read[0] * 1.05, missed, "utf8_length"))
    t = timed(lambda: slice_(CODEPOINTS, -3, NO_STOP))
    row("utf8_slice_codeunits(-3, None)", t, nbytes + 2 * total.value + 2 * (n + 1) * 4,
        verdict(t, (t_take[0] + t_read[0]) * 1.05, missed, "utf8_slice_codeunits(-3, None)"))
    emit(f"# lines that miss their bound: {'; '.join(missed) if missed else 'none'}")
    # ---- the first 2^18 rows against pyarrow
    m = 1 << 18
    host_offsets = offsets[: m + 1].cpu().numpy()
    harr = pa.Array.from_buffers(pa.string(), m, [None, pa.py_buffer(host_offsets.tobytes()),
                                                  pa.py_buffer(data[: int(host_offsets[-1])].cpu().numpy().tobytes())])
    torch.cuda.synchronize()
    assert (out_len[: 4 * m].cpu().numpy().view(np.int32) == pc.utf8_length(harr).to_numpy()).all(), "utf8_length differs from pyarrow's"
    got_offsets = out_offsets[: (m + 1) * 4].cpu().numpy().view(np.int32)
    got = pa.Array.from_buffers(pa.string(), m, [None, pa.py_buffer(got_offsets.tobytes()),
                                                 pa.py_buffer(out_data[: int(got_offsets[-1])].cpu().numpy().tobytes())])
    assert got.equals(pc.utf8_slice_codeunits(harr, -3)), "utf8_slice_codeunits(-3, None) differs from pyarrow's"
    emit("# utf8_length and utf8_slice_codeunits(-3, None) of the first 2^18 rows equal pyarrow's")
    del offsets, data, out_offsets, out_data, out_len, bits, indices, ws
    torch.cuda.empty_cache()
    emit()

    # ---- both forms of the codepoint walk over the mean row size
    sweep = 1 << a.log2_sweep_bytes
    emit(f"# the codepoint walk, rows form (one lane per row) against waves form (one wave per row), about 2^{a.log2_sweep_bytes} data bytes")
    emit(f"{'mean row bytes':<16} {'rows':>10} {'call':<32} {'rows ms':>9} {'waves ms':>9}  faster")
    crossover = None
    for mean in (8, 32, 128, 512, 4096):
        n = sweep // mean
        offsets, nbytes = offsets_of(n, mean // 2, mean + mean // 2)
        data = torch.randint(97, 123, (nbytes + 64,), dtype=torch.uint8, device=dev, generator=gen)
        span = _lib.ArxBinarySpan(None, offsets.data_ptr(), data.data_ptr(), 0, n, 0)
        out_offsets = torch.empty((n + 1) * 4 + 64, dtype=torch.uint8, device=dev)
        out_len = torch.empty(n * 4 + 64, dtype=torch.uint8, device=dev)
        ws_bytes = lib.arx_string_slice_workspace_bytes(n, 4)
        ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device=dev)
        calls = (("utf8_length", lambda p: ok(lib.arx_string_length(C.byref(span), 4, CODEPOINTS, nbytes, p, out_len.data_ptr(), stream))),
                 ("slice offsets (-3, None)", lambda p: ok(lib.arx_string_slice_offsets(C.byref(span), 4, CODEPOINTS, -3, NO_STOP, nbytes, p, ws.data_ptr(), ws_bytes,
                                                                                         out_offsets.data_ptr(), C.byref(total), stream))),
                 ("slice offsets (mean / 2, None)", lambda p: ok(lib.arx_string_slice_offsets(C.byref(span), 4, CODEPOINTS, mean // 2, NO_STOP, nbytes, p, ws.data_ptr(),
                                                                                               ws_bytes, out_offsets.data_ptr(), C.byref(total), stream))))
        for label, call in calls:
            t_rows, t_waves = timed(lambda: call(1)), timed(lambda: call(2))
            emit(f"{mean:<16} {n:>10} {label:<32} {t_rows[0]:>9.3f} {t_waves[0]:>9.3f}  {'waves' if t_waves[0] < t_rows[0] else 'rows'}")
            if label == "utf8_length" and crossover is None and t_waves[0] < t_rows[0]:
                crossover = mean
        del offsets, data, out_offsets, out_len, ws
        torch.cuda.empty_cache()
    emit(f"# first mean row size at which the waves form counts a column faster: {crossover}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
