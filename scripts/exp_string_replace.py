"""Times replace_substring (csrc/string_replace.hip) on columns generated on the device, both forms, against the work it
cannot do without: with a pattern that never occurs it does what one match_substring plus one whole-row
binary_slice(0, None) of the same column do (both existing kernels), so its time is reported as a ratio of their sum,
timed in the same run on the same column.

    a pattern that never occurs     2^--log2-rows rows of 16 bytes, then 2^--log2-sweep-bytes data bytes at mean row sizes
                                    16, 64, 128, 256, 512, 1024 and 4096 (rows of mean / 2 .. 3 mean / 2 bytes, 'a' .. 'z', no nulls);
                                    where the waves form overtakes the rows form is where kWavesPathMeanRow belongs
    a frequent pattern              2^--log2-sweep-bytes data bytes at a mean row of 64, the 4-byte pattern twice in every
                                    row, the replacement longer (8), shorter (1) and equal (4): both forms' times

A replace is timed as its two calls together, as the slice is.  Median of --reps device-event timings after 3 warm-up
calls.  The device results of the first 2^16 rows are checked against pyarrow.  Writes the table to --out.

    python scripts/exp_string_replace.py [--log2-rows 26] [--log2-sweep-bytes 27] [--reps 10] [--out profiles/string_replace.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = 0
NO_STOP = 2**63 - 1
ROWS, WAVES = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=26)
    ap.add_argument("--log2-sweep-bytes", type=int, default=27)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_replace.txt"))
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
    gen = torch.Generator(device=dev).manual_seed(61)
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

    def literal(raw):
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)

    class Column:
        """Rows of lo .. hi bytes of 'a' .. 'z' with everything the timed calls write into."""

        def __init__(self, n, lo, hi, grow):
            lengths = torch.randint(lo, hi + 1, (n,), dtype=torch.int64, device=dev, generator=gen)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum(lengths, 0, out=offsets[1:])
            self.n, self.nbytes = n, int(offsets[-1])
            assert self.nbytes + grow * n < 2**31, "the column's data does not fit int32 offsets"
            self.offsets = offsets.to(torch.int32)
            self.data = torch.randint(97, 123, (self.nbytes + 64,), dtype=torch.uint8, device=dev, generator=gen)
            self.span = _lib.ArxBinarySpan(None, self.offsets.data_ptr(), self.data.data_ptr(), 0, n, 0)
            self.out_offsets = torch.empty((n + 1) * 4 + 64, dtype=torch.uint8, device=dev)
            self.out_data = torch.empty(self.nbytes + grow * n + 64, dtype=torch.uint8, device=dev)
            self.bits = torch.empty((n + 63) // 64 * 8 + 8, dtype=torch.uint8, device=dev)
            self.ws_bytes = max(lib.arx_string_slice_workspace_bytes(n, 4), lib.arx_replace_substring_workspace_bytes(n, 4))
            self.ws = torch.empty(self.ws_bytes + 64, dtype=torch.uint8, device=dev)
            self.total = C.c_int64(0)

        def match(self, pat):
            ok(lib.arx_match_substring(C.byref(self.span), 4, 0, pat.data_ptr(), pat.numel(), self.nbytes, 0, self.bits.data_ptr(), stream))

        def slice_all(self):
            ok(lib.arx_string_slice_offsets(C.byref(self.span), 4, BYTES, 0, NO_STOP, self.nbytes, 0, self.ws.data_ptr(), self.ws_bytes,
                                            self.out_offsets.data_ptr(), C.byref(self.total), stream))
            ok(lib.arx_string_slice_data(C.byref(self.span), 4, self.ws.data_ptr(), self.ws_bytes, self.out_offsets.data_ptr(),
                                         self.total.value, self.out_data.data_ptr(), stream))

        def replace(self, pat, rep, path):
            ok(lib.arx_replace_substring_offsets(C.byref(self.span), 4, pat.data_ptr(), pat.numel(), rep.numel(), -1, self.nbytes, path,
                                                 self.ws.data_ptr(), self.ws_bytes, self.out_offsets.data_ptr(), C.byref(self.total), stream))
            ok(lib.arx_replace_substring_data(C.byref(self.span), 4, pat.data_ptr(), pat.numel(), rep.data_ptr(), rep.numel(), -1, path,
                                              self.ws.data_ptr(), self.ws_bytes, self.out_offsets.data_ptr(), self.total.value,
                                              self.out_data.data_ptr(), stream))

        def check(self, pat, rep, m=1 << 16):
            """The result left by the last replace, first m rows, against pyarrow."""
            m = min(m, self.n)
            torch.cuda.synchronize()
            host_offsets = self.offsets[: m + 1].cpu().numpy()
            harr = pa.Array.from_buffers(pa.binary(), m, [None, pa.py_buffer(host_offsets.tobytes()),
                                                          pa.py_buffer(self.data[: int(host_offsets[-1])].cpu().numpy().tobytes())])
            got_offsets = self.out_offsets[: (m + 1) * 4].cpu().numpy().view(np.int32)
            got = pa.Array.from_buffers(pa.binary(), m, [None, pa.py_buffer(got_offsets.tobytes()),
                                                         pa.py_buffer(self.out_data[: int(got_offsets[-1])].cpu().numpy().tobytes())])
            assert got.equals(pc.replace_substring(harr, bytes(pat.cpu().numpy()), bytes(rep.cpu().numpy()))), "differs from pyarrow's"

    emit(f"# replace_substring, {torch.cuda.get_device_name(0)}; no nulls; pyarrow {pa.__version__} checks the first 2^16 rows of every column")
    emit(f"# ms: median (min .. max) of {a.reps} after 3 warm-up calls, device events around the C-ABI call(s)")
    emit("# yardstick = match_substring (auto path) + binary_slice(0, None) (offsets + data) of the same column; ratio = replace / yardstick")
    emit()
    emit("# a pattern that never occurs ('wxyzwxy#' in rows of 'a' .. 'z')")
    emit(f"{'mean row':>8} {'rows':>10} {'match ms':>22} {'slice ms':>22} {'sum':>8} {'replace rows ms':>22} {'ratio':>6} {'replace waves ms':>22} {'ratio':>6}  faster")
    never, rep = literal(b"wxyzwxy#"), literal(b"0123456789")
    fmt = lambda t: f"{t[0]:>8.3f} ({t[1]:.3f}..{t[2]:.3f})"   # noqa: E731
    crossover = None
    sweep = 1 << a.log2_sweep_bytes
    for mean, n, lo, hi in [(16, 1 << a.log2_rows, 16, 16)] + [(mean, sweep // mean, mean // 2, mean + mean // 2) for mean in (16, 64, 128, 256, 512, 1024, 4096)]:
        col = Column(n, lo, hi, 0)
        t_match, t_slice = timed(lambda: col.match(never)), timed(col.slice_all)
        assert col.total.value == col.nbytes
        t_rows = timed(lambda: col.replace(never, rep, ROWS))
        assert col.total.value == col.nbytes, "the pattern occurred"
        col.check(never, rep)
        t_waves = timed(lambda: col.replace(never, rep, WAVES))
        assert col.total.value == col.nbytes
        col.check(never, rep)
        both = t_match[0] + t_slice[0]
        emit(f"{mean:>8} {n:>10} {fmt(t_match):>22} {fmt(t_slice):>22} {both:>8.3f} {fmt(t_rows):>22} {t_rows[0] / both:>6.2f} {fmt(t_waves):>22} "
             f"{t_waves[0] / both:>6.2f}  {'waves' if t_waves[0] < t_rows[0] else 'rows'}")
        if lo != hi and crossover is None and t_waves[0] < t_rows[0]:
            crossover = mean
        del col
        torch.cuda.empty_cache()
    emit(f"# first mean row size of the sweep at which the waves form is faster: {crossover}")
    emit()

    emit("# a frequent pattern: '@#@!' twice in every row, mean row 64 bytes")
    n = sweep // 64
    col = Column(n, 32, 96, 8)
    pat = literal(b"@#@!")
    starts = col.offsets[:-1].to(torch.int64)
    for at in (starts + 3, starts + 19):
        for k in range(4):
            col.data[at + k] = int(pat[k])
    emit(f"{'replacement':<14} {'rows':>10} {'out bytes':>12} {'replace rows ms':>22} {'replace waves ms':>22}")
    for label, raw in (("longer (8)", b"<<<<>>>>"), ("shorter (1)", b"-"), ("equal (4)", b"!@#@")):
        rep = literal(raw)
        t_rows = timed(lambda: col.replace(pat, rep, ROWS))
        col.check(pat, rep)
        t_waves = timed(lambda: col.replace(pat, rep, WAVES))
        col.check(pat, rep)
        assert col.total.value == col.nbytes + 2 * n * (len(raw) - 4)
        emit(f"{label:<14} {n:>10} {col.total.value:>12} {fmt(t_rows):>22} {fmt(t_waves):>22}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
