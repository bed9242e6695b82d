"""Times binary_join_element_wise (csrc/string_join.hip) on columns generated on the device against the project's own copy
of the same bytes: the summed time of a full-range binary_slice(0, None) of each input column (offsets + data calls), timed
in the same run on the same columns.  The join moves the same bytes once more a separator per piece, and reads the
operands' offsets once more per piece, so a ratio near 1 is the copy's speed and about 1.5 is one extra pass over the
offsets per piece.

    2 and 4 value columns, a one-byte literal separator, emit_null, no nulls; 2^--log2-out-bytes bytes of values in all,
    at mean value sizes 8, 32, 128 and 1024 (rows of mean / 2 .. 3 mean / 2 bytes, 'a' .. 'z')

A join is timed as its two calls together, as each slice is; the two calls are also timed apart.  Median of --reps
device-event timings after 3 warm-up calls.  The device result's first 2^16 rows are checked against pyarrow.  Writes the
table to --out.

    python scripts/exp_string_join.py [--log2-out-bytes 27] [--reps 10] [--out profiles/string_join.txt]
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
EMIT_NULL = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-out-bytes", type=int, default=27)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_join.txt"))
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
    gen = torch.Generator(device=dev).manual_seed(67)
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

    class Column:
        """n rows of lo .. hi bytes of 'a' .. 'z'."""

        def __init__(self, n, lo, hi):
            lengths = torch.randint(lo, hi + 1, (n,), dtype=torch.int64, device=dev, generator=gen)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum(lengths, 0, out=offsets[1:])
            self.n, self.nbytes = n, int(offsets[-1])
            self.offsets = offsets.to(torch.int32)
            self.data = torch.randint(97, 123, (self.nbytes + 64,), dtype=torch.uint8, device=dev, generator=gen)
            self.span = _lib.ArxBinarySpan(None, self.offsets.data_ptr(), self.data.data_ptr(), 0, n, 0)

        def host(self, m):
            offs = self.offsets[: m + 1].cpu().numpy()
            return pa.Array.from_buffers(pa.binary(), m, [None, pa.py_buffer(offs.tobytes()), pa.py_buffer(self.data[: int(offs[-1])].cpu().numpy().tobytes())])

    class Case:
        def __init__(self, k, n, lo, hi):
            self.k, self.n = k, n
            self.cols = [Column(n, lo, hi) for _ in range(k)]
            self.nbytes = sum(c.nbytes for c in self.cols)
            out = self.nbytes + (k - 1) * n
            assert out < 2**31, "the result does not fit int32 offsets"
            self.sep = torch.frombuffer(bytearray(b"-"), dtype=torch.uint8).to(dev)
            self.table = (_lib.ArxJoinOperand * (k + 1))()
            for slot, c in zip(self.table, self.cols):
                slot.kind, slot.column = _lib.JOIN_COLUMN, c.span
            self.table[k].kind, self.table[k].literal, self.table[k].literal_length = _lib.JOIN_LITERAL, self.sep.data_ptr(), 1
            self.out_offsets = torch.empty((n + 1) * 4 + 64, dtype=torch.uint8, device=dev)
            self.out_valid = torch.empty((n + 63) // 64 * 8 + 8, dtype=torch.uint8, device=dev)
            self.out_data = torch.empty(out + 64, dtype=torch.uint8, device=dev)
            self.ws_bytes = max(lib.arx_string_slice_workspace_bytes(n, 4), lib.arx_binary_join_workspace_bytes(n, 4))
            self.ws = torch.empty(self.ws_bytes + 64, dtype=torch.uint8, device=dev)
            self.total, self.nulls = C.c_int64(0), C.c_int64(0)

        def slices(self):
            for c in self.cols:
                ok(lib.arx_string_slice_offsets(C.byref(c.span), 4, BYTES, 0, NO_STOP, c.nbytes, 0, self.ws.data_ptr(), self.ws_bytes,
                                                self.out_offsets.data_ptr(), C.byref(self.total), stream))
                ok(lib.arx_string_slice_data(C.byref(c.span), 4, self.ws.data_ptr(), self.ws_bytes, self.out_offsets.data_ptr(),
                                             self.total.value, self.out_data.data_ptr(), stream))

        def join_offsets(self):
            ok(lib.arx_binary_join_offsets(self.table, self.k + 1, self.n, 4, EMIT_NULL, 0, self.ws.data_ptr(), self.ws_bytes,
                                           self.out_offsets.data_ptr(), self.out_valid.data_ptr(), C.byref(self.nulls), C.byref(self.total), stream))

        def join_data(self):
            ok(lib.arx_binary_join_data(self.table, self.k + 1, self.n, 4, EMIT_NULL, None, 0, self.out_offsets.data_ptr(), self.total.value,
                                        self.out_data.data_ptr(), stream))

        def join(self):
            self.join_offsets()
            self.join_data()

        def check(self, m=1 << 16):
            """The result left by the last join, first m rows, against pyarrow."""
            m = min(m, self.n)
            torch.cuda.synchronize()
            got_offsets = self.out_offsets[: (m + 1) * 4].cpu().numpy().view(np.int32)
            got = pa.Array.from_buffers(pa.binary(), m, [None, pa.py_buffer(got_offsets.tobytes()),
                                                         pa.py_buffer(self.out_data[: int(got_offsets[-1])].cpu().numpy().tobytes())])
            assert got.equals(pc.binary_join_element_wise(*[c.host(m) for c in self.cols], b"-")), "differs from pyarrow's"

    emit(f"# binary_join_element_wise, {torch.cuda.get_device_name(0)}; no nulls, emit_null, separator '-'; pyarrow {pa.__version__} checks the "
         "first 2^16 rows of every case")
    emit(f"# ms: median (min .. max) of {a.reps} after 3 warm-up calls, device events around the C-ABI calls")
    emit("# yardstick = binary_slice(0, None) (offsets + data) of each value column, summed; ratio = join (offsets + data) / yardstick")
    emit()
    emit(f"{'values':>6} {'mean':>5} {'rows':>9} {'out bytes':>11} {'slices ms':>22} {'join ms':>22} {'ratio':>6} {'join offsets ms':>22} {'join data ms':>22} {'data GB/s':>9}")
    fmt = lambda t: f"{t[0]:>8.3f} ({t[1]:.3f}..{t[2]:.3f})"   # noqa: E731
    budget = 1 << a.log2_out_bytes
    for k in (2, 4):
        for mean in (8, 32, 128, 1024):
            n = budget // (k * mean)
            case = Case(k, n, mean // 2, mean + mean // 2)
            t_slices = timed(case.slices)
            t_join = timed(case.join)
            assert case.total.value == case.nbytes + (k - 1) * n and case.nulls.value == 0
            case.check()
            t_offsets = timed(case.join_offsets)
            t_data = timed(case.join_data)
            emit(f"{k:>6} {mean:>5} {n:>9} {case.total.value:>11} {fmt(t_slices):>22} {fmt(t_join):>22} {t_join[0] / t_slices[0]:>6.2f} "
                 f"{fmt(t_offsets):>22} {fmt(t_data):>22} {2 * case.total.value / t_data[0] / 1e6:>9.0f}")
            del case
            torch.cuda.empty_cache()
    emit("# data GB/s: (bytes read + bytes written) of the data call = 2 x out bytes, over its time")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
