"""Times arx_compare_binary (csrc/string_compare.hip) on columns generated on the device, each line against yardsticks of
the library's own kernels over the same columns; a measured call may take its yardstick's time x 1.05.

    lengths          arx_string_length in bytes: streams the offsets only, the floor of an `equal` that the lengths decide
    starts_with      arx_match_substring(starts_with, the same literal) on the rows path, for array x literal
    never, summed    arx_match_substring on the bytes path with a pattern that never occurs, over each column, summed:
                     reads every byte, for array x array on equal rows

Columns of 'a' .. 'z' without nulls, at 2^--log2-rows rows of 0 .. 32 bytes (mean 16) and half as many of 0 .. 64 (mean 32):
    equal / less against a 16-byte literal (most rows differ from it in length)
    equal / less of the column and a copy that differs in one byte of 10 % of its rows
and 2^(--log2-rows - 6) rows of 2 KiB that share all but their last byte (int64 offsets), on both paths.  Then the sweep
behind the threshold of path 0: `less` on both paths over two columns of 2^(--log2-rows + 2) data bytes each whose rows
of 64 .. 8192 bytes are equal but for the last byte.
Median of --reps device-event timings after 3 warm-up calls.  The first 2^18 rows of every timed call are checked against
pyarrow.  Writes the table to --out.

    python scripts/exp_string_compare.py [--log2-rows 26] [--reps 10] [--out profiles/string_compare.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EQUAL, LESS = 0, 4
AUTO, ROWS, WAVES = 0, 1, 2
BYTES_UNIT, STARTS_WITH, MATCH, MATCH_ROWS, MATCH_BYTES = 0, 1, 0, 1, 2
NAMES = {EQUAL: "equal", LESS: "less"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_compare.txt"))
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
    lines, missed = [], []

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

    def row(label, t, moved, extra):
        emit(f"{label:<58} {t[0]:>9.3f} {t[1]:>9.3f} {t[2]:>9.3f} {moved / t[0] / 1e6:>9.1f} {extra}")

    def verdict(label, t, yards):
        out = []
        for name, yard in yards:
            inside = t[0] <= yard * 1.05
            out.append(f"{'inside' if inside else 'OUTSIDE'} {name} x 1.05 = {yard * 1.05:.3f}")
            if not inside:
                missed.append(f"{label} {t[0]:.3f} > {name} {yard * 1.05:.3f}")
        return "; ".join(out)

    class Column:
        """offsets of `width` bytes and data on the device"""

        def __init__(self, lengths, width, data=None):
            self.n, self.width = len(lengths), width
            offsets = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
            torch.cumsum(lengths, 0, out=offsets[1:])
            self.nbytes = int(offsets[-1])
            assert width == 8 or self.nbytes < 2**31, "the column's data does not fit int32 offsets"
            self.offsets = offsets if width == 8 else offsets.to(torch.int32)
            self.data = data if data is not None else torch.randint(97, 123, (self.nbytes + 64,), dtype=torch.uint8, device=dev, generator=gen)
            self.span = _lib.ArxBinarySpan(None, self.offsets.data_ptr(), self.data.data_ptr(), 0, self.n, 0)

        def copy_with(self, data):
            c = Column.__new__(Column)
            c.n, c.width, c.nbytes, c.offsets, c.data = self.n, self.width, self.nbytes, self.offsets, data
            c.span = _lib.ArxBinarySpan(None, c.offsets.data_ptr(), c.data.data_ptr(), 0, c.n, 0)
            return c

        def traffic(self):
            return (self.n + 1) * self.width + self.nbytes

        def host(self, m):
            off = self.offsets[: m + 1].cpu().numpy()
            return pa.Array.from_buffers(pa.binary() if self.width == 4 else pa.large_binary(), m,
                                         [None, pa.py_buffer(off.tobytes()), pa.py_buffer(self.data[: int(off[-1])].cpu().numpy().tobytes())])

    def device_bytes(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def compare(op, left, right, literal, path, out):
        col = left if left is not None else right
        hint = sum(c.nbytes for c in (left, right) if c is not None)
        ok(lib.arx_compare_binary(op, C.byref(left.span) if left is not None else None, C.byref(right.span) if right is not None else None,
                                  col.width, literal.data_ptr() if literal is not None else None, len(literal) if literal is not None else 0,
                                  hint, path, out.data_ptr(), stream))

    def checked(op, left, right, literal_bytes, out):
        """the first 2^18 answers against pyarrow"""
        col = left if left is not None else right
        m = min(1 << 18, col.n)
        torch.cuda.synchronize()
        got = np.unpackbits(out[: (m + 7) // 8].cpu().numpy(), bitorder="little")[:m].astype(bool)
        sides = [c.host(m) if c is not None else pa.scalar(literal_bytes, col.host(1).type) for c in (left, right)]
        want = getattr(pc, NAMES[op])(*sides).to_numpy(zero_copy_only=False)
        assert (got == want).all(), f"{NAMES[op]} differs from pyarrow's"

    def yard_lengths(col, scratch):
        return timed(lambda: ok(lib.arx_string_length(C.byref(col.span), col.width, BYTES_UNIT, -1, 0, scratch.data_ptr(), stream)))

    def yard_match(col, op, pat, path, out):
        return timed(lambda: ok(lib.arx_match_substring(C.byref(col.span), col.width, op, pat.data_ptr(), len(pat), col.nbytes, path,
                                                        out.data_ptr(), stream)))

    emit(f"# string comparisons, {torch.cuda.get_device_name(0)}; no nulls; pyarrow {pa.__version__} checks the first 2^18 rows of every timed call")
    emit(f"# ms: median / min / max of {a.reps} after 3 warm-up calls, device events around the C-ABI call; GB/s over the operands' offsets and")
    emit("# data plus the bitmap written (nominal: an `equal` that the lengths decide reads no data)")
    emit(f"{'call':<58} {'ms':>9} {'min':>9} {'max':>9} {'GB/s':>9}")
    literal_bytes = b"shipped_and_paid"
    assert len(literal_bytes) == 16
    literal, never = device_bytes(literal_bytes), device_bytes(b"A#never#")
    for shift, top in ((0, 32), (1, 64)):
        n = 1 << (a.log2_rows - shift)
        col = Column(torch.randint(0, top + 1, (n,), dtype=torch.int64, device=dev, generator=gen), 4)
        # a copy that differs in one byte of 10 % of its rows
        other_data = col.data.clone()
        rows = torch.nonzero((torch.rand(n, device=dev, generator=gen) < 0.1) & (col.offsets[1:] > col.offsets[:-1])).flatten()
        other_data[col.offsets[rows].long()] = 65
        other = col.copy_with(other_data)
        out = torch.empty(n // 8 + 64, dtype=torch.uint8, device=dev)
        scratch = torch.empty(n * 4 + 64, dtype=torch.uint8, device=dev)
        tag = f"2^{a.log2_rows - shift} x {top // 2}"
        emit(f"# {n} rows of 0 .. {top} bytes, {col.nbytes / n:.1f} bytes a row")
        t_len = yard_lengths(col, scratch)
        t_starts = yard_match(col, STARTS_WITH, literal, MATCH_ROWS, out)
        t_never = [yard_match(c, MATCH, never, MATCH_BYTES, out) for c in (col, other)]
        row(f"[{tag}] lengths (binary_length)", t_len, (n + 1) * 4 + n * 4, "yardstick")
        row(f"[{tag}] starts_with(literal), rows", t_starts, col.traffic() + n // 8, "yardstick")
        row(f"[{tag}] never-matching pattern, bytes, both columns summed", tuple(x + y for x, y in zip(*t_never)),
            col.traffic() + other.traffic() + n // 4, "yardstick")
        for op in (EQUAL, LESS):
            label = f"[{tag}] {NAMES[op]}(column, literal)"
            t = timed(lambda: compare(op, col, None, literal, AUTO, out))
            yards = ([("lengths", t_len[0])] if op == EQUAL else []) + [("starts_with", t_starts[0])]
            row(label, t, col.traffic() + n // 8, verdict(label, t, yards))
            checked(op, col, None, literal_bytes, out)
        for op in (EQUAL, LESS):
            label = f"[{tag}] {NAMES[op]}(column, copy equal in 90 %)"
            t = timed(lambda: compare(op, col, other, None, AUTO, out))
            row(label, t, col.traffic() + other.traffic() + n // 8, verdict(label, t, [("never, summed", t_never[0][0] + t_never[1][0])]))
            checked(op, col, other, None, out)
        del col, other, other_data, out, scratch
        torch.cuda.empty_cache()
        emit()

    def shared_prefix_pair(n, size):
        """two columns of n rows of `size` bytes, equal but for each row's last byte"""
        col = Column(torch.full((n,), size, dtype=torch.int64, device=dev), 8)
        data = col.data.clone()
        data[col.offsets[1:] - 1] = 65
        return col, col.copy_with(data)

    n = 1 << (a.log2_rows - 6)
    col, other = shared_prefix_pair(n, 2048)
    out = torch.empty(n // 8 + 64, dtype=torch.uint8, device=dev)
    emit(f"# {n} rows of 2048 bytes that share all but their last byte (int64 offsets)")
    t_never = [yard_match(c, MATCH, never, MATCH_BYTES, out) for c in (col, other)]
    summed = t_never[0][0] + t_never[1][0]
    row("[2 KiB] never-matching pattern, bytes, both columns summed", tuple(x + y for x, y in zip(*t_never)),
        col.traffic() + other.traffic() + n // 4, "yardstick")
    for op in (EQUAL, LESS):
        for path, form in ((ROWS, "rows"), (WAVES, "waves")):
            label = f"[2 KiB] {NAMES[op]}(column, column), {form}"
            t = timed(lambda: compare(op, col, other, None, path, out))
            row(label, t, col.traffic() + other.traffic() + n // 8, verdict(label, t, [("never, summed", summed)]))
            checked(op, col, other, None, out)
    del col, other, out
    torch.cuda.empty_cache()
    emit()

    total = 1 << (a.log2_rows + 2)
    emit(f"# the sweep behind path 0: less(column, column), rows equal but for the last byte, {total} data bytes a column")
    emit(f"{'bytes a row':<58} {'rows ms':>9} {'waves ms':>9}")
    for size in (64, 128, 256, 512, 1024, 2048, 4096, 8192):
        n = total // size
        col, other = shared_prefix_pair(n, size)
        out = torch.empty(n // 8 + 64, dtype=torch.uint8, device=dev)
        t_rows = timed(lambda: compare(LESS, col, other, None, ROWS, out))
        checked(LESS, col, other, None, out)
        t_waves = timed(lambda: compare(LESS, col, other, None, WAVES, out))
        checked(LESS, col, other, None, out)
        emit(f"{size:<58} {t_rows[0]:>9.3f} {t_waves[0]:>9.3f}")
        del col, other, out
        torch.cuda.empty_cache()
    emit()
    emit("# the first 2^18 rows of every timed comparison equal pyarrow's")
    emit(f"# lines outside a bound: {'; '.join(missed) if missed else 'none'}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
