"""Times the trim calls (csrc/string_trim.hip: arx_string_trim_offsets + arx_string_slice_data) on columns generated on
the device, each against two yardsticks of the library's own kernels over the same column; a measured call may take a
yardstick's time x 1.05.

    identity take                     arx_binary_take_offsets + arx_binary_take_data, int32 indices 0 .. n - 1
    utf8_slice_codeunits(0, None)     the nearest existing call: one granule a row, then the same scan and copy

Three columns of 'a' .. 'z' without nulls:
    (a) nothing to trim       2^--log2-rows rows of 0 .. 32 bytes (mean 16)
    (b) a space at each end   2^--log2-rows rows of 2 .. 30 bytes (mean 16), the first and the last byte a space
    (c) right-padded          2^(--log2-rows - 1) rows of 32 bytes: a payload of 0 .. 32 bytes, then spaces (half the rows: 2^26
                              rows of 32 bytes do not fit int32 offsets; the data bytes are those of (a))
ascii_trim_whitespace and utf8_trim_whitespace run on (a) and (b), ascii_rtrim_whitespace and utf8_rtrim(" ") on (c).
Median of --reps device-event timings after 3 warm-up calls.  The first 2^18 rows of every timed call are checked against
pyarrow.  Writes the table to --out.

    python scripts/exp_string_trim.py [--log2-rows 26] [--reps 10] [--out profiles/string_trim.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INDEX_INT32, CODEPOINTS, NO_STOP = 5, 1, 2**63 - 1
LEFT, RIGHT, BOTH = 1, 2, 3
ASCII_WS, UTF8_WS, BYTE_SET, CODEPOINT_SET = 0, 1, 2, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_trim.txt"))
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

    def offsets_of(lengths):
        offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lengths, 0, out=offsets[1:])
        nbytes = int(offsets[-1])
        assert nbytes < 2**31, "the column's data does not fit int32 offsets"
        return offsets.to(torch.int32), nbytes

    def column(kind):
        n = 1 << (a.log2_rows - 1 if kind == "c" else a.log2_rows)
        if kind == "c":
            lengths = torch.full((n,), 32, dtype=torch.int64, device=dev)
        else:
            lo, hi = (0, 32) if kind == "a" else (2, 30)
            lengths = torch.randint(lo, hi + 1, (n,), dtype=torch.int64, device=dev, generator=gen)
        offsets, nbytes = offsets_of(lengths)
        data = torch.randint(97, 123, (nbytes + 64,), dtype=torch.uint8, device=dev, generator=gen)
        if kind == "b":
            data[offsets[:-1].long()] = 32
            data[offsets[1:].long() - 1] = 32
        elif kind == "c":
            payload = torch.randint(0, 33, (n, 1), dtype=torch.int64, device=dev, generator=gen)
            data[:nbytes].view(n, 32).masked_fill_(torch.arange(32, device=dev)[None, :] >= payload, 32)
        return n, offsets, nbytes, data

    emit(f"# string trimming, {torch.cuda.get_device_name(0)}; no nulls; pyarrow {pa.__version__} checks the first 2^18 rows of every timed call")
    emit(f"# ms: median / min / max of {a.reps} after 3 warm-up calls, device events around the two C-ABI calls; GB/s over data and offsets in and out")
    emit(f"{'call':<52} {'ms':>9} {'min':>9} {'max':>9} {'GB/s':>9}")
    missed = []
    space = (C.c_uint32 * 1)(32)
    inputs = {"a": ("nothing to trim", [("ascii_trim_whitespace", BOTH, ASCII_WS, None, 0), ("utf8_trim_whitespace", BOTH, UTF8_WS, None, 0)]),
              "b": ("a space at each end", [("ascii_trim_whitespace", BOTH, ASCII_WS, None, 0), ("utf8_trim_whitespace", BOTH, UTF8_WS, None, 0)]),
              "c": ("right-padded to 32 bytes", [("ascii_rtrim_whitespace", RIGHT, ASCII_WS, None, 0),
                                                 ("utf8_rtrim(' ')", RIGHT, CODEPOINT_SET, C.cast(space, C.c_void_p), 1)])}
    for kind, (what, trims) in inputs.items():
        n, offsets, nbytes, data = column(kind)
        span = _lib.ArxBinarySpan(None, offsets.data_ptr(), data.data_ptr(), 0, n, 0)
        out_offsets = torch.empty((n + 1) * 4 + 64, dtype=torch.uint8, device=dev)
        out_data = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
        indices = torch.arange(n, dtype=torch.int32, device=dev)
        ispan = _lib.ArxSpan(None, indices.data_ptr(), 0, n, 0)
        ws_bytes = max(lib.arx_binary_take_workspace_bytes(n), lib.arx_string_slice_workspace_bytes(n, 4))
        ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device=dev)
        total = C.c_int64(0)

        def take():
            ok(lib.arx_binary_take_offsets(C.byref(span), C.byref(ispan), INDEX_INT32, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), None,
                                           None, C.byref(total), stream))
            ok(lib.arx_binary_take_data(C.byref(span), n, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), total.value, out_data.data_ptr(), stream))

        def slice_all():
            ok(lib.arx_string_slice_offsets(C.byref(span), 4, CODEPOINTS, 0, NO_STOP, nbytes, 0, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(),
                                            C.byref(total), stream))
            ok(lib.arx_string_slice_data(C.byref(span), 4, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), total.value, out_data.data_ptr(), stream))

        def trim(sides, set_kind, members, count):
            ok(lib.arx_string_trim_offsets(C.byref(span), 4, sides, set_kind, members, count, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(),
                                           C.byref(total), stream))
            ok(lib.arx_string_slice_data(C.byref(span), 4, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(), total.value, out_data.data_ptr(), stream))

        def row(label, t, moved, extra):
            emit(f"{label:<52} {t[0]:>9.3f} {t[1]:>9.3f} {t[2]:>9.3f} {moved / t[0] / 1e6:>9.1f} {extra}")

        emit(f"# ({kind}) {what}: {n} rows, {nbytes / n:.1f} bytes a row")
        t_take, t_slice = timed(take), timed(slice_all)
        row(f"({kind}) identity take", t_take, 2 * nbytes + 2 * (n + 1) * 4, "yardstick")
        row(f"({kind}) utf8_slice_codeunits(0, None)", t_slice, 2 * nbytes + 2 * (n + 1) * 4, "yardstick")
        m = 1 << 18
        host_offsets = offsets[: m + 1].cpu().numpy()
        harr = pa.Array.from_buffers(pa.string(), m, [None, pa.py_buffer(host_offsets.tobytes()),
                                                      pa.py_buffer(data[: int(host_offsets[-1])].cpu().numpy().tobytes())])
        for label, sides, set_kind, members, count in trims:
            t = timed(lambda: trim(sides, set_kind, members, count))
            verdicts = []
            for name, yard in (("take", t_take), ("slice", t_slice)):
                inside = t[0] <= yard[0] * 1.05
                verdicts.append(f"{'inside' if inside else 'OUTSIDE'} the {name}'s bound {yard[0] * 1.05:.3f}")
                if not inside:
                    missed.append(f"({kind}) {label} {t[0]:.3f} > {name} {yard[0] * 1.05:.3f}")
            row(f"({kind}) {label}", t, nbytes + total.value + 2 * (n + 1) * 4, "; ".join(verdicts))
            torch.cuda.synchronize()
            got_offsets = out_offsets[: (m + 1) * 4].cpu().numpy().view(np.int32)
            got = pa.Array.from_buffers(pa.string(), m, [None, pa.py_buffer(got_offsets.tobytes()),
                                                         pa.py_buffer(out_data[: int(got_offsets[-1])].cpu().numpy().tobytes())])
            want = pc.utf8_rtrim(harr, " ") if label.startswith("utf8_rtrim") else getattr(pc, label)(harr)
            assert got.equals(want), f"({kind}) {label} differs from pyarrow's"
        del offsets, data, out_offsets, out_data, indices, ws
        torch.cuda.empty_cache()
        emit()
    emit("# the first 2^18 rows of every timed trim equal pyarrow's")
    emit(f"# lines outside a bound: {'; '.join(missed) if missed else 'none'}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
