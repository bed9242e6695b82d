"""Times arx_temporal_component (csrc/temporal.hip) on columns generated on the device, against two yardsticks on the
same buffers: the cast int32 -> int64 for the 4-byte inputs, `add` of an int64 column and a scalar for the 8-byte ones.

One line per function x {date32, timestamp[us], timestamp[s], time64[ns]} where the reference has the pair: 2^--log2-rows
rows, 10 % nulls, GB/s over the algorithmic bytes (input width + 8 + 2/8 a row).  A component may take its yardstick's
time x 1.05 (the yardsticks move the same value bytes and no bitmap).  Median of --reps device-event timings around the
C-ABI call.  pyarrow's pc.year(timestamp[us]) on one host thread at 2^--host-log2-rows rows is recorded for scale, and the
device result of the same rows is checked against it.  --lib times another build of the library (the A/B of DESIGN.md
4.20).  Writes the table to --out.

    python scripts/exp_temporal.py [--log2-rows 28] [--reps 10] [--host-log2-rows 26] [--lib PATH] [--out profiles/temporal.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12     # HBM3E peak, bytes / s
CALENDAR = ["year", "quarter", "month", "day", "day_of_week", "day_of_year", "iso_year", "iso_week"]
TIME_OF_DAY = ["hour", "minute", "second", "millisecond", "microsecond", "nanosecond"]
COMPONENT = {name: i for i, name in enumerate(CALENDAR + TIME_OF_DAY)}
# name -> (ARX_TIME_*, bytes a value)
INPUTS = {"date32": (0, 4), "timestamp[us]": (4, 8), "timestamp[s]": (2, 8), "time64[ns]": (9, 8)}
DAY_MIN, DAY_MAX = -719162, 2932896          # 0001-01-01 .. 9999-12-31
ARX_NUM_INT32, ARX_NUM_INT64, ARX_ARITH_ADD = 4, 6, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-log2-rows", type=int, default=26)
    ap.add_argument("--lib", default=None, help="another build of libarrow_amd.so to time instead of the tree's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal.txt"))
    a = ap.parse_args()
    assert a.reps >= 10, "median of at least 10"
    import pyarrow as pa
    import pyarrow.compute as pc
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import current_stream

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load(a.lib) if a.lib else _lib.get_lib()
    stream = current_stream(dev)
    n = 1 << a.log2_rows
    words = n // 64
    gen = torch.Generator(device=dev).manual_seed(53)
    weights = (1 << torch.arange(8, device=dev, dtype=torch.int32)).to(torch.uint8)
    step = 1 << 26

    def bitmap(p_set):
        out = torch.empty(n // 8, dtype=torch.uint8, device=dev)
        for lo in range(0, n, step):
            bits = torch.rand(min(step, n - lo), device=dev, generator=gen) < p_set
            out[lo // 8:(lo + step) // 8] = (bits.view(-1, 8).to(torch.uint8) * weights).sum(1, dtype=torch.uint8)
        return out

    def randint(lo, hi, scale=1, plus=0):
        """n int64 values: uniform in [lo, hi] times scale, plus uniform in [0, plus)."""
        out = torch.empty(n, dtype=torch.int64, device=dev)
        for at in range(0, n, step):
            m = min(step, n - at)
            v = torch.randint(lo, hi + 1, (m,), dtype=torch.int64, device=dev, generator=gen) * scale
            if plus:
                v += torch.randint(0, plus, (m,), dtype=torch.int64, device=dev, generator=gen)
            out[at:at + m] = v
        return out

    columns = {"date32": randint(DAY_MIN, DAY_MAX).to(torch.int32),
               "timestamp[us]": randint(DAY_MIN, DAY_MAX, 86_400_000_000, 86_400_000_000),
               "timestamp[s]": randint(DAY_MIN, DAY_MAX, 86_400, 86_400),
               "time64[ns]": randint(0, 86_400_000_000_000 - 1)}
    valid = bitmap(0.9)
    out = torch.empty(n * 8 + 64, dtype=torch.uint8, device=dev)
    out_valid = torch.empty(words * 8 + 64, dtype=torch.uint8, device=dev)
    seven = C.c_int64(7)

    def timed(call):
        times = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = call()
            e1.record()
            assert rc == 0, lib.arx_last_error()
            e1.synchronize()
            if i >= 3:
                times.append(e0.elapsed_time(e1))
        return float(np.median(times)), min(times), max(times)

    def component(fn, name):
        span = _lib.ArxSpan(valid.data_ptr(), columns[name].data_ptr(), 0, n, -1)
        return timed(lambda: lib.arx_temporal_component(COMPONENT[fn], INPUTS[name][0], C.byref(span), n, 1, 1, out.data_ptr(),
                                                        out_valid.data_ptr(), stream))

    def yardstick(name):
        data = columns[name]
        if INPUTS[name][1] == 4:
            span = _lib.ArxSpan(None, data.data_ptr(), 0, n, 0)
            return timed(lambda: lib.arx_cast_numeric(C.byref(span), ARX_NUM_INT32, ARX_NUM_INT64, 1, 1, None, 0, out.data_ptr(), stream))
        return timed(lambda: lib.arx_arith_numeric(ARX_ARITH_ADD, 0, ARX_NUM_INT64, data.data_ptr(), None, None, 0, None,
                                                   C.cast(C.pointer(seven), C.c_void_p), None, 0, n, out.data_ptr(), None, stream))

    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def row(label, name, t, nbytes, extra=""):
        ms, lo, hi = t
        emit(f"{label:<14} {name:<14} {ms:>9.3f} {lo:>9.3f} {hi:>9.3f} {nbytes / ms / 1e6:>9.1f} {nbytes / (ms * 1e-3) / PEAK:>8.3f} {extra}")

    emit(f"# arx_temporal_component, {torch.cuda.get_device_name(0)}, 2^{a.log2_rows} rows, 10 % nulls"
         + (f"; library {os.path.basename(a.lib)}" if a.lib else ""))
    emit(f"# ms: median / min / max of {a.reps} after 3 warm-up calls, device events around the C-ABI call; GB/s over the algorithmic "
         "bytes (input width + 8 + 2/8 a row; the yardsticks: input width + 8); peak 8 TB/s")
    emit(f"{'function':<14} {'input':<14} {'ms':>9} {'min':>9} {'max':>9} {'GB/s':>9} {'of peak':>8}")
    missed = []
    for name, (_, width) in INPUTS.items():
        ty = yardstick(name)
        bound = ty[0] * 1.05
        row("cast int32->int64" if width == 4 else "add int64+scalar", name, ty, n * (width + 8), f"yardstick: bound {bound:.3f} ms")
        for fn in (CALENDAR if name != "time64[ns]" else []) + (TIME_OF_DAY if name != "date32" else []):
            t = component(fn, name)
            ok = t[0] <= bound
            if not ok:
                missed.append(f"{fn}({name}) {t[0]:.3f} > {bound:.3f}")
            row(fn, name, t, n * (width + 8 + 2 / 8), "within the bound" if ok else "MISSES the bound")
        emit()
    emit(f"# lines that miss their bound: {'; '.join(missed) if missed else 'none'}")
    # ---- the reference on one host thread, and the device result against it
    m = min(n, 1 << a.host_log2_rows)
    pa.set_cpu_count(1)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    harr = pa.Array.from_buffers(pa.timestamp("us"), m, [pa.py_buffer(host(valid[: m // 8]).tobytes()),
                                                         pa.py_buffer(host(columns["timestamp[us]"][:m]).tobytes())])
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = pc.year(harr)
        ts.append(time.perf_counter() - t0)
    component("year", "timestamp[us]")
    torch.cuda.synchronize()
    got = pa.Array.from_buffers(pa.int64(), m, [pa.py_buffer(host(out_valid[: m // 8]).tobytes()), pa.py_buffer(host(out[: m * 8]).tobytes())])
    assert got.equals(want) and got.null_count == want.null_count, "the device result differs from pyarrow's"
    host_ms = 1e3 * float(np.median(ts))
    emit(f"# pyarrow {pa.__version__} pc.year(timestamp[us]) on one host thread, 2^{a.host_log2_rows} rows: {host_ms:.1f} ms "
         f"({m * (16 + 2 / 8) / host_ms / 1e6:.2f} GB/s); the device result of the same rows equals it")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
