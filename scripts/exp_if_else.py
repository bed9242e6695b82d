"""Times arx_if_else (csrc/if_else.hip) on columns generated on the device, against arx_coalesce2 on the same buffers.

Every operand has 10 % nulls; cond is random at p = 0.5.  Per width 1, 2, 4, 8, 16 and boolean, array / array operands:
time, algorithmic GB/s (two value streams in, one out, cond's bits, three validity bitmaps in, one out: 3 W + 5/8 bytes
a row) and the fraction of the 8 TB/s peak.  At width 8 also array / scalar and a clustered cond (runs of 4096 equal
values).  The yardstick is arx_coalesce2 with an array fill at the widths it has (3 W + 3/8 bytes a row): arx_if_else may
take coalesce2_time x (3 W + 5/8) / (3 W + 3/8) x 1.05.  Per case: warm-up 3, median of --reps (>= 10) device-event
timings around the C-ABI call.  pyarrow's pc.if_else on one host thread at 2^--host-log2-rows rows of the width-8 columns
gives the baseline, and its result must equal the device's.  --lib times another build of the library (the A/B of
-DARX_IF_ELSE_SKIP).  Writes the table to --out.

    python scripts/exp_if_else.py [--log2-rows 28] [--reps 10] [--host-log2-rows 26] [--lib PATH] [--out profiles/if_else.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-log2-rows", type=int, default=26)
    ap.add_argument("--lib", default=None, help="another build of libarrow_amd.so to time instead of the tree's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "if_else.txt"))
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
    gen = torch.Generator(device=dev).manual_seed(47)
    weights = (1 << torch.arange(8, device=dev, dtype=torch.int32)).to(torch.uint8)

    def pack(bits):
        """A bool tensor of n rows -> its LSB-first bitmap (n / 8 bytes)."""
        return (bits.view(-1, 8).to(torch.uint8) * weights).sum(1, dtype=torch.uint8)

    def bitmap(p_set):
        out = torch.empty(n // 8, dtype=torch.uint8, device=dev)
        step = 1 << 26
        for lo in range(0, n, step):
            out[lo // 8:(lo + step) // 8] = pack(torch.rand(min(step, n - lo), device=dev, generator=gen) < p_set)
        return out

    def random_bytes(nbytes):
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        step = 1 << 28
        for lo in range(0, nbytes, step):
            out[lo:lo + step] = torch.randint(0, 256, (min(step, nbytes - lo),), dtype=torch.uint8, device=dev, generator=gen)
        return out

    cond_random = bitmap(0.5)
    runs = torch.rand(n // 4096, device=dev, generator=gen) < 0.5            # a partitioned column: runs of 4096 equal values
    cond_clustered = pack(runs.repeat_interleave(4096))
    cv, lv, rv = bitmap(0.9), bitmap(0.9), bitmap(0.9)
    left, right = random_bytes(n * 16), random_bytes(n * 16)
    out = torch.empty(n * 16 + 64, dtype=torch.uint8, device=dev)
    out_valid = torch.empty(words * 8 + 64, dtype=torch.uint8, device=dev)
    scalar = (C.c_uint8 * 16)(*range(1, 17))

    def span(data, validity):
        return _lib.ArxSpan(validity.data_ptr(), data.data_ptr(), 0, n, -1)

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

    def if_else(width, cond, right_scalar=False):
        cs, ls, rs = span(cond, cv), span(left, lv), span(right, rv)
        return timed(lambda: lib.arx_if_else(width, C.byref(cs), C.byref(ls), None, None if right_scalar else C.byref(rs),
                                             C.cast(scalar, C.c_void_p) if right_scalar else None, n, out.data_ptr(),
                                             out_valid.data_ptr(), stream))

    def coalesce(width):
        ls, rs = span(left, lv), span(right, rv)
        return timed(lambda: lib.arx_coalesce2(width, C.byref(ls), C.byref(rs), None, n, out.data_ptr(), out_valid.data_ptr(), stream))

    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def row(label, width, t, nbytes, extra=""):
        ms, lo, hi = t
        emit(f"{label:<28} {width:>5} {ms:>9.3f} {lo:>9.3f} {hi:>9.3f} {nbytes / ms / 1e6:>9.1f} {nbytes / (ms * 1e-3) / PEAK:>8.3f} {extra}")

    emit(f"# arx_if_else, {torch.cuda.get_device_name(0)}, 2^{a.log2_rows} rows, 10 % nulls in every operand, cond random at p = 0.5"
         + (f"; library {os.path.basename(a.lib)}" if a.lib else ""))
    emit(f"# ms: median / min / max of {a.reps} after 3 warm-up calls, device events around the C-ABI call; GB/s over the algorithmic "
         "bytes (if_else 3 W + 5/8 a row, coalesce2 3 W + 3/8); peak 8 TB/s")
    emit(f"{'case':<28} {'width':>5} {'ms':>9} {'min':>9} {'max':>9} {'GB/s':>9} {'of peak':>8}")
    missed = []
    for width in (1, 2, 4, 8, 16, 0):
        w = width if width else 0.125
        name = "bool" if width == 0 else str(width)
        t = if_else(width, cond_random)
        row("if_else array/array", name, t, n * (3 * w + 5 / 8))
        if width != 16:
            tc = coalesce(width)
            bound = tc[0] * (3 * w + 5 / 8) / (3 * w + 3 / 8) * 1.05
            ok = t[0] <= bound
            if not ok:
                missed.append(name)
            row("coalesce2 array fill", name, tc, n * (3 * w + 3 / 8), f"bound {bound:.3f} ms: if_else {'within' if ok else 'MISSES'} it")
    emit()
    row("if_else array/scalar", "8", if_else(8, cond_random, right_scalar=True), n * (2 * 8 + 4 / 8))
    row("if_else clustered cond 4096", "8", if_else(8, cond_clustered), n * (3 * 8 + 5 / 8),
        "(bytes as if both sides were read: a run reads one)")
    emit(f"# widths that miss the bound: {', '.join(missed) if missed else 'none'}")
    # ---- the reference on one host thread, and the device result against it
    m = min(n, 1 << a.host_log2_rows)
    pa.set_cpu_count(1)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    harr = lambda typ, data, valid, nbytes: pa.Array.from_buffers(typ, m, [pa.py_buffer(host(valid[: m // 8]).tobytes()),  # noqa: E731
                                                                           pa.py_buffer(host(data[:nbytes]).tobytes())])
    hc, hl, hr = harr(pa.bool_(), cond_random, cv, m // 8), harr(pa.uint64(), left, lv, m * 8), harr(pa.uint64(), right, rv, m * 8)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = pc.if_else(hc, hl, hr)
        ts.append(time.perf_counter() - t0)
    if_else(8, cond_random)
    torch.cuda.synchronize()
    got = pa.Array.from_buffers(pa.uint64(), m, [pa.py_buffer(host(out_valid[: m // 8]).tobytes()), pa.py_buffer(host(out[: m * 8]).tobytes())])
    assert got.equals(want) and got.null_count == want.null_count, "the device result differs from pyarrow's"
    host_ms = 1e3 * float(np.median(ts))
    emit(f"# pyarrow {pa.__version__} pc.if_else on one host thread, width 8, 2^{a.host_log2_rows} rows: {host_ms:.1f} ms "
         f"({m * (3 * 8 + 5 / 8) / host_ms / 1e6:.2f} GB/s); the device result of the same rows equals it")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
