"""Times arx_unary_numeric / arx_round_numeric (csrc/unary_arith.hip) on columns generated on the device against one
yardstick per element type: arx_arith_numeric `multiply` of the same column by a scalar, which reads and writes the same
bytes and is no part of that file.

One line per kernel: 2^--log2-rows rows, no validity (these kernels read the bitmap only for a failing row), device events
around the C-ABI call.  Every shape is warmed up first; then --reps rounds, each timing the yardstick and the kernel one
after the other (alternating), so that both see the same clocks.  Recorded: the kernel's median, the yardstick's median,
their ratio, and the yardstick's own min - max spread relative to its median — a kernel whose ratio lies outside that
spread is slower (or faster) than the yardstick by more than the yardstick differs from itself.  Writes the table to --out.

    python scripts/exp_unary_arith.py [--log2-rows 26] [--reps 10] [--out profiles/unary_arith.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12     # HBM3E peak, bytes / s
ARX_ARITH_MULTIPLY = 2
INT64, FLOAT32, FLOAT64 = 6, 8, 9
NEGATE, ABS, FLOOR = 0, 1, 3
DIGITS, MULTIPLE = 0, 1
HALF_TO_EVEN = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unary_arith.txt"))
    a = ap.parse_args()
    assert a.reps >= 10, "at least 10 alternating repeats"
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import current_stream

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.get_lib()
    stream = current_stream(dev)
    n = 1 << a.log2_rows
    gen = torch.Generator(device=dev).manual_seed(59)
    columns = {INT64: torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device=dev, generator=gen),
               FLOAT64: torch.randn(n, dtype=torch.float64, device=dev, generator=gen) * 1e3,
               FLOAT32: torch.randn(n, dtype=torch.float32, device=dev, generator=gen) * 1e3}
    width = {INT64: 8, FLOAT64: 8, FLOAT32: 4}
    names = {INT64: "int64", FLOAT64: "double", FLOAT32: "float"}
    scalars = {INT64: np.array([3], np.int64), FLOAT64: np.array([1.0009765625], np.float64), FLOAT32: np.array([1.0009765625], np.float32)}
    out = torch.empty(n * 8 + 64, dtype=torch.uint8, device=dev)
    errors = torch.zeros(1, dtype=torch.int64, device=dev)
    half = np.array([0.5], np.float64)

    def span(t):
        return _lib.ArxSpan(None, columns[t].data_ptr(), 0, n, 0)

    def yardstick(t):
        return lambda: lib.arx_arith_numeric(ARX_ARITH_MULTIPLY, 0, t, columns[t].data_ptr(), None, None, 0, None, scalars[t].ctypes.data,
                                             None, 0, n, out.data_ptr(), None, stream)

    def unary(op, checked, t):
        s = span(t)
        return lambda: lib.arx_unary_numeric(op, checked, t, C.byref(s), out.data_ptr(), errors.data_ptr(), stream)

    def rounding(kind, t, ndigits, multiple=None):
        s = span(t)
        return lambda: lib.arx_round_numeric(kind, HALF_TO_EVEN, t, C.byref(s), ndigits, None if multiple is None else multiple.ctypes.data,
                                             out.data_ptr(), errors.data_ptr(), stream)

    kernels = [("negate", INT64, unary(NEGATE, 0, INT64)), ("abs_checked", INT64, unary(ABS, 1, INT64)), ("floor", FLOAT64, unary(FLOOR, 0, FLOAT64)),
               ("round(ndigits=2)", FLOAT64, rounding(DIGITS, FLOAT64, 2)), ("round(ndigits=2)", FLOAT32, rounding(DIGITS, FLOAT32, 2)),
               ("round(ndigits=-2)", INT64, rounding(DIGITS, INT64, -2)),
               ("round_to_multiple(0.5)", FLOAT64, rounding(MULTIPLE, FLOAT64, 0, half))]

    def once(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = call()
        e1.record()
        assert rc == 0, lib.arx_last_error()
        e1.synchronize()
        return e0.elapsed_time(e1)

    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"# csrc/unary_arith.hip against arx_arith_numeric multiply-by-a-scalar of the same type, {torch.cuda.get_device_name(0)}, "
         f"2^{a.log2_rows} rows, no nulls")
    emit(f"# 3 warm-up calls of each, then {a.reps} rounds of (yardstick, kernel) one after the other; device events around the C-ABI call; "
         "ms are medians; GB/s over input + output bytes; peak 8 TB/s")
    emit(f"{'kernel':<24} {'type':<7} {'ms':>8} {'GB/s':>8} {'of peak':>8} {'yardstick ms':>13} {'min':>8} {'max':>8} {'spread':>8} {'ratio':>7}  verdict")
    outside = []
    for label, t, call in kernels:
        yard = yardstick(t)
        for _ in range(3):
            once(yard)
            once(call)
        ty, tk = [], []
        for _ in range(a.reps):
            ty.append(once(yard))
            tk.append(once(call))
        my, mk = float(np.median(ty)), float(np.median(tk))
        spread = (max(ty) - min(ty)) / my
        ratio = mk / my
        inside = abs(ratio - 1.0) <= spread
        if not inside:
            outside.append(f"{label} {names[t]} x{ratio:.3f}")
        nbytes = 2 * n * width[t]
        emit(f"{label:<24} {names[t]:<7} {mk:>8.4f} {nbytes / mk / 1e6:>8.1f} {nbytes / (mk * 1e-3) / PEAK:>8.3f} {my:>13.4f} {min(ty):>8.4f} "
             f"{max(ty):>8.4f} {spread:>8.3f} {ratio:>7.3f}  {'inside the spread' if inside else 'OUTSIDE the spread'}")
    torch.cuda.synchronize()
    assert int(errors.cpu()[0]) == 0, "a row of the timed columns failed"
    emit(f"# outside the yardstick's spread: {'; '.join(outside) if outside else 'none'}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
