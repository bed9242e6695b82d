"""Times arx_case_when (csrc/case_when.hip) and arx_min_max_element_wise (csrc/element_wise.hip) on columns generated on the
device, each against a yardstick that is not the code under test, in the same run on the same buffers.

Every operand has 10 % nulls; every cond is random at p = 0.5.  Per case: warm-up 3, median of --reps (>= 10) device-event
timings around the C-ABI call(s); GB/s over the algorithmic bytes; the fraction of the 8 TB/s peak.
  * case_when, one cond + else, widths 1 / 2 / 4 / 8 / 16 and boolean, against arx_if_else on the same operands (the same
    algorithmic bytes, 3 W + 5/8 a row): case_when may take if_else_time x 1.05.
  * case_when, four conds + else, width 8, against the chain of four nested arx_if_else calls that computes the same
    column (its conds are the case_when's with their null slots cleared, made outside the timed region; the two results
    are compared): it must be faster.  Bytes as if every stream were read whole: 5 W + 4 x 2/8 + 5/8 in, W + 1/8 out.
  * min / max, two array operands, widths 4 and 8, against the two-operand add of scalar.hip on the same buffers (two
    streams in, one out): min / max may take add_time x 1.05.  Also five operands at width 8.
  * pyarrow on one host thread at 2^--host-log2-rows rows: pc.case_when with four conds and pc.max_element_wise of two
    operands at width 8; the device results of the same rows must equal them.
Writes the table to --out.

    python scripts/exp_case_when.py [--log2-rows 28] [--reps 10] [--host-log2-rows 26] [--out profiles/case_when.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "case_when.txt"))
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
    n = 1 << a.log2_rows
    words = n // 64
    gen = torch.Generator(device=dev).manual_seed(53)
    weights = (1 << torch.arange(8, device=dev, dtype=torch.int32)).to(torch.uint8)

    def pack(bits):
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

    conds = [bitmap(0.5) for _ in range(4)]
    cond_valid = [bitmap(0.9) for _ in range(4)]
    conds_cleared = [c & v for c, v in zip(conds, cond_valid)]      # (for the if_else chain: a null cond is false)
    left, right = random_bytes(n * 16), random_bytes(n * 16)
    # five width-8 streams: the halves of the two 16-byte buffers and one more
    streams8 = [left[: n * 8], left[n * 8:], right[: n * 8], right[n * 8:], random_bytes(n * 8)]
    valid = [bitmap(0.9) for _ in range(5)]
    out = torch.empty(n * 16 + 64, dtype=torch.uint8, device=dev)
    out_valid = torch.empty(words * 8 + 64, dtype=torch.uint8, device=dev)
    tmp = [torch.empty(n * 8, dtype=torch.uint8, device=dev) for _ in range(2)]
    tmp_valid = [torch.empty(words * 8, dtype=torch.uint8, device=dev) for _ in range(2)]
    chain_out = torch.empty(n * 8, dtype=torch.uint8, device=dev)
    chain_valid = torch.empty(words * 8, dtype=torch.uint8, device=dev)

    def span(data, validity):
        return _lib.ArxSpan(validity.data_ptr() if validity is not None else None, data.data_ptr(), 0, n, -1 if validity is not None else 0)

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

    keep = []

    def case_when_call(width, cond_spans, value_spans, o=out, ov=out_valid):
        ctable = (C.POINTER(_lib.ArxSpan) * len(cond_spans))(*[C.pointer(s) for s in cond_spans])
        vtable = (_lib.ArxOperand * len(value_spans))()
        for j, s in enumerate(value_spans):
            vtable[j].span = C.pointer(s)
        keep.extend([cond_spans, value_spans, ctable, vtable])
        return lambda: lib.arx_case_when(width, ctable, len(cond_spans), vtable, len(value_spans), n, o.data_ptr(), ov.data_ptr(), stream)

    def if_else_call(width, cond, l, r, o=out, ov=out_valid):
        keep.extend([cond, l, r])
        return lambda: lib.arx_if_else(width, C.byref(cond), C.byref(l), None, C.byref(r), None, n, o.data_ptr(), ov.data_ptr(), stream)

    def min_max_call(num_type, op, spans):
        table = (_lib.ArxOperand * len(spans))()
        for j, s in enumerate(spans):
            table[j].span = C.pointer(s)
        keep.extend([spans, table])
        return lambda: lib.arx_min_max_element_wise(num_type, op, 1, table, len(spans), n, out.data_ptr(), out_valid.data_ptr(), stream)

    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def row(label, width, t, nbytes, extra=""):
        ms, lo, hi = t
        emit(f"{label:<34} {width:>5} {ms:>9.3f} {lo:>9.3f} {hi:>9.3f} {nbytes / ms / 1e6:>9.1f} {nbytes / (ms * 1e-3) / PEAK:>8.3f} {extra}")

    emit(f"# arx_case_when / arx_min_max_element_wise, {torch.cuda.get_device_name(0)}, 2^{a.log2_rows} rows, 10 % nulls in every operand, "
         "conds random at p = 0.5")
    emit(f"# ms: median / min / max of {a.reps} after 3 warm-up calls, device events around the C-ABI call(s); GB/s over the algorithmic "
         "bytes; peak 8 TB/s")
    emit(f"{'case':<34} {'width':>5} {'ms':>9} {'min':>9} {'max':>9} {'GB/s':>9} {'of peak':>8}")
    missed = []
    # ---- one cond + else against if_else
    for width in (1, 2, 4, 8, 16, 0):
        w = width if width else 0.125
        name = "bool" if width == 0 else str(width)
        cs, ls, rs = span(conds[0], cond_valid[0]), span(left, valid[0]), span(right, valid[1])
        t = timed(case_when_call(width, [cs], [ls, rs]))
        ti = timed(if_else_call(width, cs, ls, rs))
        bound = ti[0] * 1.05
        ok = t[0] <= bound
        if not ok:
            missed.append(f"case_when 1 cond width {name}")
        row("case_when 1 cond + else", name, t, n * (3 * w + 5 / 8))
        row("if_else array/array", name, ti, n * (3 * w + 5 / 8), f"bound {bound:.3f} ms: case_when {'within' if ok else 'MISSES'} it")
    emit()
    # ---- four conds + else, width 8, against the chain of four nested if_else calls
    cspans = [span(conds[j], cond_valid[j]) for j in range(4)]
    vspans = [span(streams8[j], valid[j]) for j in range(5)]
    four = case_when_call(8, cspans, vspans)
    t4 = timed(four)
    cleared = [span(conds_cleared[j], None) for j in range(4)]
    t3s, t2s, t1s = span(tmp[0], tmp_valid[0]), span(tmp[1], tmp_valid[1]), span(tmp[0], tmp_valid[0])
    steps = [if_else_call(8, cleared[3], vspans[3], vspans[4], tmp[0], tmp_valid[0]),
             if_else_call(8, cleared[2], vspans[2], t3s, tmp[1], tmp_valid[1]),
             if_else_call(8, cleared[1], vspans[1], t2s, tmp[0], tmp_valid[0]),
             if_else_call(8, cleared[0], vspans[0], t1s, chain_out, chain_valid)]

    def chain():
        for s in steps:
            rc = s()
            if rc != 0:
                return rc
        return 0

    tc = timed(chain)
    assert four() == 0 and chain() == 0
    torch.cuda.synchronize()
    assert torch.equal(out[: n * 8], chain_out) and torch.equal(out_valid[: words * 8], chain_valid), "case_when and the if_else chain differ"
    bytes4 = n * (5 * 8 + 4 * 2 / 8 + 5 / 8 + 8 + 1 / 8)
    faster = t4[0] < tc[0]
    if not faster:
        missed.append("case_when 4 conds against the if_else chain")
    row("case_when 4 conds + else", "8", t4, bytes4, f"{tc[0] / t4[0]:.2f} x the chain's speed: {'faster' if faster else 'NOT FASTER'}")
    row("4 nested if_else calls", "8", tc, bytes4, "(the same column; bytes as for case_when: its intermediates are not counted)")
    emit()
    # ---- min / max of two arrays against add
    for width, num_type in ((4, 4), (8, 6)):       # ARX_NUM_INT32, ARX_NUM_INT64
        ls, rs = span(left, valid[0]), span(right, valid[1])
        for op, opname in ((0, "min"), (1, "max")):
            t = timed(min_max_call(num_type, op, [ls, rs]))
            if op == 0:
                ta = timed(lambda: lib.arx_arith_numeric(0, 0, num_type, left.data_ptr(), None, None, 0, right.data_ptr(), None, None, 0, n,
                                                         out.data_ptr(), None, stream))
                bound = ta[0] * 1.05
            ok = t[0] <= bound
            if not ok:
                missed.append(f"{opname} width {width}")
            row(f"{opname}_element_wise 2 arrays", str(width), t, n * (3 * width + 3 / 8), f"bound {bound:.3f} ms: {'within' if ok else 'MISSES'} it")
        row("add 2 arrays (values only)", str(width), ta, n * 3 * width)
    t5 = timed(min_max_call(6, 1, [span(streams8[j], valid[j]) for j in range(5)]))
    row("max_element_wise 5 arrays", "8", t5, n * (6 * 8 + 6 / 8))
    emit(f"# bounds missed: {'; '.join(missed) if missed else 'none'}")
    # ---- the reference on one host thread, and the device results against it
    m = min(n, 1 << a.host_log2_rows)
    pa.set_cpu_count(1)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    harr = lambda typ, data, v, nbytes: pa.Array.from_buffers(typ, m, [pa.py_buffer(host(v[: m // 8]).tobytes()),  # noqa: E731
                                                                       pa.py_buffer(host(data[:nbytes]).tobytes())])
    hconds = [harr(pa.bool_(), conds[j], cond_valid[j], m // 8) for j in range(4)]
    hvals = [harr(pa.int64(), streams8[j], valid[j], m * 8) for j in range(5)]
    struct = pa.StructArray.from_arrays(hconds, ["a", "b", "c", "d"])

    def host_ms(f):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = f()
            ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts)), res

    cw_ms, want_cw = host_ms(lambda: pc.case_when(struct, *hvals))
    mx_ms, want_mx = host_ms(lambda: pc.max_element_wise(hvals[0], hvals[1]))
    device = lambda: pa.Array.from_buffers(pa.int64(), m, [pa.py_buffer(host(out_valid[: m // 8]).tobytes()),  # noqa: E731
                                                           pa.py_buffer(host(out[: m * 8]).tobytes())])
    assert four() == 0
    torch.cuda.synchronize()
    got = device()
    assert got.equals(want_cw) and got.null_count == want_cw.null_count, "the device case_when differs from pyarrow's"
    assert min_max_call(6, 1, [span(streams8[0], valid[0]), span(streams8[1], valid[1])])() == 0
    torch.cuda.synchronize()
    got = device()
    assert got.equals(want_mx) and got.null_count == want_mx.null_count, "the device max_element_wise differs from pyarrow's"
    emit(f"# pyarrow {pa.__version__} on one host thread, width 8, 2^{a.host_log2_rows} rows: pc.case_when of four conds and an else "
         f"{cw_ms:.1f} ms, pc.max_element_wise of two operands {mx_ms:.1f} ms; the device results of the same rows equal them")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
