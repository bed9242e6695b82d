"""Times arx_match_substring's two kernels (csrc/match_substring.hip) apart: the rows kernel (one lane per row) and the
bytes kernel (the lanes walk the bytes, hits are resolved to rows), on binary columns generated on the device:

    short   rows of 0 .. 32 bytes (mean 16)
    long    rows of 512 .. 1536 bytes (mean 1 KiB)
    skewed  99 % rows of 0 .. 32 bytes, 1 % of the rows 1 MiB each (the bytes are almost all theirs)

bytes drawn from 'a' .. 'z', against a rare pattern ("wxyz": one start position in 26^4) and a frequent one ("e": one in
26), plus a sweep of the mean row size at a fixed number of bytes with the rare pattern — the crossover of the two
kernels is where kBytesPathMeanRow belongs.  Per case: warm-up 3, median of --reps (>= 10) device-event timings around
the C-ABI call; rows/s and GB/s over data + offsets + output bytes.  The installed pyarrow on one thread on the host
copy of the same column gives the baseline, and its result must equal both kernels' bits.  Writes the table to --out.

    python scripts/exp_match_substring.py [--log2-bytes 29] [--reps 10] [--host-reps 3] [--out profiles/match_substring.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bytes", type=int, default=29, help="data bytes of each column")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_substring.txt"))
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
    total = 1 << a.log2_bytes
    gen = torch.Generator(device=dev).manual_seed(31)

    def column(lengths):
        """int32 offsets and random 'a' .. 'z' bytes of a column with these row lengths (a device int64 tensor)."""
        offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lengths, 0, out=offsets[1:])
        nbytes = int(offsets[-1])
        assert nbytes < 2**31
        data = torch.randint(97, 123, (nbytes + 64,), dtype=torch.uint8, device=dev, generator=gen)
        return offsets.to(torch.int32), data, nbytes

    def uniform(n, lo, hi):
        return torch.randint(lo, hi + 1, (n,), dtype=torch.int64, device=dev, generator=gen)

    def skewed():
        n_long = max(1, (total - (total >> 3)) >> 20)
        n = 100 * n_long
        lengths = uniform(n, 0, 32)
        lengths[torch.randperm(n, device=dev, generator=gen)[:n_long]] = 1 << 20
        return lengths

    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def run(name, lengths, patterns, host):
        offsets, data, nbytes = column(lengths)
        n = len(lengths)
        words = (n + 63) // 64
        out = torch.empty(words * 8 + 8, dtype=torch.uint8, device=dev)
        span = _lib.ArxBinarySpan(None, offsets.data_ptr(), data.data_ptr(), 0, n, 0)
        moved = nbytes + (n + 1) * 4 + words * 8
        harr = None
        if host:
            harr = pa.Array.from_buffers(pa.binary(), n, [None, pa.py_buffer(offsets.cpu().numpy().tobytes()),
                                                          pa.py_buffer(data[:nbytes].cpu().numpy().tobytes())])
        res = {}
        for pat in patterns:
            dpat = torch.frombuffer(bytearray(pat), dtype=torch.uint8).to(dev)
            want, host_ms = None, float("nan")
            if host:
                ts = []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    want = pc.match_substring(harr, pat)
                    ts.append(time.perf_counter() - t0)
                host_ms = 1e3 * float(np.median(ts))
                want = np.packbits(want.to_numpy(zero_copy_only=False), bitorder="little")
            for path, label in ((1, "rows"), (2, "bytes")):
                times = []
                for i in range(3 + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rc = lib.arx_match_substring(C.byref(span), 4, 0, dpat.data_ptr(), len(pat), nbytes, path, out.data_ptr(), stream)
                    e1.record()
                    assert rc == 0, lib.arx_last_error()
                    e1.synchronize()
                    if i >= 3:
                        times.append(e0.elapsed_time(e1))
                ms = float(np.median(times))
                if want is not None:
                    got = out[: len(want)].cpu().numpy()
                    assert (got == want).all(), (name, pat, label)
                hits = int(np.unpackbits(out[: words * 8].cpu().numpy(), bitorder="little")[:n].sum())
                res[pat, label] = ms
                emit(f"{name:<12} {n:>10} {nbytes / n:>9.1f} {pat.decode():<6} {label:<6} {ms:>9.3f} {min(times):>9.3f} {max(times):>9.3f} "
                     f"{n / ms / 1e6:>10.2f} {moved / ms / 1e6:>9.1f} {hits / n:>8.4f} {host_ms:>10.1f} {moved / host_ms / 1e6 if host else float('nan'):>8.2f}")
        del offsets, data, out
        torch.cuda.empty_cache()
        return res

    emit(f"# arx_match_substring, op match_substring, {torch.cuda.get_device_name(0)}; pyarrow {pa.__version__} on one host thread")
    emit(f"# device ms: median / min / max of {a.reps} after 3 warm-up calls, device events around the C-ABI call; GB/s over data + offsets + output")
    emit(f"{'column':<12} {'rows':>10} {'mean B':>9} {'pat':<6} {'path':<6} {'ms':>9} {'min':>9} {'max':>9} {'Mrows/s':>10} {'GB/s':>9} "
         f"{'hit rate':>8} {'host ms':>10} {'host GB/s':>8}")
    pa.set_cpu_count(1)
    rare, frequent = b"wxyz", b"e"
    run("short", uniform(total // 16, 0, 32), (rare, frequent), True)
    run("long", uniform(total // 1024, 512, 1536), (rare, frequent), True)
    run("skewed", skewed(), (rare, frequent), True)
    emit()
    emit(f"# sweep of the mean row size, {total >> 2} data bytes, pattern {rare.decode()!r}: where the bytes kernel overtakes the rows kernel")
    crossover = None
    for mean in (8, 16, 32, 64, 128, 256, 512, 1024, 4096):
        r = run(f"mean{mean}", uniform((total >> 2) // mean, mean // 2, mean + mean // 2), (rare,), False)
        if crossover is None and r[rare, "bytes"] < r[rare, "rows"]:
            crossover = mean
    emit(f"# first mean row size at which the bytes kernel is faster: {crossover}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
