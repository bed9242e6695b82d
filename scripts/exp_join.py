"""Times the full-size inner join: 2^27 int64 probe rows against 2^24 build rows, a quarter of the build keys
duplicated (the keys of tests/test_hash_join.py::test_gpu_hash_join_full_size).  Device route: the mirror,
compute.hash_join_indices (Grouper consume / lookup, csrc/hash_join.hip, the stable sort of the build ids).
Baseline: pa.Table.join of the same keys on the host, on up to 16 CPU threads.  A second leg adds a residual filter that
passes about half the pairs (left row number + right row number even; left outer, so the count, compact, unmatched-row
and validity kernels all run); the predicate's element-wise calls are timed apart.  Prints one JSON line.

    python scripts/exp_join.py [--log2-probe 27] [--log2-build 24] [--reps 5] [--host-reps 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-probe", type=int, default=27)
    ap.add_argument("--log2-build", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    import pyarrow as pa
    import torch

    import arrow_amd as amd

    rng = np.random.default_rng(27)
    nb, nl = 1 << a.log2_build, 1 << a.log2_probe
    nd = nb - nb // 4
    distinct = (np.arange(nd, dtype=np.int64) * 0x9E3779B1) & ((1 << 40) - 1)
    build = np.concatenate([distinct, distinct[rng.integers(0, nd, nb // 4)]])
    rng.shuffle(build)
    pick = rng.integers(0, nd, nl)
    probe = np.where(rng.random(nl) < 0.5, distinct[pick], (1 << 41) + pick)
    dprobe, dbuild = amd.Array.from_numpy(probe), amd.Array.from_numpy(build)
    times, rows = [], 0
    for i in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        li, ri = amd.compute.hash_join_indices([dprobe], [dbuild], "inner")
        torch.cuda.synchronize()
        if i:
            times.append(time.perf_counter() - t0)
        rows = li.length
        del li, ri
    # residual filter: (lid + rid) even, about half the pairs; evaluated with the mirror's element-wise kernels
    def half(lrows, rrows):
        s = amd.compute.add(lrows, rrows)
        q = amd.compute.divide(s, 2)
        return amd.compute.equal(amd.compute.add(q, q), s)

    # the predicate's own element-wise calls are timed apart, so that the rest is the join with its filter kernels
    ftimes, ptimes, frows, cands = [], [], 0, 0
    for i in range(a.reps + 1):
        spent = [0.0]

        def timed(lrows, rrows):
            torch.cuda.synchronize()
            p0 = time.perf_counter()
            out = half(lrows, rrows)
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - p0
            return out

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        li, ri = amd.compute.hash_join_indices([dprobe], [dbuild], "left outer", filter=timed)
        torch.cuda.synchronize()
        if i:
            ftimes.append(time.perf_counter() - t0 - spent[0])
            ptimes.append(spent[0])
        frows, cands = li.length, rows
        del li, ri
    pa.set_cpu_count(min(16, os.cpu_count() or 1))
    lt = pa.table({"k": probe, "lid": np.arange(nl, dtype=np.int64)})
    rt = pa.table({"k": build, "rid": np.arange(nb, dtype=np.int64)})
    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        j = lt.join(rt, "k", join_type="inner")
        host.append(time.perf_counter() - t0)
        assert j.num_rows == rows, (j.num_rows, rows)
        del j
    dev_ms = 1e3 * float(np.median(times))
    host_ms = 1e3 * float(np.median(host)) if host else float("nan")
    print(json.dumps({"probe_rows": nl, "build_rows": nb, "output_rows": int(rows), "device_mirror_ms": round(dev_ms, 2),
                      "filtered_left_outer_rows": int(frows), "candidate_pairs": int(cands),
                      "device_mirror_filtered_ms_without_predicate": round(1e3 * float(np.median(ftimes)), 2),
                      "predicate_ms": round(1e3 * float(np.median(ptimes)), 2),
                      "host_pa_join_ms": round(host_ms, 2), "host_threads": pa.cpu_count(),
                      "speedup": round(host_ms / dev_ms, 1) if host else None}))


if __name__ == "__main__":
    main()
