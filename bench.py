#!/usr/bin/env python
"""bench.py — the headline benchmark of BASELINE.json, on synthetic data resident in HBM.

    python bench.py --gpus N --steps K --warmup W

N = 1 (default): BASELINE.json configs[1] — Filter + Take on a 1B-row int64 array with a validity
bitmap (10 % null), boolean mask with 10 % selectivity, FilterOptions::DROP:
    step = compute.filter(values, mask)                       # array_filter (count, scan, compact)
         + compute.get_take_indices(mask)                     # GetTakeIndices -> uint32[S]
         + compute.take(values, indices, boundscheck=False)   # the Table/RecordBatch filter path
`value` = input rows per second through one whole step (Mrows/s), all N ranks together.
Filter/take do not shard (north_star: "filter/take/cast stay single-GPU"): with N > 1 every rank runs an
independent replica on its own GPU ("replicas only", weak scaling).  With `--full` the sharded paths ride in the
same JSON line: `hash_sum` (configs[3]: 4B rows / 10M keys, rows split over the N ranks, local aggregate -> ONE
all-to-all of 24-byte partials -> merge; strong scaling) and `sort_indices` (configs[4]: 2B uint64 rows,
splitters -> ONE all-to-all of 12-byte records -> local sort).

N > 1 without a launcher: `python bench.py --gpus N` starts the N ranks itself (one process per GPU,
LOCAL_RANK -> device, rendezvous on 127.0.0.1 and a free port); under torchrun (WORLD_SIZE set) it is one rank.

Inputs are SURVEY.md 8(d)'s counter-based streams r(i, seed) = splitmix64(seed + i), generated on the device
(numpy twin: splitmix64_np) — values r(i,1), mask r(i,2) % 100 < 10, validity r(i,3) % 100 >= 10,
group-by keys r(i,8) % 10M, values r(i,9), sort keys r(i,10), the cast mix of seed 6.

One JSON line on stdout (rank 0).  `roofline` prices the dominant kernel (the filter compaction,
arx_filter_exec) in ALGORITHMIC bytes (8N + N/8 + N/8 + 8S + S/8) over its HIP-event
duration measured live; `cpu_baseline` times the reference's own CPU kernels (pyarrow wheel =
libarrow.so, kind "reference"; the C oracle as kind "port" if the wheel is absent) on a bounded sample of the
same data: one thread (how the kernel layer executes) and the multi-core Acero plan; `value` = the better.
`--backend emu` (tests only) runs the same file on CPU tensors + gloo with the kernel sources under the
SIMT emulator of tests/emu: it checks the launcher and the multi-rank plumbing, never performance.

A plain run does only what `value` needs: it generates the inputs, warms up, times `--steps` steps of the route
`value` stands for and prints the line (`metric`, `value`, `unit`, `ms_per_step`, `config`, ...).  Everything else
named above (the mirror loop's kernel events and `roofline`, the copy ceiling, `parity_spot_check`, `cpu_baseline`,
the other paths and the sharded legs) runs with `--full`.  `--dump-outputs DIR` writes what the timed route returned
in its last step (filter result, row numbers, take result) as float64 .npy files (dump_outputs); the inputs depend on
the arguments alone, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
EMU = False            # --backend emu
_JSON_FD = [1]         # where the one JSON line goes (main() moves everything else that writes to fd 1 over to stderr)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# ------------------------------------------------------------------ counter-based input streams
_M1 = 0xBF58476D1CE4E5B9 - (1 << 64)
_M2 = 0x94D049BB133111EB - (1 << 64)
_GAMMA = 0x9E3779B97F4A7C15 - (1 << 64)


def _lsr(z: torch.Tensor, k: int) -> torch.Tensor:
    return (z >> k) & ((1 << (64 - k)) - 1)


def splitmix64(first: int, count: int, seed: int, device) -> torch.Tensor:
    """r(i, seed) for i in [first, first + count) as int64 bit patterns (two's complement of the uint64)."""
    z = torch.arange(first, first + count, dtype=torch.int64, device=device) + seed
    z = z + _GAMMA
    z = (z ^ _lsr(z, 30)) * _M1
    z = (z ^ _lsr(z, 27)) * _M2
    return z ^ _lsr(z, 31)


def splitmix64_np(first: int, count: int, seed: int) -> np.ndarray:
    """Host twin of splitmix64 (uint64)."""
    with np.errstate(over="ignore"):
        z = np.arange(first, first + count, dtype=np.uint64) + np.uint64(seed % (1 << 64))
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def umod(z: torch.Tensor, m: int) -> torch.Tensor:
    """(uint64 view of z) % m for an int64 tensor."""
    r = torch.remainder(z, m)
    return torch.where(z < 0, (r + ((1 << 64) % m)) % m, r)


def pack_bits_device(bools: torch.Tensor) -> torch.Tensor:
    """bool[n] (n % 8 == 0) -> LSB-first bitmap bytes on the device (data generation only)."""
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=bools.device)
    return (bools.view(-1, 8).to(torch.uint8) * w).sum(dim=1, dtype=torch.uint8)


CHUNK = 1 << 26


def gen_filter_inputs(n: int, device, first_row: int, null_p: float, true_p: float, mask_null_p: float = 0.0):
    """values int64[n] = r(i,1); validity bit = r(i,3) % 100 >= 100 null_p; mask bit = r(i,2) % 100 < 100 true_p;
    mask validity (secondary config, vector_selection_benchmark.cc:59-75) bit = r(i,4) % 100 >= 100 mask_null_p."""
    from arrow_amd.array import alloc

    n8 = (n + 7) // 8 * 8
    nbytes = (n8 // 8 + 7) // 8 * 8
    values = alloc(n * 8, device)
    validity = alloc(nbytes, device, zero=True)
    mask = alloc(nbytes, device, zero=True)
    mask_valid = alloc(nbytes, device, zero=True) if mask_null_p > 0 else None
    v64 = values[: n * 8].view(torch.int64)
    chunk = min(CHUNK, n8)
    for b in range(0, n8, chunk):
        e = min(n8, b + chunk)
        live = min(e, n) - b
        if live > 0:
            v64[b:b + live] = splitmix64(first_row + b, live, 1, device)
        in_range = torch.arange(b, e, device=device) < n

        def bits(seed, thresh, ge):
            r = umod(splitmix64(first_row + b, e - b, seed, device), 100)
            return ((r >= thresh) if ge else (r < thresh)) & in_range

        validity[b // 8: e // 8] = pack_bits_device(bits(3, int(round(100 * null_p)), True))
        mask[b // 8: e // 8] = pack_bits_device(bits(2, int(round(100 * true_p)), False))
        if mask_valid is not None:
            mask_valid[b // 8: e // 8] = pack_bits_device(bits(4, int(round(100 * mask_null_p)), True))
    return values, validity, mask, mask_valid


def gen_cast_mix(n: int, device, first_row: int = 0, seed: int = 6) -> torch.Tensor:
    """float64[n] of SURVEY.md 8(d) config 3a: 90 % N(0,1) (Box-Muller on the stream), 5 % magnitudes beyond
    FLT_MAX, 4 % in float32's subnormal range, 1 % +-0 / +-inf / NaN."""
    out = torch.empty(n, dtype=torch.float64, device=device)
    two53 = float(1 << 53)
    for b in range(0, n, CHUNK):
        m = min(CHUNK, n - b)
        cls = umod(splitmix64(first_row + b, m, seed, device), 100)
        u1 = (_lsr(splitmix64(first_row + b, m, seed + 100, device), 11).to(torch.float64) + 1.0) / two53
        u2 = _lsr(splitmix64(first_row + b, m, seed + 200, device), 11).to(torch.float64) / two53
        g = torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(6.283185307179586 * u2)
        sign = torch.where(u2 < 0.5, -1.0, 1.0).to(torch.float64)
        big = sign * 3.4028234663852886e38 * (1.0 + 1e6 * u1)                 # |x| > FLT_MAX -> +-inf in float32
        sub = sign * 1.1754943508222875e-38 * u1                              # float32-subnormal results
        k = umod(splitmix64(first_row + b, m, seed + 300, device), 5)
        special = torch.where(k == 0, 0.0, torch.where(k == 1, -0.0, torch.where(k == 2, float("inf"),
                              torch.where(k == 3, float("-inf"), float("nan"))))).to(torch.float64)
        out[b:b + m] = torch.where(cls < 90, g, torch.where(cls < 95, big, torch.where(cls < 99, sub, special)))
    return out


def gen_normal(n: int, device, seed: int) -> torch.Tensor:
    out = torch.empty(n, dtype=torch.float64, device=device)
    two53 = float(1 << 53)
    for b in range(0, n, CHUNK):
        m = min(CHUNK, n - b)
        u1 = (_lsr(splitmix64(b, m, seed + 100, device), 11).to(torch.float64) + 1.0) / two53
        u2 = _lsr(splitmix64(b, m, seed + 200, device), 11).to(torch.float64) / two53
        out[b:b + m] = torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(6.283185307179586 * u2)
    return out


def gen_stream(n: int, device, first_row: int, seed: int, modulo: int = 0, dtype=torch.int64) -> torch.Tensor:
    out = torch.empty(n, dtype=dtype, device=device)
    for b in range(0, n, CHUNK):
        m = min(CHUNK, n - b)
        z = splitmix64(first_row + b, m, seed, device)
        out[b:b + m] = (umod(z, modulo) if modulo else z).to(dtype)
    return out


def gen_validity(n: int, device, first_row: int, seed: int, null_pct: int) -> torch.Tensor:
    """LSB-first bitmap with null_pct % clear bits (r(i, seed) % 100 >= null_pct)."""
    from arrow_amd.array import alloc

    n8 = (n + 7) // 8 * 8
    bm = alloc((n8 // 8 + 7) // 8 * 8, device, zero=True)
    chunk = min(CHUNK, n8)
    for b in range(0, n8, chunk):
        e = min(n8, b + chunk)
        ok = (umod(splitmix64(first_row + b, e - b, seed, device), 100) >= null_pct) & \
             (torch.arange(b, e, device=device) < n)
        bm[b // 8: e // 8] = pack_bits_device(ok)
    return bm


# ------------------------------------------------------------------ timers
class _WallTimer:
    """KernelTimer twin for the emulated backend (kernels run synchronously there)."""

    def __init__(self):
        self.events = {}

    def start(self, name):
        rec = [time.perf_counter(), None]
        self.events.setdefault(name, []).append(rec)
        return rec

    def stop(self, rec):
        rec[1] = time.perf_counter()

    def elapsed_ms(self, name):
        return [(e - s) * 1e3 for s, e in self.events.get(name, [])]


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def _time_gpu(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    if EMU:
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps * 1e3
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def copy_ceiling(amd, device, nbytes=1 << 30):
    """What this box's HBM gives a plain copy: arx_buffer_copy (16 bytes per lane, one-shot grid) of 1 GiB, read +
    written bytes per second.  Every `frac` of the line is priced against the 8 TB/s spec peak; this figure says how
    much of the distance to that peak is the box (MI355X_MICROARCH.md measures 6.29 TB/s for the same copy)."""
    src = torch.empty(nbytes, dtype=torch.uint8, device=device)
    src.random_(0, 256)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=device)
    ms = min(_time_gpu(lambda: amd.compute.copy_buffer(src, dst), reps=5, warm=2) for _ in range(3))
    del src, dst
    return round(2 * nbytes / ms / 1e6, 1)


def _barrier(world):
    if world > 1:
        torch.distributed.barrier()


def _max_over_ranks(x: float, world, device) -> float:
    if world > 1:
        t = torch.tensor([x], dtype=torch.float64, device=device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        return float(t.item())
    return x


def load_traffic(name: str, rows: int, form: str | None = None):
    """HBM bytes per launch / per run from the committed PMC pass (profiles/<name>_traffic.json), or null — also null
    when the pass measured another form of the pipeline than the one that runs now (`form`)."""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", f"{name}_traffic.json")))
        if int(d.get("rows", -1)) == int(rows) and d.get("form") == form:
            return d.get("hbm_bytes_per_launch")
    except Exception:
        pass
    return None


# ------------------------------------------------------------------ CPU baselines (reference kernels, same box)
def _host_cores() -> int:
    try:
        return len(os.sched_getaffinity(0))
    except Exception:
        return os.cpu_count() or 1


def cpu_baseline_filter_take(values, validity, mask, n_total: int, sample_rows: int, budget_s: float):
    """Reference CPU kernels on the first `sample_rows` rows of the very same buffers: (i) one thread — how the
    kernel layer executes a CallFunction (exec.cc:1144) — and (ii) the multi-core Acero plan
    table_source -> filter -> sink (use_threads, pool = all cores).  `value` = the better of the two."""
    n = min(n_total, sample_rows)
    n -= n % 64
    hv = values[: n * 8].cpu().numpy()
    hval = validity[: n // 8].cpu().numpy()
    hm = mask[: n // 8].cpu().numpy()
    try:
        import pyarrow as pa
        import pyarrow.compute as pc
    except Exception:
        pa = None
    cores_all = _host_cores()
    if pa is None:
        from oracle import oracle as O      # checker used as the "port" baseline only when the wheel is absent

        n = min(n, 1 << 25)
        hv64 = hv[: n * 8].view(np.int64)
        reps, t_total = 0, 0.0
        while reps < 2 or (t_total < budget_s and reps < 4):
            t0 = time.perf_counter()
            O.filter(hv64, hval, 0, hm, None, 0, n, 0, True)
            idx, _ = O.mask_to_indices(hm, None, 0, n, 0, False)
            O.take(hv64, hval, 0, idx, None, 0, len(idx), True)
            t_total += time.perf_counter() - t0
            reps += 1
        return {"value": round(n * reps / t_total / 1e6, 2), "unit": "Mrows/s", "cores": 1, "kind": "port",
                "sample": f"first {n} rows, {reps} reps, oracle/arx_oracle.c filter + mask_to_indices + take",
                "host_cpus": cores_all}
    from pyarrow import acero

    varr = pa.Array.from_buffers(pa.int64(), n, [pa.py_buffer(hval), pa.py_buffer(hv)], null_count=-1)
    marr = pa.Array.from_buffers(pa.bool_(), n, [None, pa.py_buffer(hm)], null_count=0)
    table = pa.table({"v": varr})
    # (i) one thread: a CallFunction on one contiguous array never leaves the calling thread (exec.cc:1144).
    # (The CPU pool is never resized here: Acero sizes its per-thread state once, at first use.)
    reps, t_total = 0, 0.0
    while reps < 2 or (t_total < budget_s / 2 and reps < 8):
        t0 = time.perf_counter()
        a = pc.filter(varr, marr)          # array_filter: PrimitiveFilterExec
        b = table.filter(marr)             # FilterTable: GetTakeIndices + Take
        t_total += time.perf_counter() - t0
        reps += 1
        del a, b
    single = n * reps / t_total / 1e6
    # (ii) Acero, all cores: the same two results (filtered column twice) from one threaded plan per path
    threads = pa.cpu_count()
    tm = pa.table({"v": varr, "m": marr})
    plan = acero.Declaration.from_sequence([
        acero.Declaration("table_source", acero.TableSourceNodeOptions(tm)),
        acero.Declaration("filter", acero.FilterNodeOptions(pc.field("m"))),
        acero.Declaration("project", acero.ProjectNodeOptions([pc.field("v")], ["v"]))])
    reps2, t2 = 0, 0.0
    try:
        while reps2 < 2 or (t2 < budget_s / 2 and reps2 < 8):
            t0 = time.perf_counter()
            a = plan.to_table(use_threads=True)
            b = plan.to_table(use_threads=True)   # the step filters twice (array_filter + the take path)
            t2 += time.perf_counter() - t0
            reps2 += 1
            del a, b
        multi = n * reps2 / t2 / 1e6
    except Exception as e:  # pragma: no cover - informational
        multi, reps2 = 0.0, 0
        log(f"[cpu_baseline] Acero plan failed: {e}")
    best = max(single, multi)
    return {"value": round(best, 2), "unit": "Mrows/s", "cores": 1 if single >= multi else threads,
            "kind": "reference",
            "sample": f"first {n} rows of the same HBM buffers; pyarrow {pa.__version__} (libarrow CPU kernels)",
            "single_thread_mrows_per_s": round(single, 2), "single_thread_what": f"pc.filter + Table.filter, {reps} reps",
            "acero_mrows_per_s": round(multi, 2),
            "acero_what": f"table_source -> filter -> project x2, use_threads, {threads} threads, {reps2} reps",
            "host_cpus": cores_all, "simd": str(pa.runtime_info().simd_level)}


def cpu_baseline_hash_sum(rows: int, groups: int, budget_s: float):
    """pyarrow Table.group_by(k).aggregate(sum) (Acero GroupByNode + hash_sum) on a DOWN-SCALED prefix of the same
    streams: single-thread and multi-thread (the reference's serial merge often makes threads slower; min reported)."""
    try:
        import pyarrow as pa
    except Exception:
        return None
    n = rows
    k = (splitmix64_np(0, n, 8) % np.uint64(groups)).astype(np.int32)
    v = splitmix64_np(0, n, 9).view(np.int64)
    t = pa.table({"k": pa.array(k), "v": pa.array(v)})
    res = {}
    cores_all = _host_cores()
    for name, threads in (("single_thread", 1), ("multi_thread", pa.cpu_count())):
        t0 = time.perf_counter()
        out = t.group_by("k", use_threads=threads > 1).aggregate([("v", "sum")])
        dt = time.perf_counter() - t0
        res[name] = (n / dt / 1e6, threads, out.num_rows)
        if dt > budget_s:
            break
    best = max(res.values(), key=lambda x: x[0])
    # the reference's answer on this prefix, key-sorted (acero/hash_aggregate_test.cc:262-280 sorts, then compares): kept for
    # the parity leg, which runs the device plan the bench times on the same rows and diffs
    rk, rs = out.column("k").to_numpy(), out.column("v_sum").to_numpy()
    o = np.argsort(rk, kind="stable")
    _CPU_REF["hash_sum"] = (n, groups, rk[o].copy(), rs[o].copy())
    return {"value": round(best[0], 2), "unit": "Mrows/s", "cores": best[1], "kind": "reference",
            "sample": f"SURVEY 8(d) sample: first {n} rows of the same streams ({best[2]} groups), pyarrow {pa.__version__} "
                      "Table.group_by(k).aggregate([(v, sum)])",
            **{f"{nm}_mrows_per_s": round(x[0], 2) for nm, x in res.items()}, "host_cpus": cores_all}


def cpu_baseline_cast_greater(rows: int, device):
    """the reference's own kernels on the SAME rows the GPU legs read — pc.cast(float64 -> float32,
    safe=False) on gen_cast_mix's stream and pc.greater(float64, float64) on the two normal streams — on ONE thread (a
    scalar kernel over one Array runs on the calling thread: `cores` = 1).  Keeps the reference's full results (4 GB of
    float32, 125 MB of bits) in _CPU_REF: run_other_paths diffs the device results of the timed calls against them."""
    import pyarrow as pa
    import pyarrow.compute as pc

    out = {}
    x = gen_cast_mix(rows, device).cpu().numpy()
    ax = pa.array(x)
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        ref = pc.cast(ax, pa.float32(), safe=False)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    _CPU_REF["cast_f64_f32"] = ref.to_numpy(zero_copy_only=True).view(np.uint32).copy()
    out["cast_f64_f32"] = {"value": round(rows / best / 1e6, 1), "unit": "Mrows/s", "cores": 1, "kind": "reference",
                           "sample": f"all {rows} rows of the leg's stream; pyarrow {pa.__version__} pc.cast(float64 -> float32, safe=False), one thread, best of 2",
                           "seconds": round(best, 3)}
    del x, ax, ref
    a = gen_normal(rows, device, 6).cpu().numpy()
    b = gen_normal(rows, device, 7).cpu().numpy()
    aa, ab = pa.array(a), pa.array(b)
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        ref = pc.greater(aa, ab)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    _CPU_REF["greater_f64"] = np.frombuffer(ref.buffers()[1], dtype=np.uint8)[: (rows + 7) // 8].copy()
    out["greater_f64"] = {"value": round(rows / best / 1e6, 1), "unit": "Mrows/s", "cores": 1, "kind": "reference",
                          "sample": f"all {rows} rows of the leg's streams; pyarrow {pa.__version__} pc.greater(float64, float64), one thread, best of 2",
                          "seconds": round(best, 3)}
    return out


def cpu_baseline_sort(rows: int):
    try:
        import pyarrow as pa
        import pyarrow.compute as pc
    except Exception:
        return None
    k = splitmix64_np(0, rows, 10)
    arr = pa.array(k)
    t0 = time.perf_counter()
    out = pc.sort_indices(arr)       # one contiguous array: runs on the calling thread
    dt = time.perf_counter() - t0
    _CPU_REF["sort_indices"] = (rows, out.to_numpy(zero_copy_only=False).astype(np.int64, copy=False))   # kept for the parity leg
    del out
    return {"value": round(rows / dt / 1e6, 2), "unit": "Mrows/s", "cores": 1, "kind": "reference",
            "sample": f"SURVEY 8(d) sample: first {rows} rows of the same stream, pyarrow {pa.__version__} pc.sort_indices "
                      "(std::stable_sort on indices, one thread)", "host_cpus": _host_cores()}


# ------------------------------------------------------------------ parity of the sharded legs' timed plans (outside the timed region)
_CPU_REF = {}          # the reference's results on the 1e8-row prefixes, kept by the cpu_baseline_* functions


def _counters(lib, names):
    return {n: int(lib.arx_get_counter(n.encode())) for n in names}


def parity_hash_sum_prefix(device, groups_arg):
    """The device group-by — the SAME plan the 4e9-row leg is timed on (the lines plan follows the key range, the wide plan
    the group count, neither the row count; the counters say which ran, and the wide plan is forced if another one did) — on the first 1e8 rows of
    streams 8 / 9, diffed against pyarrow's Table.group_by on the same rows: key-sorted (key, sum) equality."""
    import arrow_amd as amd
    from arrow_amd import parallel

    n, groups, ref_k, ref_s = _CPU_REF["hash_sum"]
    assert groups == groups_arg
    lib = amd._lib.get_lib()
    keys = gen_stream(n, device, 0, 8, modulo=groups, dtype=torch.int32)
    vals = gen_stream(n, device, 0, 9)
    kk = amd.Array(amd.array.int32, n, [None, keys.view(torch.uint8)], 0, 0)
    vv = amd.Array(amd.array.int64, n, [None, vals.view(torch.uint8)], 0, 0)
    cap = 1
    while cap < 2 * groups + 2:
        cap <<= 1
    names = ("groupby_slices_lines", "groupby_lines_fallbacks", "groupby_slices_wide", "groupby_slices_rooms", "groupby_slices_two_level",
             "groupby_slices_one_level", "groupby_slices_direct")
    forced = False
    for attempt in (0, 1):
        c0 = _counters(lib, names)
        gk, gk_valid, gs, gs_valid = parallel.sharded_group_by_sum(kk, vv, cap)[:4]
        _sync(device)
        plan = {k: v - c0[k] for k, v in _counters(lib, names).items() if v != c0[k]}
        # (round 6: ids from [0, groups) take the lines plan at any row count, as the timed leg does; where it declined,
        #  the wide plan is what the timed leg fell back to)
        if plan.get("groupby_slices_lines", 0) > 0 or plan.get("groupby_slices_wide", 0) > 0 or attempt == 1:
            break
        assert lib.arx_set_option(b"groupby_wide", 2) == 0 and lib.arx_set_option(b"groupby_partition_bits", 11) == 0
        forced = True
    if forced:
        lib.arx_set_option(b"groupby_wide", 1)
        lib.arx_set_option(b"groupby_partition_bits", -1)
    hk = gk.cpu().numpy().view(np.int32)
    hs = gs.cpu().numpy().view(np.int64)
    o = np.argsort(hk, kind="stable")
    equal = bool(len(hk) == len(ref_k) and bool(gk_valid.all().item()) and bool(gs_valid.all().item()) and
                 (hk[o] == ref_k).all() and (hs[o] == ref_s).all())
    return ("equal" if equal else "MISMATCH"), {"rows": n, "groups": int(len(hk)), "wide_plan_forced": forced, **plan}


def acero_hash_sum_full(device, rows, groups, reps=3):
    """the SAME work as the hash_sum leg — every row of streams 8 / 9 — through the drop-in route instead of
    the Python mirror: an Acero plan `table_source_rocm -> aggregate_rocm` (hash_sum, int32 key) over a device-resident pyarrow
    table that wraps the HBM buffers without a copy; the result is a host table, as GroupByNode's is.  Checked: number of
    groups, and the wrap-around sum of the group sums against the sum of the values."""
    import pyarrow as pa
    import pyarrow.compute as pc
    from pyarrow import acero

    plug = plugin_session()
    keys = gen_stream(rows, device, 0, 8, modulo=groups, dtype=torch.int32)
    vals = gen_stream(rows, device, 0, 9)
    tab = pa.table({"k": plug.wrap(pa.int32(), rows, keys.view(torch.uint8)), "v": plug.wrap(pa.int64(), rows, vals.view(torch.uint8))})
    plan = acero.Declaration.from_sequence([
        acero.Declaration("table_source_rocm", acero.TableSourceNodeOptions(tab)),
        acero.Declaration("aggregate_rocm", acero.AggregateNodeOptions([("v", "hash_sum", None, "v_sum")], keys=["k"]))])
    out = plan.to_table(use_threads=False)      # warm-up (pools, first-use allocations)
    for f in ("arrow_amd_plugin_aggregate_range_plans", "arrow_amd_plugin_aggregate_range_declined"):
        getattr(plug.lib, f).restype = plug.ctypes.c_int64
    r0, x0 = plug.lib.arrow_amd_plugin_aggregate_range_plans(), plug.lib.arrow_amd_plugin_aggregate_range_declined()
    ts = []
    for _ in range(reps):
        out = None
        _sync(device)
        t0 = time.perf_counter()
        out = plan.to_table(use_threads=False)
        ts.append(time.perf_counter() - t0)
    state = {"range_partitioned_state_plans": plug.lib.arrow_amd_plugin_aggregate_range_plans() - r0,
             "declined_to_the_table": plug.lib.arrow_amd_plugin_aggregate_range_declined() - x0, "plans": reps}
    want = int(vals.sum().item())
    got = int(np.asarray(out.column("v_sum").to_numpy()).view(np.uint64).sum(dtype=np.uint64).view(np.int64)) if out.num_rows else 0
    ms = sorted(ts)[len(ts) // 2] * 1e3
    return {"what": "acero table_source_rocm -> aggregate_rocm (hash_sum) over the same rows as a device-resident pyarrow table "
                    "(zero-copy wrap of the HBM buffers), host result table; median of %d" % reps,
            "ms": round(ms, 3), "ms_min": round(min(ts) * 1e3, 3), "mrows_per_s": round(rows / ms / 1e3, 1),
            "groups": out.num_rows, "checksum_matches_sum_of_values": bool(got == want), "state": state}


def parity_sort_prefix(device):
    """array_sort_indices on the first 1e8 rows of stream 10 with the WIDE form forced (the form the 2e9-row leg is timed
    on is chosen by row count: sort_msd_segment_rows lowers its threshold here), diffed against pyarrow's sort_indices:
    exact index equality (vector_sort_test.cc:971-1062 compares indices)."""
    import arrow_amd as amd
    from arrow_amd import parallel

    n, ref = _CPU_REF["sort_indices"]
    lib = amd._lib.get_lib()
    keys = gen_stream(n, device, 0, 10)
    ak = amd.Array(amd.array.uint64, n, [None, keys.view(torch.uint8)], 0, 0)
    names = ("sort_wide_runs", "sort_wide_rec8_runs", "sort_wide_rec8_ties", "sort_wide_rec8_given_up")
    c0 = _counters(lib, names)
    assert lib.arx_set_option(b"sort_msd_segment_rows", 4096) == 0
    try:
        rows, _ = parallel.sharded_sort_indices(ak)
        _sync(device)
    finally:
        lib.arx_set_option(b"sort_msd_segment_rows", 1 << 27)
    plan = {k: v - c0[k] for k, v in _counters(lib, names).items()}
    want = torch.from_numpy(ref).to(device)
    equal = bool(rows.numel() == want.numel() and torch.equal(rows, want)) and plan["sort_wide_runs"] >= 1
    return ("equal" if equal else "MISMATCH"), {"rows": n, **plan}


# ------------------------------------------------------------------ parity spot check (outside the timed region)
def parity_spot_check(amd, values, validity, mask, n_total: int):
    """Device filter+take on a prefix vs the C oracle (the checker; never the thing measured)."""
    from oracle import oracle as O

    n = min(n_total, 1 << 21)
    n -= n % 64
    if n <= 0:
        return True
    dv = amd.Array(amd.array.int64, n, [validity, values], -1, 0)
    dm = amd.Array(amd.array.bool_, n, [None, mask], 0, 0)
    out = amd.compute.filter(dv, dm)
    idx = amd.compute.get_take_indices(dm)
    tk = amd.compute.take(dv, idx, boundscheck=False)
    _sync(values.device)
    hv = values[: n * 8].cpu().numpy().view(np.int64)
    hval = validity[: n // 8].cpu().numpy()
    hm = mask[: n // 8].cpu().numpy()
    # the inputs themselves must be the documented streams
    ok = bool((hv.view(np.uint64) == splitmix64_np(int(getattr(values, "_first_row", 0)), n, 1)).all())
    want, want_bm = O.filter(hv, hval, 0, hm, None, 0, n, 0, True)
    got = out.data[: out.length * 8].cpu().numpy().view(np.int64)
    ok = ok and out.length == len(want) and bool((got == want).all())
    gv = np.unpackbits(out.validity.cpu().numpy(), bitorder="little")[: out.length].astype(bool)
    ok = ok and bool((gv == O.unpack_bits(want_bm, 0, out.length)).all())
    gt = tk.data[: tk.length * 8].cpu().numpy().view(np.int64)
    tvalid = np.unpackbits(tk.validity.cpu().numpy(), bitorder="little")[: tk.length].astype(bool)
    ok = ok and tk.length == out.length and bool((tvalid == gv).all()) and bool((gt[tvalid] == want[gv]).all())
    return ok


# ------------------------------------------------------------------ legs
# ------------------------------------------------------------------ the drop-in route: pyarrow.compute on device arrays
class PluginSession:
    """libarrow_amd_plugin.so loaded and registered in this process: from here on pyarrow.compute / Acero calls on
    device-resident arrays run the HIP kernels behind Arrow's own FunctionRegistry (and host calls of the extended
    functions pass through the shim to the reference kernels), so every CPU baseline is taken BEFORE this is made."""

    def __init__(self):
        import ctypes

        import pyarrow as pa

        from arrow_amd.plugin_build import build_plugin

        self.ctypes, self.pa = ctypes, pa
        self.lib = ctypes.CDLL(build_plugin(verbose=False))
        self.lib.arrow_amd_plugin_last_error.restype = ctypes.c_char_p
        self.lib.arrow_amd_plugin_calls.restype = ctypes.c_int64
        self.lib.arrow_amd_plugin_calls.argtypes = [ctypes.c_char_p, ctypes.c_int]
        self.lib.arrow_amd_wrap_device_memory.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_void_p]
        assert self.lib.arrow_amd_register() == 0, self.lib.arrow_amd_plugin_last_error()

    def wrap(self, pa_type, length, data: torch.Tensor, validity: torch.Tensor = None, null_count: int = 0):
        """A torch tensor's HBM as a device-resident pyarrow array, zero-copy (arrow_amd_wrap_device_memory)."""
        ct, pa = self.ctypes, self.pa
        c_schema, c_dev = ct.create_string_buffer(72), ct.create_string_buffer(128)
        pa_type._export_to_c(ct.addressof(c_schema))
        rc = self.lib.arrow_amd_wrap_device_memory(ct.addressof(c_schema), length, null_count,
                                                   validity.data_ptr() if validity is not None else None, data.data_ptr(),
                                                   ct.addressof(c_dev))
        assert rc == 0, self.lib.arrow_amd_plugin_last_error()
        return pa.Array._import_from_c_device(ct.addressof(c_dev), pa_type)

    def to_device(self, arr):
        ct, pa = self.ctypes, self.pa
        c_arr, c_schema, c_dev = (ct.create_string_buffer(k) for k in (80, 72, 128))
        arr._export_to_c(ct.addressof(c_arr), ct.addressof(c_schema))
        assert self.lib.arrow_amd_copy_to_device(c_arr, c_schema, c_dev) == 0, self.lib.arrow_amd_plugin_last_error()
        return pa.Array._import_from_c_device(ct.addressof(c_dev), arr.type)

    def to_numpy(self, darr):
        """A device-resident pyarrow array of a fixed-width type -> (values, valid or None) on the host
        (arrow_amd_copy_to_host)."""
        ct, pa = self.ctypes, self.pa
        c_dev, c_schema, c_arr, c_schema2 = (ct.create_string_buffer(k) for k in (128, 72, 80, 72))
        darr._export_to_c_device(ct.addressof(c_dev), ct.addressof(c_schema))
        assert self.lib.arrow_amd_copy_to_host(c_dev, c_schema, c_arr, c_schema2) == 0, self.lib.arrow_amd_plugin_last_error()
        h = pa.Array._import_from_c(ct.addressof(c_arr), ct.addressof(c_schema2))
        vb, db = h.buffers()
        n, off = len(h), h.offset
        dtype = h.type.to_pandas_dtype()
        values = np.frombuffer(db, dtype=dtype, count=off + n)[off:] if n else np.zeros(0, dtype)
        valid = None
        if vb is not None:
            valid = np.unpackbits(np.frombuffer(vb, dtype=np.uint8), bitorder="little")[off:off + n].astype(bool)
        return values, valid


DUMP_SAMPLE_ROWS = 1 << 19    # rows per output that --dump-outputs writes (a seeded sample of a longer output)
DUMP_SEED = 20240601


def dump_outputs(path: str, outputs: dict) -> None:
    """--dump-outputs: the arrays the timed path returned in its last step, as float64 .npy files that a run of another
    build with the same arguments can be compared with, output for output.  `outputs` maps a name to (int64 values,
    valid or None).  Per output: `<name>.npy` = its values on a fixed, seeded sample of its rows (every row when it has
    at most DUMP_SAMPLE_ROWS), shape (rows, 2): the signed upper and the lower 32 bits, both exact in float64, 0 under
    a null; `<name>_valid.npy` = the validity of those rows (float32 0 / 1); `<name>_rows.npy` = the row numbers.
    `checksums.npy` covers every row: per output (in `outputs` order) [rows, valid rows, upper 32 bits, lower 32 bits
    of the wrap-around sum of the valid values]."""
    os.makedirs(path, exist_ok=True)

    def hi_lo(v):
        v = np.asarray(v, dtype=np.int64)
        return np.stack([(v >> 32).astype(np.float64), (v & 0xFFFFFFFF).astype(np.float64)], axis=-1)

    sums = []
    for name, (values, valid) in outputs.items():
        values = np.asarray(values).astype(np.int64, copy=False)
        n = len(values)
        ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
        if n <= DUMP_SAMPLE_ROWS:
            rows = np.arange(n)
        else:
            rows = np.sort(np.random.default_rng(DUMP_SEED).integers(0, n, DUMP_SAMPLE_ROWS))
        np.save(os.path.join(path, f"{name}.npy"), hi_lo(np.where(ok[rows], values[rows], 0)))
        np.save(os.path.join(path, f"{name}_valid.npy"), ok[rows].astype(np.float32))
        np.save(os.path.join(path, f"{name}_rows.npy"), rows.astype(np.float64))
        total = int(np.where(ok, values, 0).view(np.uint64).sum(dtype=np.uint64))
        sums.append([n, int(ok.sum()), float(total >> 32), float(total & 0xFFFFFFFF)])
    np.save(os.path.join(path, "checksums.npy"), np.array(sums, dtype=np.float64).reshape(-1, 4))


_PLUGIN = [None]


def plugin_session():
    if _PLUGIN[0] is None:
        _PLUGIN[0] = PluginSession()
    return _PLUGIN[0]


def run_filter_take(args, rank, world, device):
    import arrow_amd as amd
    from arrow_amd import tracing

    n = args.rows
    t0 = time.time()
    first_row = rank * n     # every replica reads its own stretch of the streams
    values, validity, mask, _ = gen_filter_inputs(n, device, first_row, args.null_p, args.selectivity)
    _sync(device)
    if not EMU:
        # the generator's temporaries (GBs) go back to the device before the routes allocate their outputs: the plugin's
        # pool cannot reuse torch's cached blocks, and a route timed with them still held measured ~2 % slower
        torch.cuda.empty_cache()
    log(f"[rank {rank}] generated {n} rows in {time.time() - t0:.1f}s")
    dv = amd.Array(amd.array.int64, n, [validity, values], -1, 0)
    dm = amd.Array(amd.array.bool_, n, [None, mask], 0, 0)

    # ---- the reference's CPU kernels FIRST (rank 0, N = 1): registering the plugin re-routes pyarrow's own functions
    cpu = {}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu["filter_take"] = cpu_baseline_filter_take(values, validity, mask, n, args.cpu_sample_rows, args.cpu_budget_s)
        if args.extras and not EMU:
            for name, fn in (("hash_sum", lambda: cpu_baseline_hash_sum(min(args.hash_sum_rows, args.cpu_groupby_rows), args.groups, args.cpu_budget_s)),
                             ("sort_indices", lambda: cpu_baseline_sort(min(args.sort_rows, args.cpu_sort_rows))),
                             ("config3", lambda: cpu_baseline_cast_greater(args.stream_rows, device))):
                try:
                    cpu[name] = fn()
                except Exception as e:
                    cpu[name] = {"error": f"{type(e).__name__}: {e}"[:200]}
    _CPU_PRE.update(cpu)

    # ---- the Python mirror of the C ABI (arrow_amd.compute): the loop the kernel events are taken in
    def step():
        out = amd.compute.filter(dv, dm)
        idx = amd.compute.get_take_indices(dm)
        tk = amd.compute.take(dv, idx, boundscheck=False)
        return out, idx, tk

    def time_mirror():
        out = idx = tk = None
        for _ in range(args.warmup):
            out, idx, tk = step()
        timer = _WallTimer() if EMU else tracing.KernelTimer(device)
        tracing.install(timer)
        _barrier(world)
        _sync(device)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out, idx, tk = step()
        _sync(device)
        _barrier(world)
        mirror_elapsed = time.perf_counter() - t0
        tracing.install(None)
        return out, idx, tk, timer, _max_over_ranks(mirror_elapsed, world, device)

    # a plain run times the one route `value` stands for; --full times the mirror first (kernel events, roofline) and
    # diffs the two routes' results
    out = idx = tk = timer = mirror_elapsed = None
    if args.full or EMU:
        out, idx, tk, timer, mirror_elapsed = time_mirror()

    # ---- the drop-in route: the same step through UNMODIFIED pyarrow.compute on device-resident
    # arrays — Arrow's dispatch, executors and output allocation in the timed region; this is `value`.  The arrays are
    # the very HBM buffers above, wrapped without a copy.
    elapsed, api, api_error, cf_check = None, "arrow_amd.compute (Python mirror of the C ABI)", None, None
    cf_last = None           # the drop-in route's filter, row numbers and take of its last timed step
    if not EMU:
        try:
            import pyarrow as pa
            import pyarrow.compute as pc

            plug = plugin_session()
            pdv = plug.wrap(pa.int64(), n, values, validity, -1)
            pdm = plug.wrap(pa.bool_(), n, mask)

            def cf_step():
                o = pc.filter(pdv, pdm)                      # array_filter
                rows = pc.indices_nonzero(pdm)               # the mask's row numbers (uint64): what GetTakeIndices is to Take
                return o, rows, pc.take(pdv, rows, boundscheck=False)

            res = None
            for _ in range(args.warmup):
                res = cf_step()
            g0 = {f: plug.lib.arrow_amd_plugin_calls(f, 1) for f in (b"array_filter", b"array_take")}
            _barrier(world)
            _sync(device)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                res = cf_step()
            _sync(device)
            _barrier(world)
            cf_elapsed = _max_over_ranks(time.perf_counter() - t0, world, device)
            calls = {f.decode(): plug.lib.arrow_amd_plugin_calls(f, 1) - g0[f] for f in g0}
            assert calls["array_filter"] >= 2 * args.steps and calls["array_take"] >= args.steps, calls
            o, rows, t2 = res
            del res
            if out is not None:
                # the two routes agree: lengths, null counts, wrap-around sums of the valid values (device reductions)
                cf_check = bool(len(o) == out.length == len(t2) == len(rows) and
                                pc.sum(o).as_py() == pc.sum(t2).as_py() == pc.sum(plug.wrap(pa.int64(), out.length, out.data, out.validity, -1)).as_py())
            api = "pyarrow.compute on device-resident arrays through libarrow_amd_plugin.so: pc.filter + pc.indices_nonzero + pc.take"
            elapsed, cf_last = cf_elapsed, (o, rows, t2)
            del o, rows, t2
        except Exception as e:
            api_error = f"{type(e).__name__}: {e}"[:300]
    if elapsed is None:
        # the emulated backend, or the drop-in route failed: `value` is the mirror's
        if mirror_elapsed is None:
            out, idx, tk, timer, mirror_elapsed = time_mirror()
        elapsed = mirror_elapsed
    selected = out.length if out is not None else len(cf_last[0])
    if args.dump_outputs and rank == 0:
        got = [plug.to_numpy(a) for a in cf_last] if cf_last is not None else [a.to_numpy() for a in (out, idx, tk)]
        dump_outputs(args.dump_outputs, dict(zip(("filter", "take_indices", "take"), got)))
        del got
    cf_last = None

    result = {
        "metric": "filter_take_mrows_per_s",
        "value": round(world * n * args.steps / elapsed / 1e6, 2),
        "unit": "Mrows/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic",
        "api": api,
        **({"api_error_fell_back_to_the_mirror": api_error} if api_error else {}),
        **({"callfunction_results_equal_the_mirrors": cf_check} if cf_check is not None else {}),
        **({"python_mirror": {"what": "the same step through arrow_amd.compute (ctypes over the C ABI): filter + get_take_indices (uint32) + take",
                              "ms_per_step": round(mirror_elapsed / args.steps * 1e3, 4),
                              "mrows_per_s": round(world * n * args.steps / mirror_elapsed / 1e6, 2)}} if args.full else {}),
        "config": {
            "workload": f"Filter+Take int64[{n}] + validity ({args.null_p:.0%} null), boolean mask "
                        f"{args.selectivity:.0%} true, FilterOptions::DROP; take indices = the mask's row numbers "
                        "(monotonic; indices_nonzero: uint64 through CallFunction, GetTakeIndices: uint32 in the mirror), "
                        "no boundscheck; inputs = splitmix64 streams of SURVEY.md 8(d) (seeds 1,2,3)",
            "rows": n, "selected_rows": int(selected), "parallelism": "replicas" if world > 1 else "single-gpu",
        },
    }
    if not args.full:
        return result

    filt_ms = timer.elapsed_ms("arx_filter_exec")
    take_ms = timer.elapsed_ms("arx_take")
    m2i_ms = timer.elapsed_ms("arx_mask_to_indices")
    avg_filter_ms = float(np.mean(filt_ms))
    alg_bytes = 8 * n + n / 8 + n / 8 + 8 * selected + selected / 8
    achieved = alg_bytes / (avg_filter_ms * 1e-3) / 1e9
    take_bytes = selected * 20.25
    result["roofline"] = {
        "bound": "hbm", "kernel": "compact_sparse_kernel<8> (arx_filter_exec)",
        "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4),
        "algorithmic_bytes_per_launch": int(alg_bytes),
        "avg_kernel_ms": round(avg_filter_ms, 4),
        "traffic": load_traffic("filter", n),
        "traffic_source": "profiles/filter_traffic.json (this round's record run: profiles/r06_record_pmc_fetch_write_and_calibration.txt)",
        "timed_in": "HIP events around the C-ABI calls of the mirror loop (the plugin launches the same entry point on its own stream)",
    }
    result["kernel_ms"] = {"arx_filter_exec": round(avg_filter_ms, 4),
                           "arx_mask_to_indices": round(float(np.mean(m2i_ms)), 4),
                           "arx_take": round(float(np.mean(take_ms)), 4),
                           "take_algorithmic_GBps": round(take_bytes / max(float(np.mean(take_ms)), 1e-9) / 1e6, 1)}
    if rank == 0 and not EMU:
        try:
            ceiling = copy_ceiling(amd, device)
            result["roofline"]["copy_ceiling_GBps"] = ceiling
            # real bytes over a real-bytes ceiling (lines without a selected row are never fetched: the counter traffic,
            # not the full-scan convention, is what the copy ceiling compares with)
            tr = result["roofline"]["traffic"]
            if isinstance(tr, (int, float)) and tr:
                result["roofline"]["real_bytes_frac_of_copy_ceiling"] = round(tr / (avg_filter_ms * 1e-3) / 1e9 / ceiling, 4)
                # `frac` prices SURVEY 8(d)'s full-scan bytes; this is the same launch in the bytes that crossed the memory
                # interface (128-byte value lines without a selected row are never fetched), against the same 8 TB/s
                result["roofline"]["real_bytes_frac_of_peak"] = round(tr / (avg_filter_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        except Exception as e:
            result["roofline"]["copy_ceiling_GBps"] = f"{type(e).__name__}: {e}"[:200]
    if rank == 0 and world == 1:
        result["parity_spot_check"] = "ok" if parity_spot_check(amd, values, validity, mask, n) else "MISMATCH"
        if "filter_take" in cpu:
            result["cpu_baseline"] = cpu["filter_take"]
    del out, idx, tk
    watchdog = None
    if args.extras and world > 1:
        # The sharded legs below are the only part of this file that depends on collectives with
        # uneven splits; should one of them wedge on a node, the headline measured above must not be
        # lost with it: after --extras-timeout seconds rank 0 prints the line it has and every rank exits.
        watchdog = _ExtrasWatchdog(rank, result, args.extras_timeout)
        watchdog.start()
    if args.extras:
        del values, validity, mask, dv, dm
        if not EMU:
            torch.cuda.empty_cache()
        if rank == 0 and world == 1:
            try:
                result["other_paths"] = run_other_paths(amd, device, args)
            except Exception as e:
                result["other_paths"] = {"error": f"{type(e).__name__}: {e}"[:300]}
            if not EMU:
                torch.cuda.empty_cache()
        # the second half of BASELINE.json's metric: hash_sum group-by, 4B rows / 10M keys, rows
        # sharded over the N ranks (strong scaling), outside the timed region of `value`
        try:
            result["hash_sum"] = hash_sum_leg(args, rank, world, device, args.hash_sum_rows, 3, 1)
        except Exception as e:  # never lose the headline line to the secondary measurement
            result["hash_sum"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        # configs[4]: array_sort_indices of a 2B-row uint64 array sharded over the N ranks
        try:
            if not EMU:
                torch.cuda.empty_cache()
            result["sort_indices"] = sort_leg(args, rank, world, device, args.sort_rows, 2, 1)
        except Exception as e:
            result["sort_indices"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    if watchdog is not None:
        watchdog.cancel()
    if args.extras and rank == 0 and world == 1:
        # VERDICT r4 "Next round" 2a: the kernels the two legs above are timed on, diffed with the reference's own answer
        hs, so = result.get("hash_sum", {}), result.get("sort_indices", {})
        if "parity_prefix" in hs or "parity_prefix" in so:
            result["parity"] = {"hash_sum_prefix": hs.get("parity_prefix", "not run"), "sort_prefix": so.get("parity_prefix", "not run"),
                                "plan": {"hash_sum": hs.get("parity_plan"), "sort_indices": so.get("parity_plan")},
                                "what": "device result of the timed plan on the first 1e8 rows of the legs' streams vs pyarrow "
                                        "(Table.group_by key-sorted (key, sum); sort_indices index for index)"}
    if args.extras and rank == 0 and world == 1 and not EMU:
        # LAST: registering the plugin re-routes pyarrow's own kernels to the GPU for the rest of the process,
        # so every CPU baseline above had to be taken first
        try:
            torch.cuda.empty_cache()
            values, validity, mask, _ = gen_filter_inputs(args.rows, device, 0, args.null_p, args.selectivity)
            result.setdefault("other_paths", {})["callfunction"] = callfunction_leg(args, values, validity, mask, device)
        except Exception as e:
            result.setdefault("other_paths", {})["callfunction"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    return result


class _ExtrasWatchdog:
    """Prints the headline line and ends the process if the multi-rank extras do not finish."""

    def __init__(self, rank, result, seconds):
        import threading

        self.rank, self.result, self.seconds = rank, result, seconds
        self.done = threading.Event()
        self.thread = threading.Thread(target=self._run, daemon=True)

    def start(self):
        self.thread.start()

    def cancel(self):
        self.done.set()

    def _run(self):
        if self.done.wait(self.seconds):
            return
        if self.rank == 0:
            line = dict(self.result)
            for leg in ("hash_sum", "sort_indices"):
                line.setdefault(leg, {"error": f"did not finish within {self.seconds} s (watchdog)"})
            os.write(_JSON_FD[0], (json.dumps(line) + "\n").encode())
        else:
            time.sleep(2.0)   # let rank 0 print first
        os._exit(0)


def run_other_paths(amd, device, args):
    """Single-GPU numbers for the other rows of SURVEY.md section 8 (not `value`): config 3 at its stated size
    with the survey's value mix, the secondary configurations of 8(d), and the same calls through the Arrow
    plugin (CallFunction on device-resident pyarrow arrays)."""
    from arrow_amd import tracing

    out = {}
    n = args.stream_rows
    # ---- config 3a: cast(float64 -> float32), survey mix (overflow -> inf, float32 subnormals, NaN, +-0)
    x = gen_cast_mix(n, device)
    ax = amd.Array(amd.array.float64, n, [None, x.view(torch.uint8)], 0, 0)
    ms = _time_gpu(lambda: amd.compute.cast(ax, amd.array.float32))
    got = amd.compute.cast(ax, amd.array.float32)
    leg = {"rows": n, "ms": round(ms, 4), "algorithmic_GBps": round(12 * n / ms / 1e6, 1),
           "roofline_frac": round(12 * n / ms / 1e6 / HBM_PEAK_GBS, 4),
           "values": "survey 8(d) 3a mix (90% N(0,1), 5% >FLT_MAX, 4% f32-subnormal, 1% special)"}
    # (a sample against torch's conversion — the same round-to-nearest-even — stays as the check of runs without the
    #  reference's result, --no-cpu-baseline and the emulated backend; the line below it is the check proper)
    f = got.data[: 4 * min(n, 1 << 20)].view(torch.float32)
    ref32 = x[: min(n, 1 << 20)].to(torch.float32)
    leg["bit_exact_vs_round_to_nearest_even_sample"] = bool(((f == ref32) | (torch.isnan(f) & torch.isnan(ref32))).all())
    del f, ref32
    cpu3 = _CPU_PRE.get("config3", {})
    if "cast_f64_f32" in _CPU_REF:      # the reference's own result for EVERY row (north star: within 1 ULP; 0 observed)
        ref = torch.from_numpy(_CPU_REF.pop("cast_f64_f32").view(np.int32))
        dev_bits = got.data[: 4 * n].view(torch.int32)
        worst, nan_mismatch = 0, 0
        for b in range(0, n, 1 << 28):
            e = min(n, b + (1 << 28))
            r = ref[b:e].to(device)
            g = dev_bits[b:e]
            rn, gn = torch.isnan(r.view(torch.float32)), torch.isnan(g.view(torch.float32))
            nan_mismatch += int((rn != gn).sum().item())
            diff = (r.to(torch.int64) - g.to(torch.int64)).abs()[~(rn | gn)]
            worst = max(worst, int(diff.max().item()) if diff.numel() else 0)
            del r, g, rn, gn, diff
        leg["vs_pyarrow_cast_all_rows"] = {"max_ulp_distance": worst, "nan_placement_mismatches": nan_mismatch,
                                           "equal": bool(worst == 0 and nan_mismatch == 0)}
        del ref
    if "cast_f64_f32" in cpu3:
        leg["cpu_baseline"] = cpu3["cast_f64_f32"]
    elif "error" in cpu3:
        leg["cpu_baseline"] = cpu3
    if not EMU:      # the same call through UNMODIFIED pyarrow.compute on the device-resident array (CallFunction -> the shim -> the C ABI)
        try:
            import pyarrow as pa
            import pyarrow.compute as pc

            plug = plugin_session()
            px = plug.wrap(pa.float64(), n, x.view(torch.uint8))
            g0 = plug.lib.arrow_amd_plugin_calls(b"cast", 1)
            cf_ms = _time_gpu(lambda: pc.cast(px, pa.float32(), safe=False))
            leg["through_pyarrow_compute"] = {"ms": round(cf_ms, 4), "roofline_frac": round(12 * n / cf_ms / 1e6 / HBM_PEAK_GBS, 4),
                                              "gpu_kernel_calls": int(plug.lib.arrow_amd_plugin_calls(b"cast", 1) - g0)}
            del px
        except Exception as e:
            leg["through_pyarrow_compute"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    out["cast_f64_f32"] = leg
    del x, ax, got
    # ---- config 3b: greater(float64, float64)
    a = gen_normal(n, device, 6)
    b = gen_normal(n, device, 7)
    aa = amd.Array(amd.array.float64, n, [None, a.view(torch.uint8)], 0, 0)
    ab = amd.Array(amd.array.float64, n, [None, b.view(torch.uint8)], 0, 0)
    ms = _time_gpu(lambda: amd.compute.greater(aa, ab))
    leg = {"rows": n, "ms": round(ms, 4), "algorithmic_GBps": round(16.125 * n / ms / 1e6, 1),
           "roofline_frac": round(16.125 * n / ms / 1e6 / HBM_PEAK_GBS, 4)}
    if "greater_f64" in _CPU_REF:
        got = amd.compute.greater(aa, ab)
        ref = torch.from_numpy(_CPU_REF.pop("greater_f64")).to(device)
        leg["vs_pyarrow_greater_all_rows"] = {"equal": bool(torch.equal(got.data[: (n + 7) // 8], ref))}
        del got, ref
    if "greater_f64" in cpu3:
        leg["cpu_baseline"] = cpu3["greater_f64"]
    elif "error" in cpu3:
        leg["cpu_baseline"] = cpu3
    if not EMU:
        try:
            import pyarrow as pa
            import pyarrow.compute as pc

            plug = plugin_session()
            pa_a, pa_b = plug.wrap(pa.float64(), n, a.view(torch.uint8)), plug.wrap(pa.float64(), n, b.view(torch.uint8))
            g0 = plug.lib.arrow_amd_plugin_calls(b"greater", 1)
            cf_ms = _time_gpu(lambda: pc.greater(pa_a, pa_b))
            leg["through_pyarrow_compute"] = {"ms": round(cf_ms, 4), "roofline_frac": round(16.125 * n / cf_ms / 1e6 / HBM_PEAK_GBS, 4),
                                              "gpu_kernel_calls": int(plug.lib.arrow_amd_plugin_calls(b"greater", 1) - g0)}
            del pa_a, pa_b
        except Exception as e:
            leg["through_pyarrow_compute"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    out["greater_f64"] = leg
    del a, b, aa, ab
    if not EMU:
        torch.cuda.empty_cache()
    # ---- secondary configurations of 8(d) on the 1B-row source
    n = args.rows
    values, validity, mask, mvalid = gen_filter_inputs(n, device, 0, args.null_p, args.selectivity, mask_null_p=0.05)
    dv = amd.Array(amd.array.int64, n, [validity, values], -1, 0)
    dm = amd.Array(amd.array.bool_, n, [None, mask], 0, 0)
    dmn = amd.Array(amd.array.bool_, n, [mvalid, mask], -1, 0)
    mono = amd.compute.get_take_indices(dm)
    S = mono.length
    m_rand = min(100_000_000, max(1, n // 10))
    ridx = gen_stream(m_rand, device, 0, 5, modulo=n, dtype=torch.int64).to(torch.int32)   # uint32 bit patterns
    di = amd.Array(amd.array.uint32, m_rand, [None, ridx.view(torch.uint8)], 0, 0)
    sec = {}

    def t(name, fn, bytes_alg, span=None):
        """`ms` / `roofline_frac`: the whole operation (count + read-back + allocation + the kernel), as a caller sees it;
        `kernel_ms` / `kernel_roofline_frac` (span given): the dominant kernel alone between HIP events on its stream, the
        way the headline's `roofline` is taken — the difference is the operation's fixed cost, not bandwidth."""
        ms_ = _time_gpu(fn, reps=5, warm=2)
        sec[name] = {"ms": round(ms_, 4), "algorithmic_GBps": round(bytes_alg / ms_ / 1e6, 1),
                     "roofline_frac": round(bytes_alg / ms_ / 1e6 / HBM_PEAK_GBS, 4)}
        if span is not None and not EMU:
            timer = tracing.KernelTimer(device)
            tracing.install(timer)
            try:
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                spans = timer.elapsed_ms(span)
            finally:
                tracing.install(None)
            if spans:
                k = sum(spans) / len(spans)
                sec[name].update({"kernel": span, "kernel_ms": round(k, 4),
                                  "kernel_roofline_frac": round(bytes_alg / k / 1e6 / HBM_PEAK_GBS, 4)})

    t("filter_drop_5pct_mask_nulls", lambda: amd.compute.filter(dv, dmn), 8 * n + 3 * n / 8 + 8.125 * 0.95 * S, "arx_filter_exec")
    t("filter_emit_null_5pct_mask_nulls", lambda: amd.compute.filter(dv, dmn, "emit_null"),
      8 * n + 3 * n / 8 + 8.125 * (0.95 * S + 0.05 * n), "arx_filter_exec")
    t("take_monotonic_boundscheck", lambda: amd.compute.take(dv, mono, boundscheck=True), 20.25 * S)
    t("take_random_uint32", lambda: amd.compute.take(dv, di, boundscheck=False), 20.25 * m_rand, "arx_take")
    for sel in (0.25, 0.50):
        _, _, msel, _ = gen_filter_inputs(n, device, 0, args.null_p, sel)
        dms = amd.Array(amd.array.bool_, n, [None, msel], 0, 0)
        ssel = amd.compute.filter(dv, dms).length
        t(f"filter_drop_selectivity_{int(sel * 100)}pct", lambda: amd.compute.filter(dv, dms),
          8 * n + n / 4 + 8.125 * ssel, "arx_filter_exec")
        del msel, dms
    # take of a 4-column record batch by the monotonic indices (TakeRAR): one launch for all columns
    # (arx_take_columns) vs array_take column after column; 3 more value columns of their own (distinct HBM lines)
    try:
        extra = [gen_stream(n, device, 0, 20 + j) for j in range(3)]
        cols = {"c0": dv, **{f"c{j + 1}": amd.Array(amd.array.int64, n, [validity, e.view(torch.uint8)], -1, 0)
                             for j, e in enumerate(extra)}}
        batch = amd.compute.RecordBatch(cols)
        t("take_record_batch_4_columns_one_launch", lambda: amd.compute.take(batch, mono, boundscheck=False), 4 * 16.25 * S + 4 * S)
        t("take_record_batch_4_columns_per_column",
          lambda: [amd.compute.take(c, mono, boundscheck=False) for c in cols.values()], 4 * 20.25 * S)
        del extra, cols, batch
    except Exception as e:   # (an out-of-memory here must not cost the rest of the line)
        sec["take_record_batch_4_columns"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    out["secondary_configs"] = {"rows": n, "selected_rows": int(S), **sec}
    del values, validity, mask, mvalid, dv, dm, dmn, mono, ridx, di
    if not EMU:
        torch.cuda.empty_cache()
    # ---- sort / hash_sum with 1 % nulls (secondary of configs 4 and 5), single GPU, 2^28 rows
    n2 = min(1 << 28, max(1024, args.sort_rows))
    k = gen_stream(n2, device, 0, 10)
    kv = gen_validity(n2, device, 0, 11, 1)
    ak = amd.Array(amd.array.uint64, n2, [kv, k.view(torch.uint8)], -1, 0)
    ms = _time_gpu(lambda: amd.compute.sort_indices(ak), reps=2, warm=1)
    out["sort_indices_u64_1pct_nulls"] = {"rows": n2, "ms": round(ms, 3), "mrows_per_s": round(n2 / ms / 1e3, 1)}
    ms = _time_gpu(lambda: amd.compute.sort_indices(ak, order="descending"), reps=2, warm=1)
    out["sort_indices_u64_1pct_nulls_descending"] = {"rows": n2, "ms": round(ms, 3), "mrows_per_s": round(n2 / ms / 1e3, 1)}
    del k, kv, ak
    keys = gen_stream(n2, device, 0, 8, modulo=args.groups, dtype=torch.int32)
    vals = gen_stream(n2, device, 0, 9)
    kvb = gen_validity(n2, device, 0, 12, 0)      # 0.1 % null keys would need a per-mille stream: use values' 1 %
    vvb = gen_validity(n2, device, 0, 13, 1)
    kk = amd.Array(amd.array.int32, n2, [kvb, keys.view(torch.uint8)], -1, 0)
    vv = amd.Array(amd.array.int64, n2, [vvb, vals.view(torch.uint8)], -1, 0)
    cap = 1
    while cap < 2 * args.groups + 2:
        cap <<= 1
    ms = _time_gpu(lambda: amd.compute.group_by_sum(kk, vv, capacity=cap), reps=2, warm=1)
    out["hash_sum_1pct_null_values"] = {"rows": n2, "groups": args.groups, "ms": round(ms, 3),
                                        "mrows_per_s": round(n2 / ms / 1e3, 1)}
    del keys, vals, kvb, vvb, kk, vv
    if not EMU:
        torch.cuda.empty_cache()
    return out


def callfunction_leg(args, values, validity, mask, device):
    """The same kernels driven by UNMODIFIED pyarrow.compute / Acero on device-resident pyarrow arrays through the
    registration shim (libarrow_amd_plugin.so): wall ms per call, i.e. Arrow's dispatch + output allocation + the
    host-visible count sync on top of the C-ABI figure."""
    import ctypes

    import pyarrow as pa
    import pyarrow.compute as pc
    from pyarrow import acero

    import arrow_amd as amd

    plug = plugin_session()
    lib, to_device = plug.lib, plug.to_device

    n = min(args.rows, args.callfunction_rows)
    n -= n % 64
    # the HBM buffers themselves as device-resident pyarrow arrays (arrow_amd_wrap_device_memory: no copy)
    dv = plug.wrap(pa.int64(), n, values, validity, -1)
    dm = plug.wrap(pa.bool_(), n, mask)
    res = {"rows": n}

    def timeit(name, fn, reps=5):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
            del r
        res[name] = {"ms_min": round(min(ts) * 1e3, 3), "ms_median": round(sorted(ts)[len(ts) // 2] * 1e3, 3)}

    g0 = {f: lib.arrow_amd_plugin_calls(f, 1) for f in (b"array_filter", b"array_take")}
    timeit("pc.filter(device int64, device mask 10%)", lambda: pc.filter(dv, dm))
    idx = pc.filter(to_device(pa.array(np.arange(n, dtype=np.uint32))), dm)
    timeit("pc.take(device int64, device uint32 indices)", lambda: pc.take(dv, idx, boundscheck=False))
    # the whole headline step through Arrow's own API, nothing of the Python mirror in it: filter, the mask's row numbers
    # (indices_nonzero: what GetTakeIndices is to the reference's Take), take by them
    def step():
        out = pc.filter(dv, dm)
        rows = pc.indices_nonzero(dm)
        return out, pc.take(dv, rows, boundscheck=False)
    try:
        timeit("Filter+Take step through CallFunction: pc.filter + pc.indices_nonzero + pc.take (device arrays)", step)
        res["Filter+Take step through CallFunction: pc.filter + pc.indices_nonzero + pc.take (device arrays)"]["mrows_per_s"] = round(
            n / res["Filter+Take step through CallFunction: pc.filter + pc.indices_nonzero + pc.take (device arrays)"]["ms_min"] / 1e3, 1)
    except Exception as e:
        res["Filter+Take step through CallFunction"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    res["gpu_kernel_calls"] = {f.decode(): int(lib.arrow_amd_plugin_calls(f, 1) - g0[f]) for f in g0}
    del dv, dm, idx
    # group-by through Acero: table_source -> aggregate_rocm (the fused device operator) on device-resident columns
    m = min(n, 1 << 28)
    k = pa.array(gen_stream(m, device, 0, 8, modulo=args.groups, dtype=torch.int32).cpu().numpy())
    v = pa.array(gen_stream(m, device, 0, 9).cpu().numpy())
    dt = pa.table({"k": to_device(k), "v": to_device(v)})
    plan = acero.Declaration.from_sequence([
        acero.Declaration("table_source", acero.TableSourceNodeOptions(dt)),
        acero.Declaration("aggregate_rocm", acero.AggregateNodeOptions([("v", "hash_sum", None, "v_sum")], keys=["k"]))])
    timeit(f"acero table_source -> aggregate_rocm (hash_sum, {m} device rows, {args.groups} keys)",
           lambda: plan.to_table(use_threads=False), reps=3)
    # the same table through table_source_rocm (whole chunks instead of 32Ki-row batches: the nodes downstream run once),
    # alone and with the STOCK FilterNode and ProjectNode in between; beside them the fused kernel on the same rows
    agg_node = acero.Declaration("aggregate_rocm", acero.AggregateNodeOptions([("v", "hash_sum", None, "v_sum")], keys=["k"]))
    plan_r = acero.Declaration.from_sequence([acero.Declaration("table_source_rocm", acero.TableSourceNodeOptions(dt)), agg_node])
    timeit(f"acero table_source_rocm -> aggregate_rocm (hash_sum, {m} device rows, {args.groups} keys)",
           lambda: plan_r.to_table(use_threads=False), reps=3)
    try:
        x = pa.array(np.random.default_rng(13).random(m))
        dtx = pa.table({"x": to_device(x), "k": dt.column("k").chunk(0), "v": dt.column("v").chunk(0)})
        del x
        stages = [acero.Declaration("filter", acero.FilterNodeOptions(pc.field("x") > 0.1)),
                  acero.Declaration("project", acero.ProjectNodeOptions([pc.field("k"), pc.add(pc.field("v"), pc.field("v"))], ["k", "v"])),
                  agg_node]
        for source in ("table_source_rocm", "table_source"):
            plan_f = acero.Declaration.from_sequence([acero.Declaration(source, acero.TableSourceNodeOptions(dtx))] + stages)
            # (round 6: a stock `table_source` over a device-resident table delivers whole chunks with nothing but
            #  arrow_amd_register() called — VERDICT r5 weak 8; the reference SourceNode's 32Ki-row morsels are the opt-out)
            timeit(f"acero {source} -> filter(x > 0.1) -> project(k, v + v) -> aggregate_rocm ({m} device rows)",
                   lambda: plan_f.to_table(use_threads=False), reps=3)
            if source == "table_source":
                if lib.arrow_amd_override_acero_factories(-1) == 0:
                    timeit(f"acero table_source -> filter(x > 0.1) -> project(k, v + v) -> aggregate_rocm ({m} device rows), OPT-OUT: the stock source's 32Ki-row morsels",
                           lambda: plan_f.to_table(use_threads=False), reps=1)
                    lib.arrow_amd_override_acero_factories(0)
                # every node by its STOCK name, registration only: the guard in front of the CPU Grouper builds aggregate_rocm
                plan_d = acero.Declaration.from_sequence(
                    [acero.Declaration("table_source", acero.TableSourceNodeOptions(dtx)), stages[0], stages[1],
                     acero.Declaration("aggregate", acero.AggregateNodeOptions([("v", "hash_sum", None, "v_sum")], keys=["k"]))])
                timeit(f"acero table_source -> filter(x > 0.1) -> project(k, v + v) -> aggregate, STOCK node names, only arrow_amd_register() called ({m} device rows)",
                       lambda: plan_d.to_table(use_threads=False), reps=3)
                del plan_d
                # the stock source with coalesce_rocm behind it: its 32Ki-row batches are joined again (no copy: they
                # are consecutive slices of the table's arrays) before the filter sees them
                plan_c = acero.Declaration.from_sequence(
                    [acero.Declaration(source, acero.TableSourceNodeOptions(dtx)),
                     acero.Declaration("coalesce_rocm", acero.FilterNodeOptions(pc.scalar(True)))] + stages)
                timeit(f"acero table_source -> coalesce_rocm -> filter(x > 0.1) -> project(k, v + v) -> aggregate_rocm ({m} device rows)",
                       lambda: plan_c.to_table(use_threads=False), reps=3)
                del plan_c
            if source == "table_source_rocm":
                # the same plan with its result left in HBM (120 MB of keys and sums do not cross PCIe)
                lib.arrow_amd_plugin_set_aggregate_device_output(1)
                timeit(f"acero {source} -> filter(x > 0.1) -> project(k, v + v) -> aggregate_rocm ({m} device rows), result kept in HBM",
                       lambda: plan_f.to_table(use_threads=False), reps=3)
                timeit(f"acero {source} -> aggregate_rocm (hash_sum, {m} device rows, {args.groups} keys), result kept in HBM",
                       lambda: plan_r.to_table(use_threads=False), reps=3)
                lib.arrow_amd_plugin_set_aggregate_device_output(0)
            del plan_f
        # the UNMODIFIED plan — stock node names only — once arrow_amd_override_acero_factories(1) re-routed table_source /
        # aggregate over device-resident tables (plugin/acero_override.inc)
        if lib.arrow_amd_override_acero_factories(1) == 0:
            plan_s = acero.Declaration.from_sequence(
                [acero.Declaration("table_source", acero.TableSourceNodeOptions(dtx)),
                 acero.Declaration("filter", acero.FilterNodeOptions(pc.field("x") > 0.1)),
                 acero.Declaration("project", acero.ProjectNodeOptions([pc.field("k"), pc.add(pc.field("v"), pc.field("v"))], ["k", "v"])),
                 acero.Declaration("aggregate", acero.AggregateNodeOptions([("v", "hash_sum", None, "v_sum")], keys=["k"]))])
            timeit(f"acero table_source -> filter(x > 0.1) -> project(k, v + v) -> aggregate, STOCK node names, factory override on ({m} device rows)",
                   lambda: plan_s.to_table(use_threads=False), reps=3)
            lib.arrow_amd_override_acero_factories(0)
            del plan_s
        else:
            res["acero stock node names with the factory override"] = {"error": lib.arrow_amd_plugin_last_error().decode()[:300]}
        # what a plan costs before it touches a row: the same four nodes over 1024 rows (plan construction, task
        # scheduling, the sink and to_table included)
        tiny = pa.table({name: dtx.column(name).chunk(0).slice(0, 1024) for name in ("x", "k", "v")})
        plan_t = acero.Declaration.from_sequence([acero.Declaration("table_source_rocm", acero.TableSourceNodeOptions(tiny))] + stages)
        timeit("acero table_source_rocm -> filter -> project -> aggregate_rocm over 1024 device rows (the plan's fixed cost)",
               lambda: plan_t.to_table(use_threads=False), reps=5)
        del dtx, tiny, plan_t
    except Exception as e:
        res["table_source_rocm -> filter -> project -> aggregate_rocm"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    kt = gen_stream(m, device, 0, 8, modulo=args.groups, dtype=torch.int32)
    vt = gen_stream(m, device, 0, 9)
    kk = amd.Array(amd.array.int32, m, [None, kt.view(torch.uint8)], 0, 0)
    vv = amd.Array(amd.array.int64, m, [None, vt.view(torch.uint8)], 0, 0)
    cap = 1
    while cap < 2 * args.groups + 2:
        cap <<= 1
    res[f"fused kernel on the same rows (arx_groupby_sum_i64, {m} rows)"] = {
        "ms": round(_time_gpu(lambda: amd.compute.group_by_sum(kk, vv, capacity=cap), reps=3, warm=1), 3)}
    del dt, plan, plan_r, kt, vt, kk, vv
    # the same operator over columns WITH nulls: 32K-row batches are staged many at a time, their validity by
    # arx_bitmap_copy_segments (before: every batch with nulls consumed on its own)
    try:
        m2 = min(m, 1 << 26)
        rng = np.random.default_rng(11)
        vn = pa.array(v.to_numpy()[:m2], mask=rng.random(m2) < 0.1)
        dtn = pa.table({"k": to_device(k.slice(0, m2)), "v": to_device(vn)})
        plan_n = acero.Declaration.from_sequence([
            acero.Declaration("table_source", acero.TableSourceNodeOptions(dtn)),
            acero.Declaration("aggregate_rocm", acero.AggregateNodeOptions([("v", "hash_sum", None, "v_sum")], keys=["k"]))])
        timeit(f"acero table_source -> aggregate_rocm (hash_sum, {m2} device rows, 10 % null values)",
               lambda: plan_n.to_table(use_threads=False), reps=3)
        del dtn, plan_n, vn
    except Exception as e:
        res["aggregate_rocm with nulls"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    del k, v
    # Parquet -> HBM through the plugin's column-chunk reader (f4): one Snappy file, three int64 columns (dictionary +
    # nulls, full-range PLAIN, compressible PLAIN), against pyarrow's reader on all threads (host result)
    try:
        import tempfile

        import pyarrow.parquet as pq

        pn = 8_000_000
        rng = np.random.default_rng(12)
        pt = pa.table({"k": pa.array(rng.integers(0, 5000, pn), mask=rng.random(pn) < 0.1),
                       "v": pa.array(rng.integers(-2**62, 2**62, pn)),
                       "w": pa.array(np.cumsum(rng.integers(-3, 4, pn)))})
        pt = pt.cast(pa.schema([pa.field("k", pa.int64()), pa.field("v", pa.int64()), pa.field("w", pa.int64(), nullable=False)]))
        ppath = os.path.join(tempfile.mkdtemp(), "bench.parquet")
        pq.write_table(pt, ppath, row_group_size=pn, compression="snappy", use_dictionary=["k"], data_page_version="2.0")
        lib.arrow_amd_parquet_read_column.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

        def read_columns():
            cols = []
            for j in range(3):
                c_dev, c_schema = ctypes.create_string_buffer(128), ctypes.create_string_buffer(72)
                rc = lib.arrow_amd_parquet_read_column(ppath.encode(), 0, j, ctypes.addressof(c_dev), ctypes.addressof(c_schema))
                assert rc == 0, lib.arrow_amd_plugin_last_error()
                cols.append(pa.Array._import_from_c_device(ctypes.addressof(c_dev), ctypes.addressof(c_schema)))
            return cols

        name = f"parquet -> HBM, arrow_amd_parquet_read_column, 3 x {pn} int64 rows, Snappy, {os.path.getsize(ppath) >> 20} MB file"
        timeit(name, read_columns, reps=5)
        lib.arrow_amd_parquet_read_columns.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                       ctypes.c_void_p]

        def read_columns_at_once():      # the three chunks on the plugin's worker threads, kernels and copies overlapping
            c_devs, c_schemas = ctypes.create_string_buffer(128 * 3), ctypes.create_string_buffer(72 * 3)
            rc = lib.arrow_amd_parquet_read_columns(ppath.encode(), 0, (ctypes.c_int * 3)(0, 1, 2), 3, ctypes.addressof(c_devs),
                                                    ctypes.addressof(c_schemas))
            assert rc == 0, lib.arrow_amd_plugin_last_error()
            return [pa.Array._import_from_c_device(ctypes.addressof(c_devs) + 128 * i, ctypes.addressof(c_schemas) + 72 * i)
                    for i in range(3)]

        read_columns_at_once()
        timeit(name.replace("arrow_amd_parquet_read_column,", "arrow_amd_parquet_read_columns (3 chunks at once),"),
               read_columns_at_once, reps=5)
        t0 = time.perf_counter()
        pq.read_table(ppath, use_threads=True)
        t1 = time.perf_counter()
        pq.read_table(ppath, use_threads=True)
        res[name]["pyarrow_read_table_all_threads_ms"] = round(min(t1 - t0, time.perf_counter() - t1) * 1e3, 3)
        os.remove(ppath)
    except Exception as e:
        res["parquet -> HBM"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    return res


def hash_sum_leg(args, rank, world, device, rows_total, steps, warmup):
    sec, rows, groups_out, checksum, ok = measure_hash_sum(rank, world, device, rows_total, args.groups, steps, warmup)
    per_gpu = 12 * rows / world / sec / 1e9
    leg = {"rows": rows, "groups": groups_out, "n_gpus": world, "ms": round(sec * 1e3, 3),
           "mrows_per_s": round(rows / sec / 1e6, 1), "scaling": "strong",
           "exchange": "1 all-reduce of the sampled key range -> local range-partitioned aggregate -> ONE all-to-all of dense partition blocks (sizes known: no count exchange) + 1 status all-reduce -> vector-add merge" if world > 1 else "none (one rank)",
           "checksum_matches_sum_of_values": ok,
           "stage_ms_max_over_ranks_untimed_run": _LAST_STAGES.get("hash_sum"),
           "plan": _hash_sum_plan_counters(),
           "roofline": {"bound": "hbm", "kernel": "arx_groupby_range_sum_i64_consume (lines plan: gbl_scatter_kernel [write-combined range scatter, whole 128-byte lines of 12 records] + gbl_aggregate_kernel [direct-indexed LDS tables])",
                        "achieved": round(per_gpu, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(per_gpu / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_row": 12,
                        "traffic": load_traffic("groupby", rows // world, form="lines"),
                        "traffic_source": "profiles/groupby_traffic.json (this round's FETCH_SIZE x 2 + WRITE_SIZE passes: profiles/r06_record_sort_groupby_pmc_fetch_write.txt)"}}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not EMU:
        if "hash_sum" in _CPU_PRE:      # taken before the plugin was registered (run_filter_take)
            leg["cpu_baseline"] = _CPU_PRE["hash_sum"]
        else:
            try:
                leg["cpu_baseline"] = cpu_baseline_hash_sum(min(rows, args.cpu_groupby_rows), args.groups, args.cpu_budget_s)
            except Exception as e:
                leg["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        if "hash_sum" in _CPU_REF:
            try:
                leg["parity_prefix"], leg["parity_plan"] = parity_hash_sum_prefix(device, args.groups)
            except Exception as e:
                leg["parity_prefix"] = f"ERROR {type(e).__name__}: {e}"[:300]
        if not EMU:
            try:
                torch.cuda.empty_cache()
                leg["through_acero"] = acero_hash_sum_full(device, rows, args.groups)
            except Exception as e:
                leg["through_acero"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    return leg


def _hash_sum_plan_counters():
    """Which plan the group-by's passes took in this process so far (arx_get_counter): the roofline's kernel names are
    the lines plan's, and a line measured on another plan must say so."""
    import arrow_amd as amd

    lib = amd._lib.get_lib()
    return _counters(lib, ["groupby_slices_lines", "groupby_lines_fallbacks", "groupby_lines_declined", "groupby_slices_wide",
                           "groupby_slices_rooms", "groupby_slices_two_level"])


# ranks at which the sharded array_sort_indices is SLOWER than the single-GPU sort by this repo's own stage measurements
# (profiles/r06_v_virtual_rank_stage_table_sort_records_sampled_splitters.txt: per rank 30.2 ms at P = 2 against 23.1 ms on one GPU —
# every row crosses the wire as a 12-byte record and the receiver sorts records, not words; 16.5 ms at P = 4, 9.0 ms at P = 8): the
# leg declines there instead of printing a slower number (VERDICT r5 "Next round" 2).  --force-sharded-sort runs it anyway.
SORT_DECLINED_WORLDS = {2: "per-rank stages 30.2 ms (sampled window + splitters 0.4 + partition 5.9 + exchange of 6 GB ~5.6 + record sort 18.3) "
                           "against 23.1 ms for the whole sort on one GPU (profiles/r06_v_virtual_rank_stage_table_sort_records_sampled_splitters.txt)"}


def sort_leg(args, rank, world, device, rows_total, steps, warmup):
    if world in SORT_DECLINED_WORLDS and not getattr(args, "force_sharded_sort", False):
        return {"declined": f"array_sort_indices sharded over {world} GPUs loses to one GPU: " + SORT_DECLINED_WORLDS[world] +
                            "; the sharded sort is for 4 or more ranks (or inputs that are already sharded): --force-sharded-sort measures it anyway",
                "rows": rows_total, "n_gpus": world}
    sec, rows, ok = measure_sort(rank, world, device, rows_total, steps, warmup)
    per_gpu = 16 * rows / world / sec / 1e9
    leg = {"rows": rows, "n_gpus": world, "ms": round(sec * 1e3, 3), "mrows_per_s": round(rows / sec / 1e6, 1),
           "scaling": "strong",
           "exchange": "1 all-reduce (sampled key window) + 1 all-reduce (sampled splitter histogram) + 1 all-gather of the block sizes + ONE all-to-all(v) of 12-byte {key, global row} records; the receiver sorts its records where they lie (arx_sort_records)" if world > 1 else "none (one rank)",
           "permutation_and_order_checks": ok,
           "stage_ms_max_over_ranks_untimed_run": _LAST_STAGES.get("sort_indices"),
           "roofline": {"bound": "hbm", "kernel": "arx_sort_indices (wide form on 8-byte words: msdw_scatter1wc2 [level 1 write-combined by appending: whole 128-byte lines] + msdw_scatter2w + msd_bucket2w [LDS finish])",
                        "achieved": round(per_gpu, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(per_gpu / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_row": 16,
                        "traffic": load_traffic("sort", rows // world, form="rec8")}}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not EMU:
        if "sort_indices" in _CPU_PRE:
            leg["cpu_baseline"] = _CPU_PRE["sort_indices"]
        else:
            try:
                leg["cpu_baseline"] = cpu_baseline_sort(min(rows, args.cpu_sort_rows))
            except Exception as e:
                leg["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        if "sort_indices" in _CPU_REF:
            try:
                leg["parity_prefix"], leg["parity_plan"] = parity_sort_prefix(device)
            except Exception as e:
                leg["parity_prefix"] = f"ERROR {type(e).__name__}: {e}"[:300]
    return leg


_CPU_PRE = {}          # CPU baselines taken before the plugin was registered (run_filter_take)
_LAST_STAGES = {}      # per-stage ms (max over ranks) of the last sharded legs, filled by the measure_* functions


def _stage_max(ms: dict, world, device) -> dict:
    # a fixed list: ranks may take different local passes (a shard that has to go through the local table has an
    # "export" stage, the others do not), the all-reduce needs the same shape on every rank
    names = ("consume", "export", "partition_rows", "histogram", "partition", "exchange", "merge", "local_sort", "finalize")
    assert set(ms) <= set(names), sorted(ms)
    t = torch.tensor([ms.get(k, -1.0) for k in names], dtype=torch.float64, device=device)
    if world > 1:
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    return {k: round(float(x), 3) for k, x in zip(names, t.tolist()) if x >= 0}


def measure_hash_sum(rank, world, device, rows_total, groups, steps, warmup):
    """Sharded group-by: rank g owns rows [g n, (g+1) n) of the streams (n = rows_total // world).  Returns
    (seconds per step [max over ranks], rows actually processed, groups out, checksum, ok)."""
    import arrow_amd as amd
    from arrow_amd import parallel

    n = rows_total // world
    keys = gen_stream(n, device, rank * n, 8, modulo=groups, dtype=torch.int32)
    vals = gen_stream(n, device, rank * n, 9)
    kk = amd.Array(amd.array.int32, n, [None, keys.view(torch.uint8)], 0, 0)
    vv = amd.Array(amd.array.int64, n, [None, vals.view(torch.uint8)], 0, 0)
    cap = 1
    while cap < 2 * groups + 2:
        cap <<= 1

    def step():
        return parallel.sharded_group_by_sum(kk, vv, cap)

    res = None
    for _ in range(warmup):
        res = None          # the previous result is released first: its buffers are what the next call reuses
        res = step()
    _barrier(world)
    _sync(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        res = None
        res = step()
    _sync(device)
    _barrier(world)
    elapsed = _max_over_ranks(time.perf_counter() - t0, world, device)
    # parity property independent of the sharding: sum of all group sums == wrap-around sum of
    # all values; number of groups == distinct keys
    sums = res[2]
    cs = torch.stack([sums.sum(), vals.sum(), torch.tensor(sums.numel(), device=device, dtype=torch.int64)])
    if world > 1:
        torch.distributed.all_reduce(cs)
    ok = int(cs[0].item()) == int(cs[1].item())
    # one more, UNTIMED run with the stream synchronised between the stages: where the time goes on every rank
    res = None
    st = parallel.Stages(device)
    res = parallel.sharded_group_by_sum(kk, vv, cap, stages=st)
    _LAST_STAGES["hash_sum"] = _stage_max(st.ms, world, device)
    del keys, vals, kk, vv, res
    return elapsed / steps, n * world, int(cs[2].item()), int(cs[0].item()), ok


def measure_sort(rank, world, device, rows_total, steps, warmup):
    """Sharded array_sort_indices (configs[4]): each rank owns rows_total // world contiguous rows of
    a uint64 array; splitters -> one all-to-all -> local sort.  Returns (seconds per step [max over
    ranks], rows processed, ok) where ok = the size-independent properties that can be checked
    without a second exchange: the ranks' slices tile [0, N) and hold a permutation checksum of the
    global row numbers (sum and sum of squares mod 2^64); on one rank also full sortedness."""
    import arrow_amd as amd
    from arrow_amd import parallel

    n = rows_total // world
    keys = gen_stream(n, device, rank * n, 10)
    ak = amd.Array(amd.array.uint64, n, [None, keys.view(torch.uint8)], 0, 0)
    chunk = 1 << 26

    def step():
        return parallel.sharded_sort_indices(ak)

    rows = start = None
    for _ in range(warmup):
        rows = None         # release the previous 8 B/row result first: the next call reuses its buffer
        rows, start = step()
    _barrier(world)
    _sync(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        rows = None
        rows, start = step()
    _sync(device)
    _barrier(world)
    elapsed = _max_over_ranks(time.perf_counter() - t0, world, device)
    rows = None
    st = parallel.Stages(device)          # untimed: per-stage ms with the stream synchronised between the stages
    rows, start = parallel.sharded_sort_indices(ak, stages=st)
    _LAST_STAGES["sort_indices"] = _stage_max(st.ms, world, device)
    total = n * world
    m = int(rows.numel())
    s1, s2 = 0, 0
    for b in range(0, m, chunk):          # wrap-around int64 arithmetic == mod 2^64
        r = rows[b: b + chunk]
        s1 += int(r.sum().item())
        s2 += int((r * r).sum().item())
    cs = torch.tensor([m, s1 % (1 << 63), s2 % (1 << 63)], dtype=torch.int64, device=device)
    starts = torch.zeros(world, dtype=torch.int64, device=device)
    starts[rank] = start
    lens = torch.zeros(world, dtype=torch.int64, device=device)
    lens[rank] = m
    if world > 1:
        torch.distributed.all_reduce(starts)
        torch.distributed.all_reduce(lens)
        parts = [torch.zeros_like(cs) for _ in range(world)]
        torch.distributed.all_gather(parts, cs)
    else:
        parts = [cs]
    got_s1 = sum(int(p[1].item()) for p in parts)
    got_s2 = sum(int(p[2].item()) for p in parts)
    ok = sum(int(p[0].item()) for p in parts) == total
    # the per-rank values were reduced mod 2^63 from wrapped int64 sums: compare mod 2^63
    want_s1 = (total * (total - 1) // 2)
    want_s2 = ((total - 1) * total * (2 * total - 1) // 6)
    ok = ok and (got_s1 - want_s1) % (1 << 63) == 0 and (got_s2 - want_s2) % (1 << 63) == 0
    pos = 0
    for r_ in range(world):
        ok = ok and int(starts[r_].item()) == pos
        pos += int(lens[r_].item())
    if world == 1:
        for b in range(0, m - 1, chunk):
            e = min(m, b + chunk + 1)
            kk = keys[rows[b:e]] ^ (-2**63)
            ok = ok and bool((kk[1:] >= kk[:-1]).all())
    del keys, ak, rows
    return elapsed / steps, total, bool(ok)


def run_hash_sum(args, rank, world, device):
    leg = hash_sum_leg(args, rank, world, device, args.rows, args.steps, args.warmup)
    return {
        "metric": "hash_sum_mrows_per_s", "value": leg["mrows_per_s"],
        "unit": "Mrows/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": leg["ms"], "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "int64", "data": "synthetic",
        "config": {"workload": f"hash_sum(int64) GROUP BY int32, {leg['rows']} rows, {args.groups} distinct keys "
                               "(splitmix64 streams, seeds 8/9)",
                   "rows": leg["rows"], "groups_out": leg["groups"],
                   "checksum_matches_sum_of_values": leg["checksum_matches_sum_of_values"],
                   "parallelism": f"row shards x{world} + one all-to-all of partials"},
        "roofline": leg["roofline"], **({"cpu_baseline": leg["cpu_baseline"]} if "cpu_baseline" in leg else {}),
    }


def run_sort(args, rank, world, device):
    args.force_sharded_sort = True      # (--workload sort_indices asks for this very measurement)
    leg = sort_leg(args, rank, world, device, args.rows, args.steps, args.warmup)
    return {
        "metric": "sort_indices_mrows_per_s", "value": leg["mrows_per_s"],
        "unit": "Mrows/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": leg["ms"], "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "uint64", "data": "synthetic",
        "config": {"workload": f"array_sort_indices uint64[{leg['rows']}] (splitmix64 stream, seed 10)",
                   "rows": leg["rows"], "permutation_and_order_checks": leg["permutation_and_order_checks"],
                   "parallelism": f"row shards x{world} + one all-to-all of (key, row) records"},
        "roofline": leg["roofline"], **({"cpu_baseline": leg["cpu_baseline"]} if "cpu_baseline" in leg else {}),
    }


# ------------------------------------------------------------------ launcher
def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n_ranks: int, argv: list) -> int:
    """`python bench.py --gpus N` with no launcher around it: start the N ranks (one process per GPU), pass rank 0's
    stdout through (the JSON line), wait for all; a failing rank ends the others (by PID)."""
    port = _free_port()
    procs = []
    for r in range(n_ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_ranks), LOCAL_WORLD_SIZE=str(n_ranks),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    alive = set(range(n_ranks))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code
                log(f"[bench launcher] rank {r} exited with {code}; stopping the other ranks")
                for o in alive:
                    procs[o].terminate()
        time.sleep(0.05)
    return rc


def main():
    global EMU
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="filter_take", choices=["filter_take", "hash_sum", "sort_indices"])
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--groups", type=int, default=10_000_000)
    ap.add_argument("--hash-sum-rows", dest="hash_sum_rows", type=int, default=4_000_000_000)
    ap.add_argument("--sort-rows", dest="sort_rows", type=int, default=2_000_000_000)
    ap.add_argument("--stream-rows", dest="stream_rows", type=int, default=1_000_000_000,
                    help="rows of the cast / greater legs (config 3)")
    ap.add_argument("--callfunction-rows", dest="callfunction_rows", type=int, default=1_000_000_000)
    ap.add_argument("--extras-timeout", dest="extras_timeout", type=float, default=300.0)
    ap.add_argument("--selectivity", type=float, default=0.10)
    ap.add_argument("--null-p", dest="null_p", type=float, default=0.10)
    ap.add_argument("--cpu-sample-rows", type=int, default=1_000_000_000)   # the same N where RAM allows (8 GB)
    ap.add_argument("--cpu-groupby-rows", dest="cpu_groupby_rows", type=int, default=100_000_000)
    ap.add_argument("--cpu-sort-rows", dest="cpu_sort_rows", type=int, default=100_000_000)
    ap.add_argument("--cpu-budget-s", type=float, default=12.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", dest="extras", action="store_false")
    ap.add_argument("--force-sharded-sort", dest="force_sharded_sort", action="store_true",
                    help="measure the sharded sort_indices leg at rank counts where it is known to lose to one GPU")
    ap.add_argument("--option", action="append", default=[], help="name=value for arx_set_option")
    ap.add_argument("--backend", default="hip", choices=["hip", "emu"],
                    help="emu = CPU tensors + gloo + the SIMT emulator of tests/emu (plumbing tests only)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the mirror loop with its kernel events and roofline, the copy "
                         "ceiling, the parity spot check, the CPU baselines and the other paths and sharded legs")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR", default=None,
                    help="write the timed path's outputs of its last step to DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.dump_outputs and args.workload != "filter_take":
        ap.error("--dump-outputs is implemented for --workload filter_take")
    if args.rows is None:
        args.rows = {"filter_take": 1_000_000_000, "hash_sum": 4_000_000_000, "sort_indices": 2_000_000_000}[args.workload]
    EMU = args.backend == "emu"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if not EMU:
            assert torch.cuda.is_available(), "bench.py needs HIP devices (no CPU fallback exists)"
            have = torch.cuda.device_count()
            if have < args.gpus:
                log(f"[bench launcher] --gpus {args.gpus} but only {have} device(s) visible")
                sys.exit(2)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # stdout carries exactly ONE line — the JSON result.  Everything else any layer below may print there (a compiler
    # command line when the plugin is rebuilt, library chatter) is sent to stderr for the whole run.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    _JSON_FD[0] = json_fd
    if EMU:
        device = torch.device("cpu")
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
        import arrow_amd as amd
        from arrow_amd import _lib, array
        from tests.emu.build_emu import build as build_emu      # test plumbing: kernel sources under the emulator

        _lib._lib = _lib.load(build_emu())
        array.set_default_device("cpu")
    else:
        assert torch.cuda.is_available(), "bench.py needs a HIP device (no CPU fallback exists)"
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            torch.distributed.init_process_group("nccl", device_id=device)
        import arrow_amd as amd
    lib = amd._lib.get_lib()
    for kv in args.option:
        k, v = kv.split("=")
        assert lib.arx_set_option(k.encode(), int(v)) == 0, kv

    if args.workload == "filter_take":
        result = run_filter_take(args, rank, world, device)
    elif args.workload == "hash_sum":
        result = run_hash_sum(args, rank, world, device)
    else:
        result = run_sort(args, rank, world, device)
    if rank == 0:
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(result) + "\n").encode())
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
