"""bench.py's plain run and --dump-outputs on the emulated backend: a plain line carries the headline fields and nothing
that --full adds, the dumped arrays are the filter / take step of the splitmix64 streams (restated in numpy here), and a
--full run with the same arguments dumps the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 20000


def _bench(extra, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--backend", "emu", "--rows", str(ROWS), "--steps", "3",
           "--warmup", "1"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def _want():
    """The step restated on the host: values r(i,1), validity r(i,3) % 100 >= 10, mask r(i,2) % 100 < 10."""
    sys.path.insert(0, ROOT)
    import bench

    vals = bench.splitmix64_np(0, ROWS, 1).view(np.int64)
    valid = bench.splitmix64_np(0, ROWS, 3) % np.uint64(100) >= 10
    rows = np.flatnonzero(bench.splitmix64_np(0, ROWS, 2) % np.uint64(100) < 10)
    return vals[rows], valid[rows], rows


def _hi_lo(v):
    return np.stack([(v >> 32).astype(np.float64), (v & 0xFFFFFFFF).astype(np.float64)], axis=-1)


def test_plain_line_is_the_headline_only(tmp_path):
    line = _bench([], tmp_path)
    assert line["metric"] == "filter_take_mrows_per_s" and line["unit"] == "Mrows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int64" and line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value and ms_per_step are the same measurement: rows per step over the time of one step
    assert abs(line["value"] - ROWS / line["ms_per_step"] / 1e3) <= 0.01 * line["value"] + 0.01
    assert line["config"]["rows"] == ROWS and line["config"]["selected_rows"] == len(_want()[2])
    for key in ("roofline", "kernel_ms", "python_mirror", "parity_spot_check", "cpu_baseline", "other_paths", "hash_sum",
                "sort_indices"):
        assert key not in line, key


def test_dump_outputs_are_the_step_and_equal_under_full(tmp_path):
    plain, full = tmp_path / "plain", tmp_path / "full"
    _bench(["--dump-outputs", str(plain)], tmp_path)
    line = _bench(["--full", "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(full)], tmp_path)
    assert line["parity_spot_check"] == "ok" and "roofline" in line
    got, again = _load(plain), _load(full)
    assert sorted(got) == sorted(again) == sorted(
        ["checksums"] + [f"{o}{s}" for o in ("filter", "take_indices", "take") for s in ("", "_valid", "_rows")])
    for name in got:
        assert got[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(got[name], again[name]), name
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    vals, valid, rows = _want()
    s = len(rows)
    assert np.array_equal(got["filter_rows"], np.arange(s))
    for name in ("filter", "take"):
        assert np.array_equal(got[name], _hi_lo(np.where(valid, vals, 0))), name
        assert np.array_equal(got[f"{name}_valid"], valid.astype(np.float32)), name
    assert np.array_equal(got["take_indices"], _hi_lo(rows.astype(np.int64)))
    assert np.array_equal(got["take_indices_valid"], np.ones(s, np.float32))
    total = int(np.where(valid, vals, 0).view(np.uint64).sum(dtype=np.uint64))
    assert got["checksums"].shape == (3, 4)
    assert got["checksums"][0].tolist() == [s, int(valid.sum()), total >> 32, total & 0xFFFFFFFF]


def test_dump_outputs_samples_long_outputs_the_same_way_every_time(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    n = 3 * bench.DUMP_SAMPLE_ROWS + 5
    rng = np.random.default_rng(3)
    vals = rng.integers(-2**63, 2**63 - 1, size=n, dtype=np.int64)
    valid = rng.random(n) < 0.9
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": (vals, valid), "y": (np.arange(n, dtype=np.uint64), None)})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    rows = a["x_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_SAMPLE_ROWS and (np.diff(rows) >= 0).all() and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(a["x"], _hi_lo(np.where(valid[rows], vals[rows], 0)))
    assert np.array_equal(a["x_valid"], valid[rows].astype(np.float32))
    assert np.array_equal(a["y"], _hi_lo(rows))
    total = int(np.where(valid, vals, 0).view(np.uint64).sum(dtype=np.uint64))
    assert a["checksums"].tolist() == [[n, int(valid.sum()), total >> 32, total & 0xFFFFFFFF],
                                       [n, n, (n * (n - 1) // 2) >> 32, (n * (n - 1) // 2) & 0xFFFFFFFF]]
