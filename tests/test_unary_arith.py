"""One-operand arithmetic and rounding (arrow_amd.compute.negate .. round_to_multiple, arx_unary_numeric, arx_round_numeric,
csrc/unary_arith.hip) against pyarrow.compute on the host copies of the same arrays: the valid slots BIT FOR BIT (floats
are compared as integers — these are exact IEEE operations, there is no tolerance), validity, null_count, result type and
result offset 0, and no validity buffer when the input has none.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the MI355X
plus one column of 10^6 rows per type.

Rows the reference refuses ("overflow occurred during rounding", "Rounding V up to multiple of M would overflow") are taken
out by a per-value reference call, and the device's own refusal of them is checked.  Every float rounding case asserts that
at most 5 % of its rows were taken out — but for round(ndigits=400): there pow10 is +inf in both float types, and the
reference refuses EVERY finite row, +-0.0 included (pyarrow 25: pc.round([0.0], 400) raises); that case asserts exactly
this instead — the reference refuses all finite rows and no other, the device raises the same Status on the column, and the
rows that are left (NaN, +-inf) come back with their bits."""
import ctypes as C
import re

import numpy as np
import pytest

from . import util as U

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

OFFSET = 13
INT_TYPES = {"int8": (pa.int8(), np.int8, 0), "uint8": (pa.uint8(), np.uint8, 1), "int16": (pa.int16(), np.int16, 2),
             "uint16": (pa.uint16(), np.uint16, 3), "int32": (pa.int32(), np.int32, 4), "uint32": (pa.uint32(), np.uint32, 5),
             "int64": (pa.int64(), np.int64, 6), "uint64": (pa.uint64(), np.uint64, 7)}
FLOAT_TYPES = {"float": (pa.float32(), np.float32, 8), "double": (pa.float64(), np.float64, 9)}
TYPES = {**INT_TYPES, **FLOAT_TYPES}
SIGNED = ("int8", "int16", "int32", "int64")
MODES = ["down", "up", "towards_zero", "towards_infinity", "half_down", "half_up", "half_towards_zero", "half_towards_infinity",
         "half_to_even", "half_to_odd"]
HALF_MODES = MODES[4:]
UNARY = {"negate": 0, "negate_checked": 0, "abs": 1, "abs_checked": 1, "sign": 2, "floor": 3, "ceil": 4, "trunc": 5}
NDIGITS = [-400, -12, -2, -1, 0, 1, 2, 11, 15, 16, 17, 23, 400]
MULTIPLES = [0.5, 0.25, 1, 3, 0.1, 1e-3, 7.5, 1e30, 1e-30]
MAX_REFUSED = 0.05


def functions_of(name):
    """The reference's kernel lists (the table of DESIGN.md 4.25)."""
    fns = ["negate", "abs", "abs_checked", "sign"]
    if not name.startswith("u"):
        fns.append("negate_checked")
    if name in FLOAT_TYPES:
        fns += ["floor", "ceil", "trunc"]
    return fns


def rows_per_wave(name):
    """Rows one wave takes with one load (csrc/unary_arith.hip): 64 lanes x 16 bytes."""
    return 64 * 16 // TYPES[name][1]().itemsize


def lengths_of(name):
    w = rows_per_wave(name)
    return [0, 1, 63, 64, 65, w - 1, w + 1, 4097]


def rng_for(*key):
    return U.rng_for(0xA17, *key)


# ---------------------------------------------------------------- values
def int_specials(name):
    info = np.iinfo(TYPES[name][1])
    values = [info.min, info.min + 1, 0, 1, info.max - 1, info.max]
    return values + ([-1] if info.min < 0 else [])


def int_values(rng, name, n, keep_min=True):
    dt = TYPES[name][1]
    info = np.iinfo(dt)
    out = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    sp = np.array(int_specials(name), dtype=dt)
    k = min(n, len(sp))
    out[:k] = sp[:k]
    if n >= 2 * len(sp):
        out[-len(sp):] = sp          # (the specials in the last lanes as well)
    if not keep_min:
        out[out == info.min] = info.min + 1
    return out


def float_specials(name):
    dt = TYPES[name][1]
    fi = np.finfo(dt)
    ties = [s * (k + 0.5) / 10 ** j for j in range(4) for k in (0, 1, 2, 3, 12, 265) for s in (1, -1)]
    sp = [0.0, -0.0, np.nan, np.inf, -np.inf, float(fi.smallest_subnormal), 0.5, -0.5, 2.5, 2.675, 1.005, float(fi.max), -float(fi.max)]
    return np.array(sp + ties, dtype=dt)


def float_values(rng, name, n, with_max=True):
    """The specials first (and last), seeded random over 18 decades (1e-9 .. 1e9, both signs) in between."""
    dt = TYPES[name][1]
    out = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-9, 9, n)).astype(dt)
    sp = float_specials(name)
    if not with_max:
        sp = sp[np.abs(sp) != np.finfo(dt).max]
    k = min(n, len(sp))
    out[:k] = sp[:k]
    if n >= 2 * len(sp):
        out[-len(sp):] = sp
    return out


def values_of(rng, name, n, keep_min=True):
    return int_values(rng, name, n, keep_min) if name in INT_TYPES else float_values(rng, name, n)


def column(name, values, valid=None, offset=0):
    """The numpy `values` as a pyarrow column of the type, under the validity `valid` (the nulls' bytes stay as they are),
    seen from `offset` on."""
    t = TYPES[name][0]
    n = len(values)
    vbuf = None if valid is None else pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
    arr = pa.Array.from_buffers(t, n, [vbuf, pa.py_buffer(np.ascontiguousarray(values).tobytes())])
    return arr.slice(offset) if offset else arr


def make_column(rng, name, n, offset, null_p, keep_min=True):
    total = n + offset + (3 if offset else 0)
    values = values_of(rng, name, total, keep_min=True)
    valid = (rng.random(total) >= null_p) if null_p else None
    if not keep_min and name in SIGNED:      # the signed minimum stays only under nulls: a checked form must not see it
        lo = np.iinfo(TYPES[name][1]).min
        values[(values == lo) & (valid if valid is not None else True)] = lo + 1
    arr = column(name, values, valid)
    return arr.slice(offset, n) if offset else arr


# ---------------------------------------------------------------- comparison
def raw_bits(arr):
    """The value slots of a pyarrow primitive array as unsigned integers of their width."""
    w = arr.type.bit_width // 8
    buf = arr.buffers()[1]
    if buf is None or len(arr) == 0:
        return np.zeros(0, dtype=f"u{w}")
    return np.frombuffer(buf, dtype=f"u{w}", count=arr.offset + len(arr))[arr.offset:]


def validity_of(arr):
    return np.ones(len(arr), bool) if arr.null_count == 0 else np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), bool)


def assert_same(got, want, arr, what):
    """got: the device result (an arrow_amd.Array); want: the reference's result for the host column `arr`."""
    assert got.type.name == str(want.type), (what, got.type.name, str(want.type))
    assert got.offset == 0 and got.length == len(want), what
    host = got.to_pyarrow()
    ok = validity_of(want)
    assert (validity_of(host) == ok).all(), what
    assert got.null_count == want.null_count, (what, got.null_count, want.null_count)
    g, w = raw_bits(host)[ok], raw_bits(want)[ok]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, "first differing valid slot", int(bad[0]), hex(int(g[bad[0]])), hex(int(w[bad[0]])), bad.size)
    if arr.buffers()[0] is None:
        assert got.validity is None, what


def check(amd, fn, arr, what=(), **options):
    want = getattr(pc, fn)(arr, **options)
    got = getattr(amd.compute, fn)(amd.Array.from_pyarrow(arr), **options)
    assert_same(got, want, arr, (fn, what, options))
    return got


def reference_accepts(fn, arr, **options):
    """Per row: does the reference compute it (True) or refuse it; and the refusal texts by row."""
    ok = np.ones(len(arr), bool)
    texts = {}
    try:
        getattr(pc, fn)(arr, **options)
        return ok, texts
    except pa.ArrowInvalid:
        pass
    valid = validity_of(arr)
    for i in np.flatnonzero(valid):
        try:
            getattr(pc, fn)(arr.slice(int(i), 1), **options)
        except pa.ArrowInvalid as e:
            ok[i] = False
            texts[int(i)] = str(e)
    return ok, texts


def without_rows(name, arr, keep):
    """The column with only the rows of `keep` (values and validity re-packed)."""
    values = np.frombuffer(arr.buffers()[1], dtype=TYPES[name][1], count=arr.offset + len(arr))[arr.offset:][keep]
    valid = validity_of(arr)[keep]
    return column(name, values, None if arr.buffers()[0] is None else valid)


# ---------------------------------------------------------------- negate .. trunc
def _unary_grid(amd, name):
    for n in lengths_of(name):
        for offset in (0, OFFSET):
            for null_p in (0.0, 0.2):
                rng = rng_for("grid", name, n, offset, null_p)
                arr = make_column(rng, name, n, offset, null_p)
                safe = make_column(rng, name, n, offset, null_p, keep_min=False)
                for fn in functions_of(name):
                    checked_signed = fn.endswith("_checked") and name in SIGNED
                    check(amd, fn, safe if checked_signed else arr, (name, n, offset, null_p))


def _unary_known_answers(amd):
    run = lambda fn, values, t: getattr(amd.compute, fn)(amd.Array.from_pyarrow(pa.array(values, t))).to_pyarrow().to_pylist()  # noqa: E731
    assert run("negate", [1, 0, 255], pa.uint8()) == [255, 0, 1]                      # unsigned negate wraps
    assert run("negate", [-128, 127, None], pa.int8()) == [-128, -127, None]
    assert run("abs", [-128, -127, 5], pa.int8()) == [-128, 127, 5]
    assert run("abs", [200, 0], pa.uint8()) == [200, 0] and run("abs_checked", [200, 0], pa.uint8()) == [200, 0]
    assert run("sign", [-5, 0, 9, None], pa.int64()) == [-1, 0, 1, None]
    assert run("sign", [7, 0], pa.uint32()) == [1, 0]
    got = amd.compute.sign(amd.Array.from_pyarrow(pa.array([-0.0, 0.0, -3.5, np.inf], pa.float64()))).to_pyarrow()
    assert raw_bits(got).tolist() == raw_bits(pa.array([0.0, 0.0, -1.0, 1.0], pa.float64())).tolist()   # sign(-0.0) == +0.0
    assert run("floor", [-0.5, 2.5], pa.float32()) == [-1.0, 2.0] and run("ceil", [-1.5, 2.5], pa.float64()) == [-1.0, 3.0]
    assert run("trunc", [-1.5, 2.5], pa.float64()) == [-1.0, 2.0]
    r = lambda values, t, **o: amd.compute.round(amd.Array.from_pyarrow(pa.array(values, t)), **o).to_pyarrow()  # noqa: E731
    zero = r([-0.4, -0.5], pa.float64())                                                # the signs of zero
    assert raw_bits(zero).tolist() == [1 << 63, 1 << 63]
    assert raw_bits(r([-0.5], pa.float64(), round_mode="half_up")).tolist() == [1 << 63]
    assert r([2.5, 3.5, 2.675], pa.float64()).to_pylist() == [2.0, 4.0, 3.0]
    assert r([2.675, 1.005], pa.float64(), ndigits=2).to_pylist() == pc.round(pa.array([2.675, 1.005]), 2).to_pylist()
    assert r([15, 25, -15, 7], pa.int32(), ndigits=-1).to_pylist() == [20, 20, -20, 10]
    assert r([15, 25], pa.int32(), ndigits=3).to_pylist() == [15, 25]                   # ndigits >= 0: the input


def _checked_errors(amd):
    for name in SIGNED:
        t, dt, _ = INT_TYPES[name]
        lo = int(np.iinfo(dt).min)
        values = np.array([3, lo, -7, lo, 9, 0, 1, 2, 3, 4], dtype=dt)
        for fn in ("negate_checked", "abs_checked"):
            for arr in (column(name, values), column(name, values, offset=1), column(name, values[:2])):
                with pytest.raises(pa.ArrowInvalid, match="^overflow$"):
                    getattr(pc, fn)(arr)
                with pytest.raises(amd.ArrowInvalid, match="^overflow$"):
                    getattr(amd.compute, fn)(amd.Array.from_pyarrow(arr))
            # the minimum under a null does not fail
            valid = values != lo
            check(amd, fn, column(name, values, valid), (name, "minimum under nulls"))
            check(amd, fn, column(name, values, valid, offset=1), (name, "minimum under nulls, sliced"))
        check(amd, "negate", column(name, values), name)
        check(amd, "abs", column(name, values), name)


# ---------------------------------------------------------------- rounding of floats
def _round_float_case(amd, fn, name, arr, **options):
    what = (fn, name, options)
    ok, texts = reference_accepts(fn, arr, **options)
    valid = validity_of(arr)
    refused = int((~ok).sum())
    finite = np.isfinite(np.frombuffer(arr.buffers()[1], dtype=TYPES[name][1], count=arr.offset + len(arr))[arr.offset:])
    if fn == "round" and options.get("ndigits") == 400:
        assert ((~ok) == (finite & valid)).all(), what          # pow10 is +inf: the reference refuses every finite row
    else:
        assert refused <= MAX_REFUSED * len(arr), (what, refused, len(arr))
    if refused:
        assert set(texts.values()) == {"overflow occurred during rounding"}, (what, set(texts.values()))
        with pytest.raises(amd.ArrowInvalid, match="^overflow occurred during rounding$"):
            getattr(amd.compute, fn)(amd.Array.from_pyarrow(arr), **options)
        arr = without_rows(name, arr, ok)
    check(amd, fn, arr, what, **options)
    return refused


def _round_floats(amd, name, ndigits_list=NDIGITS):
    rng = rng_for("round", name)
    n = 400
    arr = make_column(rng, name, n, OFFSET, 0.2)
    plain = make_column(rng, name, 200, 0, 0.0)
    for ndigits in ndigits_list:
        for mode in MODES:
            _round_float_case(amd, "round", name, arr, ndigits=ndigits, round_mode=mode)
        _round_float_case(amd, "round", name, plain, ndigits=ndigits)


def _round_to_multiple_floats(amd, name):
    rng = rng_for("round_to_multiple", name)
    arr = make_column(rng, name, 400, OFFSET, 0.2)
    plain = make_column(rng, name, 200, 0, 0.0)
    for multiple in MULTIPLES:
        for mode in MODES:
            _round_float_case(amd, "round_to_multiple", name, arr, multiple=multiple, round_mode=mode)
        _round_float_case(amd, "round_to_multiple", name, plain, multiple=multiple)


def _round_shapes(amd, name):
    """round / round_to_multiple over the grid's lengths, offsets and null shares (one option set each)."""
    for n in lengths_of(name):
        for offset in (0, OFFSET):
            for null_p in (0.0, 0.2):
                rng = rng_for("round shapes", name, n, offset, null_p)
                if name in FLOAT_TYPES:
                    total = n + offset + (3 if offset else 0)
                    values = float_values(rng, name, total, with_max=False)
                    valid = (rng.random(total) >= null_p) if null_p else None
                    arr = column(name, values, valid)
                    arr = arr.slice(offset, n) if offset else arr
                    check(amd, "round", arr, (name, n, offset, null_p), ndigits=2)
                    check(amd, "round", arr, (name, n, offset, null_p), ndigits=-1, round_mode="half_up")
                    check(amd, "round_to_multiple", arr, (name, n, offset, null_p), multiple=0.25, round_mode="towards_infinity")
                else:
                    arr = make_column(rng, name, n, offset, null_p)
                    check(amd, "round", arr, (name, n, offset, null_p), ndigits=3)
                    check(amd, "round", arr, (name, n, offset, null_p), ndigits=-1, round_mode="towards_zero")
                    check(amd, "round_to_multiple", arr, (name, n, offset, null_p), multiple=7, round_mode="towards_zero" if name in SIGNED else "half_down")


# ---------------------------------------------------------------- rounding of integers
OVERFLOW_TEXT = re.compile(r"^Rounding (.*) (up|down) to (multiples?) of (.*) would overflow$", re.DOTALL)


def device_error(amd, fn, arr, **options):
    with pytest.raises(amd.ArrowInvalid) as err:
        getattr(amd.compute, fn)(amd.Array.from_pyarrow(arr), **options)
    return str(err.value)


def _round_int_case(amd, fn, name, values, m, **options):
    """All of `values`: the rows the reference computes equal it; each row it refuses is refused alone with its text — for
    the 8-bit types, whose value and multiple the reference prints as raw characters, with the same direction and the same
    "multiple" / "multiples", and the numbers in their place."""
    what = (fn, name, m, options)
    arr = column(name, values)
    ok, texts = reference_accepts(fn, arr, **options)
    if not ok.all():
        last = int(np.flatnonzero(~ok)[-1])
        parts = OVERFLOW_TEXT.match(texts[last])
        assert parts, (what, texts[last])
        want_last = f"Rounding {int(values[last])} {parts.group(2)} to {parts.group(3)} of {m} would overflow"
        assert device_error(amd, fn, arr, **options) == want_last, what                 # the whole column: the last failing row
        for i in np.flatnonzero(~ok):
            parts = OVERFLOW_TEXT.match(texts[int(i)])
            assert parts, (what, texts[int(i)])
            want = f"Rounding {int(values[i])} {parts.group(2)} to {parts.group(3)} of {m} would overflow"
            if TYPES[name][1]().itemsize > 1:
                assert texts[int(i)] == want, (what, texts[int(i)], want)
            assert device_error(amd, fn, column(name, values[i:i + 1]), **options) == want, (what, int(values[i]))
    if ok.any():
        check(amd, fn, column(name, values[ok]), what, **options)
    return int((~ok).sum())


def _round_int8_exhaustive(amd, name):
    dt = TYPES[name][1]
    info = np.iinfo(dt)
    values = np.arange(info.min, info.max + 1, dtype=np.int64).astype(dt)
    multiples = [1, 2, 3, 5, 7, 10, 63] + ([100, 127] if name == "uint8" else [])
    refused = 0
    for m in multiples:
        for mode in MODES:
            refused += _round_int_case(amd, "round_to_multiple", name, values, m, multiple=m, round_mode=mode)
    for ndigits in (-1,) + ((-2,) if name == "uint8" else ()):       # 100 is above half of int8's maximum
        for mode in MODES:
            refused += _round_int_case(amd, "round", name, values, 10 ** -ndigits, ndigits=ndigits, round_mode=mode)
    assert refused > 0


def _round_int_ends(amd, name):
    dt = TYPES[name][1]
    info = np.iinfo(dt)
    lo, hi = int(info.min), int(info.max)
    ends = sorted({lo, lo + 1, lo + 2, lo + 5, lo + 999, 0, 1, 5, 15, 25, hi // 2, hi // 2 + 1, hi - 999, hi - 5, hi - 2, hi - 1, hi}
                  | ({-1, -5, -15, -25, lo // 2, lo // 2 - 1} if lo < 0 else set()))
    values = np.array(ends, dtype=dt)
    for m in (1, 2, 10, 1000, hi // 2, hi // 2 - 1):
        for mode in MODES:
            _round_int_case(amd, "round_to_multiple", name, values, m, multiple=m, round_mode=mode)
    for ndigits in (-1, -3):
        for mode in MODES:
            _round_int_case(amd, "round", name, values, 10 ** -ndigits, ndigits=ndigits, round_mode=mode)
    # a multiple above half the maximum: the four modes that do not compare 2 |rem| with it (the reference's options take
    # no Python int above int64's maximum, which leaves uint64 out)
    for mode in MODES[:4] if hi // 2 + 2 < 2**63 else ():
        _round_int_case(amd, "round_to_multiple", name, values, hi // 2 + 2, multiple=hi // 2 + 2, round_mode=mode)


def _round_errors(amd):
    dev = amd.Array.from_pyarrow
    # ---- two failing rows, in both orders: the later one is named
    for name in ("int16", "int64", "uint64", "int8"):
        dt = TYPES[name][1]
        info = np.iinfo(dt)
        a, b = int(info.max), int(info.max) - 1
        for values in ([a, 5, b, 7], [b, 5, a, 7]):
            arr = column(name, np.array(values, dtype=dt))
            with pytest.raises(pa.ArrowInvalid) as ref:
                pc.round(arr, ndigits=-1, round_mode="up")
            text = device_error(amd, "round", arr, ndigits=-1, round_mode="up")
            assert text == f"Rounding {values[2]} up to multiple of 10 would overflow", (name, text)
            if name != "int8":
                assert text == str(ref.value), (name, text, str(ref.value))
            # ... unless it sits under a null
            valid = np.array([True, True, False, True])
            assert device_error(amd, "round", column(name, np.array(values, dtype=dt), valid), ndigits=-1, round_mode="up") == \
                f"Rounding {values[0]} up to multiple of 10 would overflow"
            # every failing value under a null: no failure
            check(amd, "round", column(name, np.array(values, dtype=dt), np.array([False, True, False, True])), name, ndigits=-1, round_mode="up")
    lo = -32768
    arr = column("int16", np.array([32767, 0, lo], dtype=np.int16))
    with pytest.raises(pa.ArrowInvalid) as ref:
        pc.round(arr, ndigits=-1, round_mode="half_up")
    assert device_error(amd, "round", arr, ndigits=-1, round_mode="half_up") == str(ref.value) == \
        "Rounding -32768 down to multiples of 10 would overflow"
    # ---- floats
    for name, big in (("double", 1e308), ("float", 3e38)):
        arr = column(name, np.array([big], dtype=TYPES[name][1]))
        with pytest.raises(pa.ArrowInvalid, match="^overflow occurred during rounding$"):
            pc.round(arr, 2)
        assert device_error(amd, "round", arr, ndigits=2) == "overflow occurred during rounding"
        under = column(name, np.array([1.25, big, 2.5], dtype=TYPES[name][1]), np.array([True, False, True]))
        check(amd, "round", under, (name, "overflow under a null"), ndigits=2)
    # ---- the arguments
    for name in ("int8", "uint8", "int16", "int64", "uint64"):
        arr = column(name, np.array([1, 2, 3], dtype=TYPES[name][1]))
        nd = -(len(str(int(np.iinfo(TYPES[name][1]).max))))
        for mode in ("down", "half_to_even"):
            with pytest.raises(pa.ArrowInvalid) as ref:
                pc.round(arr, ndigits=nd, round_mode=mode)
            assert device_error(amd, "round", arr, ndigits=nd, round_mode=mode) == str(ref.value) == \
                f"Rounding to {nd} digits is out of range for type {name}"
    for name in ("int8", "uint32", "int64", "float", "double"):
        arr = column(name, np.array([1, 2, 3], dtype=TYPES[name][1]))
        for multiple in (0, -2):
            with pytest.raises(pa.ArrowInvalid, match="^Rounding multiple must be positive$"):
                pc.round_to_multiple(arr, multiple=multiple)
            assert device_error(amd, "round_to_multiple", arr, multiple=multiple) == "Rounding multiple must be positive"
        with pytest.raises(pa.ArrowInvalid, match="^Rounding multiple must be non-null and valid$"):
            pc.round_to_multiple(arr, multiple=pa.scalar(None, arr.type))
        assert device_error(amd, "round_to_multiple", arr, multiple=None) == "Rounding multiple must be non-null and valid"
        assert device_error(amd, "round_to_multiple", arr, multiple=amd.Scalar(None, dev(arr).type, False)) == \
            "Rounding multiple must be non-null and valid"
    nan = column("double", np.array([1.5]))
    with pytest.raises(pa.ArrowInvalid, match="^Rounding multiple must be positive$"):
        pc.round_to_multiple(nan, multiple=float("nan"))
    assert device_error(amd, "round_to_multiple", nan, multiple=float("nan")) == "Rounding multiple must be positive"
    # the reference's cast of the multiple to the column's type
    a8 = column("int8", np.array([1, 5], dtype=np.int8))
    for multiple in (2.5, 300, -129, 300.0):
        with pytest.raises(pa.ArrowInvalid) as ref:
            pc.round_to_multiple(a8, multiple=multiple)
        assert device_error(amd, "round_to_multiple", a8, multiple=multiple) == str(ref.value), multiple
    check(amd, "round_to_multiple", a8, "a whole float multiple", multiple=2.0)
    check(amd, "round_to_multiple", column("float", np.array([1.5, 0.26], dtype=np.float32)), "a double multiple of a float column", multiple=0.1)
    # ---- a multiple above half the type's maximum in a half mode: refused, by name
    for name, m, fn, options in (("int8", 64, "round_to_multiple", {"multiple": 64}), ("uint8", 128, "round_to_multiple", {"multiple": 128}),
                                 ("int8", 100, "round", {"ndigits": -2}), ("int64", 2**62, "round_to_multiple", {"multiple": 2**62}),
                                 ("uint64", 10**19, "round", {"ndigits": -19}), ("int16", 10**4 * 2, "round_to_multiple", {"multiple": 20000})):
        arr = column(name, np.array([1, 2, 3], dtype=TYPES[name][1]))
        for mode in HALF_MODES:
            with pytest.raises(amd.ArrowNotImplementedError) as err:
                getattr(amd.compute, fn)(dev(arr), round_mode=mode, **options)
            assert fn in str(err.value) and name in str(err.value) and str(m) in str(err.value) and "arrow_amd" in str(err.value), str(err.value)
        if (name, fn) == ("uint64", "round"):       # (the reference's own round(uint64, -19) ends the process: no host call)
            assert getattr(amd.compute, fn)(dev(arr), round_mode="down", **options).to_pyarrow().to_pylist() == [0, 0, 0]
        else:
            check(amd, fn, arr, (name, m, "not a half mode"), round_mode="down", **options)


# ---------------------------------------------------------------- the mirror
def _mirror_and_refusals(amd):
    rng = rng_for("mirror")
    names = amd.compute.get_function_registry().get_function_names()
    arr = column("double", float_values(rng, "double", 300, with_max=False), rng.random(300) >= 0.2)     # (no row the reference refuses)
    d = amd.Array.from_pyarrow(arr)
    for fn in list(UNARY) + ["round", "round_to_multiple"]:
        assert fn in names, fn
        assert_same(amd.compute.call_function(fn, [d]), getattr(pc, fn)(arr), arr, fn)       # (the defaults of the two options)
    assert_same(amd.compute.call_function("round", [d], amd.compute.RoundOptions(2, "half_up")), pc.round(arr, 2, "half_up"), arr, "options")
    assert_same(amd.compute.call_function("round_to_multiple", [d], amd.compute.RoundToMultipleOptions(0.5, "up")),
                pc.round_to_multiple(arr, 0.5, "up"), arr, "options")
    assert_same(amd.compute.round_to_multiple(d, amd.Scalar(3, d.type)), pc.round_to_multiple(arr, 3.0), arr, "a Scalar multiple")
    with pytest.raises(ValueError, match='"bogus" is not a valid round mode'):
        pc.round(arr, round_mode="bogus")
    with pytest.raises(ValueError, match='"bogus" is not a valid round mode'):
        amd.compute.round(d, round_mode="bogus")
    # a known null count comes through without a read-back; a slice's is counted on first use
    known = amd.compute.negate(d)
    if not callable(d._null_count) and d._null_count >= 0:
        assert not callable(known._null_count)
    assert known.null_count == arr.null_count
    sl = amd.compute.abs(d.slice(3))
    assert sl.null_count == arr.slice(3).null_count and sl.offset == 0
    plain = amd.compute.sign(amd.Array.from_pyarrow(make_column(rng, "int32", 100, 0, 0.0)))
    assert plain.validity is None and plain.null_count == 0 and plain.type.name == "int8"
    # ---- the reference's kernel lists
    for fn, name in (("negate_checked", "uint8"), ("negate_checked", "uint64"), ("floor", "int32"), ("ceil", "uint8"), ("trunc", "int64")):
        host = make_column(rng, name, 10, 0, 0.0)
        with pytest.raises(amd.ArrowNotImplementedError, match="has no kernel matching input types") as err:
            getattr(amd.compute, fn)(amd.Array.from_pyarrow(host))
        assert str(err.value) == f"Function '{fn}' has no kernel matching input types ({host.type})"
    with pytest.raises(pa.ArrowNotImplementedError, match="has no kernel matching input types"):
        pc.negate_checked(make_column(rng, "uint8", 10, 0, 0.0))
    flags = amd.Array.from_pyarrow(pa.array([True, False]))
    for fn in ("negate", "abs", "sign", "round", "round_to_multiple"):
        with pytest.raises(amd.ArrowNotImplementedError, match="has no kernel matching input types"):
            getattr(amd.compute, fn)(flags)


# ---------------------------------------------------------------- the C ABI directly
def c_span(arr):
    """(ArxSpan, kept device buffers) of a host pyarrow array: its buffers uploaded as they are, offset and all."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    vb, db = arr.buffers()[:2]
    w = arr.type.bit_width // 8
    end = arr.offset + len(arr)
    keep = [to_device(np.frombuffer(vb, dtype=np.uint8)[: (end + 7) // 8]) if vb is not None else None,
            to_device(np.frombuffer(db, dtype=np.uint8)[: end * w])]
    return _lib.ArxSpan(keep[0].data_ptr() if keep[0] is not None else None, keep[1].data_ptr(), arr.offset, len(arr),
                        arr.null_count if vb is not None else 0), keep


def _c_abi(amd):
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    sync = lambda t: torch.cuda.synchronize() if t.is_cuda else None  # noqa: E731
    pad = 64
    count = lambda: (lib.arx_get_counter(b"unary_arith_launches"), lib.arx_get_counter(b"round_launches"))  # noqa: E731
    # ---- written bytes: exactly length results, nothing after them
    for name in ("int8", "uint16", "int32", "int64", "float", "double"):
        for n in (1, 15, 16, 17, rows_per_wave(name) + 1, 1001):
            rng = rng_for("c abi", name, n)
            arr = make_column(rng, name, n, OFFSET, 0.2)
            span, keep = c_span(arr)
            w = arr.type.bit_width // 8
            for fn, out_w in (("negate", w), ("sign", 1 if name in INT_TYPES else w)):
                out = to_device(np.full(n * out_w + pad, 0xEE, np.uint8))
                before = count()
                assert lib.arx_unary_numeric(UNARY[fn], 0, TYPES[name][2], C.byref(span), out.data_ptr(), None, None) == 0, lib.arx_last_error()
                sync(out)
                assert count() == (before[0] + 1, before[1])
                data = out.cpu().numpy()[: n * out_w + pad]
                assert (data[n * out_w:] == 0xEE).all(), (fn, name, n)
                want = getattr(pc, fn)(arr)
                ok = validity_of(want)
                assert (data[: n * out_w].view(f"u{out_w}")[ok] == raw_bits(want)[ok]).all(), (fn, name, n)
            out = to_device(np.full(n * w + pad, 0xEE, np.uint8))
            errors = to_device(np.zeros(8, np.uint8))
            multiple = np.array([3], dtype=TYPES[name][1])
            before = count()
            call = (1, MODES.index("down"), TYPES[name][2], C.byref(span), 0, multiple.ctypes.data)
            assert lib.arx_round_numeric(*call, out.data_ptr(), errors.data_ptr(), None) == 0, lib.arx_last_error()
            assert count() == (before[0], before[1] + 1)
            ok, _ = reference_accepts("round_to_multiple", arr, multiple=3, round_mode="down")
            rc = lib.arx_round_status(*call, errors.data_ptr(), None)
            assert (rc == 0) == bool(ok.all()), (name, n, lib.arx_last_error())
            data = out.cpu().numpy()[: n * w + pad]
            assert (data[n * w:] == 0xEE).all(), (name, n)
            if rc == 0:
                want = pc.round_to_multiple(arr, multiple=3, round_mode="down")
                okv = validity_of(want)
                assert (data[: n * w].view(f"u{w}")[okv] == raw_bits(want)[okv]).all(), (name, n)
            else:
                assert lib.arx_last_error().startswith(b"Rounding ") and lib.arx_last_error().endswith(b"would overflow")
    # ---- bad arguments: ARX_INVALID, nothing launched, nothing written
    arr = make_column(rng_for("invalid"), "int32", 100, 0, 0.2)
    span, keep = c_span(arr)
    farr = make_column(rng_for("invalid f"), "double", 100, 0, 0.0)
    fspan, fkeep = c_span(farr)
    out = to_device(np.full(100 * 8 + pad, 0xEE, np.uint8))
    errors = to_device(np.zeros(8, np.uint8))
    three = np.array([3], dtype=np.int32)
    before = count()
    I32, F64 = 4, 9
    unary = lambda op, checked, t, s=span, o=out, e=errors: lib.arx_unary_numeric(  # noqa: E731
        op, checked, t, C.byref(s) if s is not None else None, o.data_ptr() if o is not None else None, e.data_ptr() if e is not None else None, None)
    for args, text in (((6, 0, I32), b"no kernel for op"), ((-1, 0, I32), b"no kernel for op"), ((0, 0, 10), b"no kernel for op"),
                       ((0, 0, -1), b"no kernel for op"), ((2, 1, I32), b"no kernel for op"), ((3, 1, F64), b"no kernel for op"),
                       ((3, 0, I32), b"no kernel for op"), ((5, 0, 7), b"no kernel for op"), ((0, 1, 5), b"no kernel for op"),
                       ((0, 0, I32, None), b"NULL values"), ((0, 0, I32, span, None), b"NULL out"), ((0, 1, I32, span, out, None), b"NULL errors")):
        assert unary(*args) == _lib.ARX_INVALID, args
        assert text in lib.arx_last_error(), (args, lib.arx_last_error())
    rnd = lambda kind, mode, t, s=span, nd=0, m=three, o=out, e=errors: lib.arx_round_numeric(  # noqa: E731
        kind, mode, t, C.byref(s) if s is not None else None, nd, m.ctypes.data if m is not None else None,
        o.data_ptr() if o is not None else None, e.data_ptr() if e is not None else None, None)
    for args, text in (((2, 0, I32), b"no kernel for kind"), ((-1, 0, I32), b"no kernel for kind"), ((0, 10, I32), b"no kernel for kind"),
                       ((0, -1, I32), b"no kernel for kind"), ((1, 0, 10), b"no kernel for kind"), ((1, 0, I32, span, 0, None), b"NULL multiple"),
                       ((1, 0, I32, None), b"NULL values"), ((1, 0, I32, span, 0, three, None), b"NULL out"),
                       ((1, 0, I32, span, 0, three, out, None), b"NULL errors"),
                       ((1, 0, I32, span, 0, np.array([0], np.int32)), b"Rounding multiple must be positive"),
                       ((0, 0, I32, span, -10), b"Rounding to -10 digits is out of range for type int32")):
        assert rnd(*args) == _lib.ARX_INVALID, args
        assert text in lib.arx_last_error(), (args, lib.arx_last_error())
    assert rnd(1, MODES.index("half_up"), I32, span, 0, np.array([2**30], np.int32)) == _lib.ARX_NOT_IMPLEMENTED
    assert rnd(1, MODES.index("up"), F64, fspan, 0, np.array([-1.0])) == _lib.ARX_INVALID and b"must be positive" in lib.arx_last_error()
    sync(out)
    untouched = lambda: (out.cpu().numpy()[: 100 * 8 + pad] == 0xEE).all()  # noqa: E731
    assert untouched() and count() == before
    # length 0 succeeds, launches nothing and writes nothing
    empty = _lib.ArxSpan(None, keep[1].data_ptr(), 0, 0, 0)
    assert unary(0, 1, I32, empty) == 0 and unary(0, 1, I32, empty, None, None) == 0
    assert rnd(0, 0, I32, empty, -1) == 0 and lib.arx_round_status(0, 0, I32, C.byref(empty), -1, None, errors.data_ptr(), None) == 0
    assert untouched() and count() == before


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("name", list(TYPES))
def test_unary_grid(emu_ctx, name):
    _unary_grid(emu_ctx, name)


@pytest.mark.emu
def test_unary_known_answers_and_checked_errors(emu_ctx):
    _unary_known_answers(emu_ctx)
    _checked_errors(emu_ctx)


@pytest.mark.emu
@pytest.mark.parametrize("name", list(FLOAT_TYPES))
def test_round_floats_every_ndigits_and_mode(emu_ctx, name):
    _round_floats(emu_ctx, name)


@pytest.mark.emu
@pytest.mark.parametrize("name", list(FLOAT_TYPES))
def test_round_to_multiple_floats_every_multiple_and_mode(emu_ctx, name):
    _round_to_multiple_floats(emu_ctx, name)


@pytest.mark.emu
@pytest.mark.parametrize("name", list(TYPES))
def test_round_shapes(emu_ctx, name):
    _round_shapes(emu_ctx, name)


@pytest.mark.emu
@pytest.mark.parametrize("name", ["int8", "uint8"])
def test_round_8_bit_exhaustive(emu_ctx, name):
    _round_int8_exhaustive(emu_ctx, name)


@pytest.mark.emu
@pytest.mark.parametrize("name", ["int16", "uint16", "int32", "uint32", "int64", "uint64"])
def test_round_integer_ends(emu_ctx, name):
    _round_int_ends(emu_ctx, name)


@pytest.mark.emu
def test_round_errors(emu_ctx):
    _round_errors(emu_ctx)


@pytest.mark.emu
def test_unary_mirror_and_refusals(emu_ctx):
    _mirror_and_refusals(emu_ctx)


@pytest.mark.emu
def test_unary_c_abi_written_bytes_invalid_arguments_and_counters(emu_ctx):
    _c_abi(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TYPES))
def test_gpu_unary_grid_and_round_shapes(gpu_ctx, name):
    _unary_grid(gpu_ctx, name)
    _round_shapes(gpu_ctx, name)


@pytest.mark.gpu
def test_gpu_unary_known_answers_errors_and_mirror(gpu_ctx):
    _unary_known_answers(gpu_ctx)
    _checked_errors(gpu_ctx)
    _round_errors(gpu_ctx)
    _mirror_and_refusals(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FLOAT_TYPES))
def test_gpu_round_floats(gpu_ctx, name):
    _round_floats(gpu_ctx, name)
    _round_to_multiple_floats(gpu_ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INT_TYPES))
def test_gpu_round_integers(gpu_ctx, name):
    if name in ("int8", "uint8"):
        _round_int8_exhaustive(gpu_ctx, name)
    else:
        _round_int_ends(gpu_ctx, name)


@pytest.mark.gpu
def test_gpu_unary_c_abi(gpu_ctx):
    _c_abi(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TYPES))
def test_gpu_unary_1e6_rows(gpu_ctx, name):
    rng = rng_for("1e6", name)
    n = 1_000_000
    total = n + OFFSET
    valid = rng.random(total) >= 0.05
    if name in FLOAT_TYPES:
        values = float_values(rng, name, total, with_max=False)
    else:
        values = int_values(rng, name, total)
        if name in SIGNED:
            values[(values == np.iinfo(values.dtype).min) & valid] += 1
    arr = column(name, values, valid, offset=OFFSET)
    for fn in functions_of(name):
        check(gpu_ctx, fn, arr, ("1e6", name))
    if name in FLOAT_TYPES:
        check(gpu_ctx, "round", arr, ("1e6", name), ndigits=2)
        check(gpu_ctx, "round", arr, ("1e6", name), ndigits=-2, round_mode="half_towards_zero")
        check(gpu_ctx, "round_to_multiple", arr, ("1e6", name), multiple=0.5, round_mode="half_to_odd")
    else:
        check(gpu_ctx, "round", arr, ("1e6", name), ndigits=-1, round_mode="towards_zero")
        check(gpu_ctx, "round_to_multiple", arr, ("1e6", name), multiple=7, round_mode="towards_zero" if name in SIGNED else "half_down")
