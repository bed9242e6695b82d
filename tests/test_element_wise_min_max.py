"""min_element_wise / max_element_wise (arrow_amd.compute, arx_min_max_element_wise, csrc/element_wise.hip) against
pyarrow.compute on the host copies of the same arrays: values by `equals`, float columns also by bit pattern (equals tells
neither +0 from -0 nor one NaN from another), null_count and result offset 0 — exact equality, no tolerances.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus columns of 10^6 rows built from numpy buffers.  Scalars are typed pyarrow scalars and every operand of a call
has one type, so the reference promotes nothing."""
import ctypes as C
import struct

import numpy as np
import pytest

from . import test_case_when as CW
from . import test_if_else as IE
from . import util as U

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

# rows one wave takes at a time (csrc/element_wise.hip): 64 x (16 / W) x element_wise_steps = 512 at W = 8, 1024 at W = 4, 2, 1
ROWS_PER_WAVE = (512, 1024)
LENGTHS = sorted({0, 1, 63, 64, 65, 4097, 100_000} | {r + d for r in ROWS_PER_WAVE for d in (-1, 1)})
NUMERIC = {"int8": pa.int8(), "uint8": pa.uint8(), "int16": pa.int16(), "uint16": pa.uint16(), "int32": pa.int32(),
           "uint32": pa.uint32(), "int64": pa.int64(), "uint64": pa.uint64(), "float32": pa.float32(), "float64": pa.float64()}
TYPES = dict(NUMERIC, **{"timestamp[us]": pa.timestamp("us")})
OFFSETS = (13, 5, 70, 3, 64)               # every operand at its own alignment (the result's offset is 0)
OPS = {"min": ("min_element_wise", 0), "max": ("max_element_wise", 1)}     # name -> (function, ARX_ELEMENT_WISE_*)
NUM_TYPE = {name: j for j, name in enumerate(NUMERIC)}                     # ARX_NUM_*


def rng_for(*key):
    return U.rng_for(0xE1E, *key)


def column(rng, t, n, null_p):
    """IE.column, with a narrow value range for the wide integers so that ties between operands occur."""
    if pa.types.is_integer(t) and t.bit_width >= 32:
        mask = (rng.random(n) < null_p) if null_p else None
        lo = 0 if pa.types.is_unsigned_integer(t) else -40
        return pa.array(rng.integers(lo, 40, n), t, mask=mask)
    return IE.column(rng, t, n, null_p)


def cut(rng, t, n, null_p, offset):
    return column(rng, t, n + offset + 3, null_p).slice(offset, n)


def can_be_null(x):
    return (x.null_count != 0 and x.buffers()[0] is not None) if isinstance(x, pa.Array) else not x.is_valid


def result_can_be_null(operands, skip_nulls):
    return all(can_be_null(x) for x in operands) if skip_nulls else any(can_be_null(x) for x in operands)


def check(amd, op, operands, skip_nulls, what=()):
    name = OPS[op][0]
    want = getattr(pc, name)(*operands, skip_nulls=skip_nulls)
    got = getattr(amd.compute, name)(*[IE.amd_operand(amd, x) for x in operands], skip_nulls=skip_nulls)
    assert got.offset == 0 and got.length == len(want), what
    CW.assert_same(got.to_pyarrow(), want, what)
    assert got.null_count == want.null_count, (what, got.null_count, want.null_count)
    if not result_can_be_null(operands, skip_nulls):
        assert got.validity is None, what
    return got


def _grid(amd, n):
    for name, t in TYPES.items():
        for k in (1, 2, 3, 5):
            for nulls in range(3):          # no operand with nulls, every second one, all of them
                rng = rng_for("grid", n, name, k, nulls)
                operands = [cut(rng, t, n, 0.1 if (nulls == 2 or (nulls == 1 and j % 2 == 0)) else 0.0, OFFSETS[j]) for j in range(k)]
                for op in OPS:
                    for skip_nulls in (True, False):
                        check(amd, op, operands, skip_nulls, ("grid", n, name, k, nulls, op, skip_nulls))


def _operand_forms(amd):
    n = 1000
    for name in ("int16", "uint64", "float32", "timestamp[us]"):
        t = TYPES[name]
        rng = rng_for("forms", name)
        arrays = [cut(rng, t, n, 0.1, OFFSETS[j]) for j in range(2)]
        plain = cut(rng, t, n, 0.0, OFFSETS[2])
        five, nine, null = pa.scalar(5, t), pa.scalar(9, t), pa.scalar(None, t)
        for operands in ([arrays[0], five], [five, arrays[0]], [arrays[0], null], [null, arrays[0]], [five, arrays[0], nine, arrays[1]],
                         [null, arrays[0], five], [arrays[0], null, null], [plain, five], [plain, null], [null, plain, nine], [plain]):
            for op in OPS:
                for skip_nulls in (True, False):
                    got = check(amd, op, operands, skip_nulls, ("forms", name, op, skip_nulls, [str(x)[:12] for x in operands]))
                    if not skip_nulls and any(x is null for x in operands):
                        assert not callable(got._null_count) and got.null_count == n      # known without a read-back


# ---- the reference's fold, pinned by bit pattern
P0, N0 = 0.0, -0.0
NAN_A = {"float32": 0x7FC00000, "float64": 0x7FF8000000000000}             # the default quiet NaN
NAN_B = {"float32": 0xFFC00123, "float64": 0xFFF8000000000123}             # another one: sign and payload set


def bits_column(name, patterns):
    """A float column from bit patterns (None = null); pyarrow's own conversions might quieten or replace a NaN."""
    dt, t = (np.uint32, pa.float32()) if name == "float32" else (np.uint64, pa.float64())
    valid = np.array([p is not None for p in patterns])
    data = np.array([0 if p is None else p for p in patterns], dtype=dt)
    return pa.Array.from_buffers(t, len(patterns), [pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if not valid.all() else None,
                                                    pa.py_buffer(data.tobytes())])


def _pins(amd):
    for name in ("float32", "float64"):
        t = TYPES[name]
        pack = (lambda x: struct.unpack("<I", struct.pack("<f", x))[0]) if name == "float32" else (lambda x: struct.unpack("<Q", struct.pack("<d", x))[0])
        p0, n0, two, inf, ninf = pack(P0), pack(N0), pack(2.0), pack(float("inf")), pack(float("-inf"))
        a, b = NAN_A[name], NAN_B[name]
        if name == "float32":
            # Which of two float32 NaNs the reference returns depends on which of its internal loops a row falls in (observed:
            # the same operands with and without a validity bitmap give different payloads), so for float32 only the default
            # NaN is pinned; the device keeps the accumulator's.
            b = a
        col = lambda *patterns: bits_column(name, list(patterns))  # noqa: E731

        def pin(op, operands, want_patterns, skip_nulls=True):
            """The device result, the reference's result and the literal patterns agree (None = a null row)."""
            fn = OPS[op][0]
            want = col(*want_patterns)
            ref = getattr(pc, fn)(*operands, skip_nulls=skip_nulls)
            CW.assert_same(ref, want, ("the reference against the literal", name, op, want_patterns))
            got = getattr(amd.compute, fn)(*[IE.amd_operand(amd, x) for x in operands], skip_nulls=skip_nulls).to_pyarrow()
            CW.assert_same(got, want, ("the device against the literal", name, op, want_patterns))
            CW.assert_same(got, ref, ("the device against the reference", name, op, want_patterns))

        # The reference's step is std::fmin / std::fmax as its build resolves them, and the two widths differ (pyarrow 25.0.0,
        # x86-64): for float64 a tie keeps the accumulator and of two NaNs the right one's bits come out; for float32 a tie
        # takes the right operand and of two NaNs the accumulator stays — and the fold starts from the default NaN (`a`), so a
        # float32 NaN that comes from arrays alone is always `a`.  Each pin below holds against pyarrow and against the
        # literal patterns; the float64 patterns are the ones the feature was specified with.
        f64 = name == "float64"
        # a tie of +0 and -0, for min and for max
        for op in OPS:
            pin(op, [col(p0, n0), col(n0, p0)], [p0, n0] if f64 else [n0, p0])
        # a scalar -0.0 anywhere in the argument list: the scalars are folded first, so it is the accumulator of every row
        minus_zero = pa.scalar(N0, t)
        for op in OPS:
            pin(op, [minus_zero, col(p0, n0)], [n0, n0] if f64 else [p0, n0])
            pin(op, [col(p0, n0), minus_zero], [n0, n0] if f64 else [p0, n0])
            pin(op, [col(p0, n0), minus_zero, col(p0, p0)], [n0, n0] if f64 else [p0, p0])
        # NaN against NaN
        for op in OPS:
            pin(op, [col(a, b), col(b, a)], [b, a] if f64 else [a, a])
            pin(op, [col(b, b)], [b, b] if f64 else [a, a])                    # one operand: a copy (float32: but for its NaNs)
        # a NaN loses to any number, the infinities included
        pin("min", [col(a, a, inf, ninf, b), col(inf, ninf, b, a, two)], [inf, ninf, inf, ninf, two])
        pin("max", [col(a, a, inf, ninf, b), col(inf, ninf, b, a, two)], [inf, ninf, inf, ninf, two])
        # a null against a NaN is a NaN under skip_nulls, null without
        for op in OPS:
            pin(op, [col(None), col(b)], [b if f64 else a])
            pin(op, [col(None), col(b)], [None], skip_nulls=False)
        # three operands with nulls, zeros of both signs and NaNs
        for op in OPS:
            pin(op, [col(None, n0, a), col(p0, None, a), col(n0, p0, two)], [p0, n0, two] if f64 else [n0, p0, two])
        # scalars: a NaN scalar loses to the rows, a null scalar is skipped or makes every row null
        nan_scalar = col(b)[0]
        for op in OPS:
            pin(op, [nan_scalar, col(two, a, None)], [two, a if f64 else b, b])
            pin(op, [col(two, a, None), pa.scalar(None, t)], [two, a, None])
            pin(op, [col(two, a, None), pa.scalar(None, t)], [None, None, None], skip_nulls=False)


def _integer_extremes(amd):
    for name, t in NUMERIC.items():
        if name.startswith("float"):
            continue
        info = np.iinfo(np.dtype(t.to_pandas_dtype()))
        lo, hi, mid = int(info.min), int(info.max), int(info.max) // 2 + 1     # (mid: 2^63 for uint64, above the signed range)
        left = pa.array([lo, hi, lo, hi, mid, mid - 1, None, 0], t)
        right = pa.array([hi, lo, lo, hi, mid - 1, mid, hi, None], t)
        want_min = [lo, lo, lo, hi, mid - 1, mid - 1, hi, 0]
        want_max = [hi, hi, lo, hi, mid, mid, hi, 0]
        assert check(amd, "min", [left, right], True, ("extremes", name)).to_pylist() == want_min
        assert check(amd, "max", [left, right], True, ("extremes", name)).to_pylist() == want_max
        assert check(amd, "min", [left, right], False, ("extremes", name)).to_pylist() == want_min[:6] + [None, None]
        assert check(amd, "max", [left, pa.scalar(mid, t)], True, ("extremes, scalar", name)).to_pylist() == [mid, hi, mid, hi, mid, mid, mid, mid]
        assert check(amd, "min", [pa.scalar(mid, t), right], True, ("extremes, scalar", name)).to_pylist() == [mid, lo, lo, mid, mid - 1, mid, mid, mid]


def _caps(amd):
    n = 200
    rng = rng_for("caps")
    operands = [column(rng, pa.int32(), n, 0.3) for _ in range(33)]
    for op in OPS:
        check(amd, op, operands[:32], True, "32 operands")
        check(amd, op, operands[:32], False, "32 operands")
        check(amd, op, operands[:31] + [pa.scalar(-7, pa.int32())], True, "31 arrays and a scalar")
    doperands = [amd.Array.from_pyarrow(x) for x in operands]
    with pytest.raises(amd.ArrowNotImplementedError, match="33 operands on device-resident arrays: the device kernel takes up to 32"):
        amd.compute.max_element_wise(*doperands)


# ---------------------------------------------------------------- the C ABI directly
def c_min_max(amd, t, op, skip_nulls, operands, with_validity=True, pad=64):
    """arx_min_max_element_wise on host pyarrow operands: (rc, raw data bytes, raw validity bytes | None); both output
    buffers are filled with 0xEE first and carry `pad` bytes after what the call may write."""
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n = next(len(x) for x in operands if isinstance(x, pa.Array))
    w = t.byte_width
    words = (n + 63) // 64
    keep = []
    table = (_lib.ArxOperand * len(operands))()
    for j, x in enumerate(operands):
        if isinstance(x, pa.Array):
            span, bufs = IE.c_operand(x)
            keep.extend([span, bufs])
            table[j].span = C.pointer(span)
        elif x.is_valid:
            raw = IE.c_scalar_bytes(x)
            keep.append(C.create_string_buffer(raw, len(raw)))
            table[j].scalar = C.cast(keep[-1], C.c_void_p)
    out_bytes, valid_bytes = n * w + pad, words * 8 + pad
    out = to_device(np.full(out_bytes, 0xEE, np.uint8))
    valid = to_device(np.full(valid_bytes, 0xEE, np.uint8)) if with_validity else None
    rc = lib.arx_min_max_element_wise(NUM_TYPE[str(t).replace("float", "float32").replace("double", "float64")], OPS[op][1], 1 if skip_nulls else 0,
                                      table, len(operands), n, out.data_ptr(), valid.data_ptr() if with_validity else None, None)
    if out.is_cuda:
        torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:out_bytes], (valid.cpu().numpy()[:valid_bytes] if with_validity else None)


def check_c(amd, t, op, skip_nulls, operands, what):
    want = getattr(pc, OPS[op][0])(*operands, skip_nulls=skip_nulls)
    CW.check_raw(lambda v: c_min_max(amd, t, op, skip_nulls, operands, with_validity=v), want, len(want), t.byte_width,
                 result_can_be_null(operands, skip_nulls), b"NULL out_validity", what)


def _c_abi(amd):
    for name in ("uint8", "int16", "float32", "int64", "float64"):
        t = TYPES[name]
        five, null = pa.scalar(5, t), pa.scalar(None, t)
        for n in (1, 64, 65, 257, 1001, 4099):
            rng = rng_for("c abi", name, n)
            arrays = [column(rng, t, n + 80, 0.1).slice(OFFSETS[j], n) for j in range(3)]
            plain = column(rng, t, n + 80, 0.0).slice(OFFSETS[3], n)
            for op in OPS:
                for skip_nulls in (True, False):
                    check_c(amd, t, op, skip_nulls, arrays, (name, n, op, skip_nulls, "arrays"))
                    check_c(amd, t, op, skip_nulls, arrays[:2] + [plain], (name, n, op, skip_nulls, "arrays, one without nulls"))
                    if n in (65, 1001):
                        check_c(amd, t, op, skip_nulls, [arrays[0]], (name, n, op, skip_nulls, "one operand"))
                        check_c(amd, t, op, skip_nulls, [plain], (name, n, op, skip_nulls, "one operand without nulls"))
                        check_c(amd, t, op, skip_nulls, [five, arrays[0], null], (name, n, op, skip_nulls, "scalar / array / null"))
                        check_c(amd, t, op, skip_nulls, [plain, five], (name, n, op, skip_nulls, "no nulls, a scalar"))
                        check_c(amd, t, op, skip_nulls, [plain, plain, plain], (name, n, op, skip_nulls, "no nulls"))


def _invalid_arguments(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n = 100
    rng = rng_for("invalid")
    spans, keep = {}, []
    for which, null_p in (("a", 0.1), ("b", 0.1), ("p", 0.0)):
        spans[which], bufs = IE.c_operand(IE.column(rng, pa.int32(), n, null_p))
        keep.append(bufs)
    spans["short"] = _lib.ArxSpan(None, spans["p"].data, 0, n - 1, 0)
    spans["nodata"] = _lib.ArxSpan(None, None, 0, n, 0)
    for name in ("a", "p"):
        spans[name + "_0"] = _lib.ArxSpan(spans[name].validity, spans[name].data, 0, 0, 0)
    out = to_device(np.full(n * 4 + 64, 0xEE, np.uint8))
    valid = to_device(np.full(16 + 64, 0xEE, np.uint8))
    seven = C.c_int64(7)
    DEFAULT = object()

    def call(num_type=4, op=0, skip_nulls=1, operands=("a", "b"), length=n, o=out, v=valid, table=DEFAULT, count=None, both=None):
        if table is DEFAULT:
            table = (_lib.ArxOperand * max(len(operands), 1))()
            for j, k in enumerate(operands):
                if isinstance(k, str):
                    table[j].span = C.pointer(spans[k])
                elif k is not None:
                    table[j].scalar = C.cast(C.pointer(k), C.c_void_p)
            if both is not None:
                table[both].scalar = C.cast(C.pointer(seven), C.c_void_p)
        return lib.arx_min_max_element_wise(num_type, op, skip_nulls, table, len(operands) if count is None else count, length,
                                            o.data_ptr() if o is not None else None, v.data_ptr() if v is not None else None, None)

    for kwargs, text in (({"num_type": -1}, b"numeric type -1"), ({"num_type": 10}, b"numeric type 10"), ({"op": 2}, b"op 2"), ({"op": -1}, b"op -1"),
                         ({"operands": ()}, b"0 operands; the device kernel takes 1 to 32"),
                         ({"operands": ("p",) * 33}, b"33 operands; the device kernel takes 1 to 32"),
                         ({"length": -1}, b"negative length"), ({"table": None}, b"NULL operands"),
                         ({"operands": ("a", "short")}, b"of operand 1 is not length"), ({"length": n - 1}, b"of operand 0 is not length"),
                         ({"both": 1}, b"operand 1 is given as an array and as a scalar"), ({"o": None}, b"NULL out_data"),
                         ({"operands": ("a", "nodata")}, b"NULL data buffer of operand 1"),
                         ({"v": None}, b"NULL out_validity, but every operand"),                                      # skip_nulls: all can be null
                         ({"operands": ("a", None), "v": None}, b"NULL out_validity, but every operand"),
                         ({"operands": ("a", "p"), "skip_nulls": 0, "v": None}, b"NULL out_validity, but an operand"),
                         ({"operands": ("p", None), "skip_nulls": 0, "v": None}, b"NULL out_validity, but an operand")):
        assert call(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    untouched = lambda: (out.cpu().numpy()[: n * 4 + 64] == 0xEE).all() and (valid.cpu().numpy()[: 16 + 64] == 0xEE).all()  # noqa: E731
    assert untouched()
    # length 0 succeeds, launches nothing and writes nothing
    count = lambda: lib.arx_get_counter(b"element_wise_launches")  # noqa: E731
    before = count()
    for num_type in (0, 4, 7, 9):
        assert call(num_type=num_type, operands=("a_0", "p_0", seven), length=0) == 0
        assert call(num_type=num_type, operands=("a_0", "p_0"), length=0, o=None, v=None) == 0
    assert count() == before and untouched()
    # one launch per call; out_validity = NULL where the result cannot hold a null
    assert call() == 0 and count() == before + 1
    valid[:16] = 0xEE
    assert call(operands=("a", "p"), v=None) == 0 and count() == before + 2            # skip_nulls: one operand never null is enough
    assert call(operands=("a", seven), v=None) == 0 and count() == before + 3
    assert call(operands=("p", "p", seven), skip_nulls=0, v=None) == 0 and count() == before + 4
    assert (valid.cpu().numpy()[: 16 + 64] == 0xEE).all()


def _mirror(amd):
    from arrow_amd.array import int32, type_from_name

    rng = rng_for("mirror")
    n = 500
    a, b, p = IE.column(rng, pa.int32(), n, 0.1), IE.column(rng, pa.int32(), n, 0.1), IE.column(rng, pa.int32(), n, 0.0)
    da, db, dp = (amd.Array.from_pyarrow(x) for x in (a, b, p))
    s = lambda x: pa.scalar(x, pa.int32())  # noqa: E731
    for fn in ("min_element_wise", "max_element_wise"):
        mine, ref = getattr(amd.compute, fn), getattr(pc, fn)
        assert mine(da, db).to_pyarrow().equals(ref(a, b))
        assert mine(da, db, skip_nulls=False).to_pyarrow().equals(ref(a, b, skip_nulls=False))
        assert amd.compute.call_function(fn, [da, db]).to_pyarrow().equals(ref(a, b))
        options = amd.compute.ElementWiseAggregateOptions(skip_nulls=False)
        assert amd.compute.call_function(fn, [da, db], options).to_pyarrow().equals(ref(a, b, skip_nulls=False))
        assert fn in amd.compute.get_function_registry().get_function_names()
        # Python numbers take the other operands' type; None is a null scalar; arrow_amd.Scalar
        assert mine(da, 0).to_pyarrow().equals(ref(a, s(0)))
        assert mine(-5, da, None).to_pyarrow().equals(ref(s(-5), a, s(None)))
        assert mine(da, None, skip_nulls=False).to_pyarrow().equals(ref(a, s(None), skip_nulls=False))
        assert mine(amd.Scalar(9, int32), dp, 3).to_pyarrow().equals(ref(s(9), p, s(3)))
        assert mine(da).to_pyarrow().equals(a)                                               # one operand is a copy
        f64 = IE.column(rng, pa.float64(), n, 0.0)
        assert mine(1.5, amd.Array.from_pyarrow(f64)).to_pyarrow().equals(ref(pa.scalar(1.5), f64))
        # ---- refusals
        with pytest.raises(amd.ArrowNotImplementedError, match="operand 0 is int32, operand 1 is double"):
            mine(da, amd.Array.from_pyarrow(f64))
        with pytest.raises(amd.ArrowNotImplementedError, match="operand 0 is int32, operand 2 is int64"):
            mine(da, db, amd.Scalar(1, type_from_name("int64")))
        for untyped in ((1, 2), (None, 2), (None,)):
            with pytest.raises(amd.ArrowNotImplementedError, match="carries a type"):
                mine(*untyped)
        with pytest.raises(amd.ArrowNotImplementedError, match="of scalars only"):
            mine(amd.Scalar(1, int32), 2)
        for typ in (pa.string(), pa.binary(), pa.bool_()):
            odd = amd.Array.from_pyarrow(pa.array(["a", None, "c"] * 4, pa.string()).cast(typ) if typ != pa.bool_() else pa.array([True, None] * 6))
            with pytest.raises(amd.ArrowNotImplementedError, match="has no kernel matching input types") as err:
                mine(odd, odd)
            assert str(err.value) == f"Function '{fn}' has no kernel matching input types ({typ}, {typ})"
        with pytest.raises(amd.ArrowInvalid, match="same length"):
            mine(da, dp.slice(1))
        # ---- no validity buffer when the result cannot hold a null; null counts known or lazy
        for args, kwargs in (((dp, dp), {}), ((da, dp), {}), ((da, 7), {}), ((dp, 7), {"skip_nulls": False})):
            res = mine(*args, **kwargs)
            assert res.validity is None and res.null_count == 0
        lazy = mine(da, db)
        assert callable(lazy._null_count)
        assert lazy.null_count == ref(a, b).null_count and not callable(lazy._null_count)


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_min_max_element_wise_grid(emu_ctx, n):
    _grid(emu_ctx, n)


@pytest.mark.emu
def test_min_max_element_wise_operand_forms(emu_ctx):
    _operand_forms(emu_ctx)


@pytest.mark.emu
def test_min_max_element_wise_float_pins(emu_ctx):
    _pins(emu_ctx)


@pytest.mark.emu
def test_min_max_element_wise_integer_extremes(emu_ctx):
    _integer_extremes(emu_ctx)


@pytest.mark.emu
def test_min_max_element_wise_caps(emu_ctx):
    _caps(emu_ctx)


@pytest.mark.emu
def test_min_max_element_wise_c_abi_written_bytes(emu_ctx):
    _c_abi(emu_ctx)


@pytest.mark.emu
def test_min_max_element_wise_c_abi_invalid_arguments_length_zero_and_counters(emu_ctx):
    _invalid_arguments(emu_ctx)


@pytest.mark.emu
def test_min_max_element_wise_mirror(emu_ctx):
    _mirror(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
def test_gpu_min_max_element_wise_grid(gpu_ctx):
    for n in LENGTHS:
        _grid(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_min_max_element_wise_forms_pins_extremes_and_caps(gpu_ctx):
    _operand_forms(gpu_ctx)
    _pins(gpu_ctx)
    _integer_extremes(gpu_ctx)
    _caps(gpu_ctx)


@pytest.mark.gpu
def test_gpu_min_max_element_wise_c_abi(gpu_ctx):
    _c_abi(gpu_ctx)
    _invalid_arguments(gpu_ctx)


@pytest.mark.gpu
def test_gpu_min_max_element_wise_mirror(gpu_ctx):
    _mirror(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["int8", "uint64", "float64"])
def test_gpu_min_max_element_wise_1e6_rows_from_numpy_buffers(gpu_ctx, name):
    rng = rng_for("1e6", name)
    n = 1_000_000
    t = TYPES[name]

    def from_buffers(offset):
        total = n + offset
        valid = np.packbits(rng.random(total) >= 0.05, bitorder="little")
        if pa.types.is_floating(t):
            data = rng.standard_normal(total)
            data[rng.random(total) < 0.01] = np.nan
            data[rng.random(total) < 0.01] = -0.0
        else:
            dt = np.dtype(t.to_pandas_dtype())
            data = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, total, dtype=dt, endpoint=True)
        return pa.Array.from_buffers(t, total, [pa.py_buffer(valid.tobytes()), pa.py_buffer(data.tobytes())]).slice(offset)

    operands = [from_buffers(OFFSETS[j]) for j in range(3)]
    for op in OPS:
        for skip_nulls in (True, False):
            check(gpu_ctx, op, operands, skip_nulls, ("1e6", name, op, skip_nulls))
    check(gpu_ctx, "max", operands + [pa.scalar(0, t)], True, ("1e6, a scalar", name))
