"""case_when (arrow_amd.compute.case_when, arx_case_when, csrc/case_when.hip) against pyarrow.compute.case_when on the host
copies of the same arrays: values by `equals` (floats also by bit pattern), null_count and result offset 0 — exact
equality, no tolerances.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus columns of 10^6 rows built from numpy buffers.  Width 16 (decimal128) has no mirror type and goes through the
C ABI, as do the checks of what the call may and may not write.  Scalars are typed pyarrow scalars, so the reference
promotes nothing.  The column makers and the C-ABI upload helpers are those of tests/test_if_else.py."""
import ctypes as C
import decimal

import numpy as np
import pytest

from . import test_if_else as IE
from . import util as U

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

# rows one wave takes at a time (csrc/case_when.hip): 64 x kCaseWhenWords at widths 8 and 16, 64 x (8 / W) x
# kCaseWhenPackedSteps at widths 4, 2 and 1
ROWS_PER_WAVE = (256, 512, 1024, 2048)
LENGTHS = [0, 1, 63, 64, 65] + [r + d for r in ROWS_PER_WAVE for d in (-1, 1)] + [4097, 100_000]
TYPES = IE.TYPES
COND_OFFSETS = (13, 3, 29, 64, 7)          # every operand at its own bit alignment (the result's is 0)
VALUE_OFFSETS = (5, 70, 1, 66, 9)          # (the else is the value after the last cond's)


def rng_for(*key):
    return U.rng_for(0xCA5E, *key)


def cut(rng, t, n, null_p, offset):
    return IE.column(rng, t, n + offset + 3, null_p).slice(offset, n)


def cond_struct(conds):
    return pa.StructArray.from_arrays(list(conds), [f"c{j}" for j in range(len(conds))])


def bits_of(arr):
    """A float column's values as integers of its width (equals() tells neither +0 from -0 nor one NaN from another)."""
    width = {pa.float32(): np.uint32, pa.float64(): np.uint64}.get(arr.type)
    if width is None:
        return None
    a = arr.slice(0) if arr.offset == 0 else pa.concat_arrays([arr])
    return np.frombuffer(a.buffers()[1], dtype=width, count=len(a))


def assert_same(got, want, what):
    """got (a pyarrow array made of the device result's buffers) equals want: type, values, validity, float bit patterns."""
    assert got.type == want.type and len(got) == len(want), what
    assert got.null_count == want.null_count, (what, got.null_count, want.null_count)
    if bits_of(want) is None:
        assert got.equals(want), (what, str(want.type), len(want))
    elif len(want):                                            # (equals() is false for a NaN against itself)
        valid = np.asarray(pc.is_valid(want))
        assert (np.asarray(pc.is_valid(got)) == valid).all(), (what, "validity")
        assert (bits_of(got)[valid] == bits_of(want)[valid]).all(), (what, "bit patterns")


def cannot_be_null(values, num_conds):
    return len(values) == num_conds + 1 and all((x.null_count == 0 or x.buffers()[0] is None) if isinstance(x, pa.Array) else x.is_valid
                                                for x in values)


def check(amd, conds, values, what=()):
    want = pc.case_when(cond_struct(conds), *values)
    got = amd.compute.case_when([amd.Array.from_pyarrow(c) for c in conds], *[IE.amd_operand(amd, v) for v in values])
    assert got.offset == 0 and got.length == len(want), what
    assert_same(got.to_pyarrow(), want, what)
    assert got.null_count == want.null_count, (what, got.null_count, want.null_count)
    if cannot_be_null(values, len(conds)):
        assert got.validity is None, what
    return got


def _grid(amd, n):
    for name, t in TYPES.items():
        for k in (1, 2, 3):
            for with_else in (False, True):
                for nulls in range(8 if with_else else 4):
                    p_conds, p_values, p_else = (0.1 if nulls & bit else 0.0 for bit in (1, 2, 4))
                    rng = rng_for("grid", n, name, k, with_else, nulls)
                    conds = [cut(rng, pa.bool_(), n, p_conds, COND_OFFSETS[j]) for j in range(k)]
                    values = [cut(rng, t, n, p_values, VALUE_OFFSETS[j]) for j in range(k)]
                    if with_else:
                        values.append(cut(rng, t, n, p_else, VALUE_OFFSETS[k]))
                    check(amd, conds, values, ("grid", n, name, k, with_else, nulls))


def _operand_forms(amd):
    n = 1000
    for name in ("int16", "int64", "bool"):
        t = TYPES[name]
        rng = rng_for("forms", name)
        conds = [cut(rng, pa.bool_(), n, 0.1, COND_OFFSETS[j]) for j in range(2)]
        one = pa.scalar(True, t) if name == "bool" else pa.scalar(-12345, t)
        forms = lambda j: {"array": cut(rng, t, n, 0.1, VALUE_OFFSETS[j]), "scalar": one, "null": pa.scalar(None, t)}  # noqa: E731
        for f0, v0 in forms(0).items():
            for f1, v1 in forms(1).items():
                got = check(amd, conds, [v0, v1], ("forms", name, f0, f1))
                if f0 == f1 == "null":
                    assert not callable(got._null_count) and got.null_count == n      # known without a read-back
                for f2, v2 in forms(2).items():
                    check(amd, conds, [v0, v1, v2], ("forms", name, f0, f1, f2))
        # an else, and no value can be null: no validity buffer, whatever the conds hold
        plain = lambda j: cut(rng, t, n, 0.0, VALUE_OFFSETS[j])  # noqa: E731
        for values in ([plain(0), plain(1), plain(2)], [one, plain(1), one], [one, one, one]):
            assert check(amd, conds, values, ("forms no nulls", name)).validity is None


def _skips_and_early_exit(amd):
    n = 64 * 9 + 37
    rows = np.arange(n)
    shifted = lambda bits, off: pa.array(np.concatenate([np.zeros(off, bool), bits])).slice(off)  # noqa: E731
    for name in ("int8", "int32", "int64", "bool"):
        t = TYPES[name]
        for null_p in (0.0, 0.1):
            rng = rng_for("skips", name, null_p)
            values = [cut(rng, t, n, null_p, VALUE_OFFSETS[j]) for j in range(4)]
            random_conds = [cut(rng, pa.bool_(), n, null_p, COND_OFFSETS[j]) for j in range(3)]
            all_false = [shifted(np.zeros(n, bool), COND_OFFSETS[j]) for j in range(3)]
            check(amd, all_false, values[:3], ("all conds false", name, null_p))
            check(amd, all_false, values, ("all conds false, else", name, null_p))
            first_true = [shifted(np.ones(n, bool), COND_OFFSETS[0])] + random_conds[1:]
            check(amd, first_true, values, ("first cond all true", name, null_p))
            check(amd, first_true, [values[0], pa.scalar(None, t), values[2]], ("first cond all true, no else", name, null_p))
            # the first cond takes whole words, the second the others: a word's rows all come from one stream
            by_word = [shifted((rows // 64) % 2 == 0, COND_OFFSETS[0]), shifted(np.ones(n, bool), COND_OFFSETS[1])]
            check(amd, by_word, values[:3], ("alternating words", name, null_p))
            # a cond that is true only in null slots takes nothing
            dead = rng.random(n) < 0.4
            only_null = pa.Array.from_buffers(pa.bool_(), n, [pa.py_buffer(np.packbits(~dead, bitorder="little").tobytes()),
                                                              pa.py_buffer(np.packbits(dead, bitorder="little").tobytes())])
            assert only_null.null_count == int(dead.sum()) and not pc.any(only_null).as_py()
            got = check(amd, [only_null, random_conds[1]], values[:3], ("true only in null slots", name, null_p))
            assert_same(got.to_pyarrow(), pc.case_when(cond_struct([random_conds[1]]), values[1], values[2]), "the dead cond drops out")


def _null_slots_are_zero(amd):
    n = 300
    rng = rng_for("null slots")
    garbage = lambda: pa.Array.from_buffers(pa.int32(), n, [pa.py_buffer(np.packbits(rng.random(n) >= 0.3, bitorder="little").tobytes()),  # noqa: E731
                                                             pa.py_buffer(rng.integers(1, 2**31, n, dtype=np.int32).tobytes())])
    conds = [IE.column(rng, pa.bool_(), n, 0.1) for _ in range(2)]
    values = [garbage(), garbage()]
    got = check(amd, conds, values, "garbage under nulls")
    data = got.data.cpu().numpy()[: n * 4].view(np.int32)
    assert (data[~np.asarray(pc.is_valid(pc.case_when(cond_struct(conds), *values)))] == 0).all()


def _caps(amd):
    n = 200
    rng = rng_for("caps")
    conds = [pa.array(rng.random(n) < 0.08, pa.bool_()) for _ in range(17)]
    values = [IE.column(rng, pa.int32(), n, 0.1) for _ in range(18)]
    check(amd, conds[:16], values[:16], "16 conds")
    check(amd, conds[:16], values[:17], "16 conds and an else")
    dconds = [amd.Array.from_pyarrow(c) for c in conds]
    dvalues = [amd.Array.from_pyarrow(v) for v in values]
    with pytest.raises(amd.ArrowNotImplementedError, match="17 conds on device-resident arrays: the device kernel takes up to 16"):
        amd.compute.case_when(dconds, *dvalues[:17])


# ---------------------------------------------------------------- the C ABI directly
def c_case_when(amd, t, conds, values, with_validity=True, pad=64):
    """arx_case_when on host pyarrow operands: (rc, raw data bytes, raw validity bytes | None); both output buffers are
    filled with 0xEE first and carry `pad` bytes after what the call may write."""
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n, w = len(conds[0]), IE.width_of(t)
    words = (n + 63) // 64
    keep = []
    cspans = []
    for c in conds:
        span, bufs = IE.c_operand(c)
        keep.append(bufs)
        cspans.append(span)
    ctable = (C.POINTER(_lib.ArxSpan) * len(conds))(*[C.pointer(s) for s in cspans])
    vtable = (_lib.ArxOperand * len(values))()
    for j, x in enumerate(values):
        if isinstance(x, pa.Array):
            span, bufs = IE.c_operand(x)
            keep.extend([span, bufs])
            vtable[j].span = C.pointer(span)
        elif x.is_valid:
            raw = IE.c_scalar_bytes(x)
            keep.append(C.create_string_buffer(raw, len(raw)))
            vtable[j].scalar = C.cast(keep[-1], C.c_void_p)
    out_bytes, valid_bytes = (words * 8 if w == 0 else n * w) + pad, words * 8 + pad
    out = to_device(np.full(out_bytes, 0xEE, np.uint8))
    valid = to_device(np.full(valid_bytes, 0xEE, np.uint8)) if with_validity else None
    rc = lib.arx_case_when(w, ctable, len(conds), vtable, len(values), n, out.data_ptr(), valid.data_ptr() if with_validity else None, None)
    if out.is_cuda:
        torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:out_bytes], (valid.cpu().numpy()[:valid_bytes] if with_validity else None)


def check_raw(call, want, n, w, nullable, needs_text, what):
    """The raw outputs of a C-ABI call equal the reference, null slots are zero, nothing else is written, and
    out_validity = NULL is accepted exactly when nothing can be null."""
    from arrow_amd import _lib

    lib = _lib.get_lib()
    words = (n + 63) // 64
    rc, data, valid = call(True)
    assert rc == 0, (what, lib.arx_last_error())
    nbytes = words * 8 if w == 0 else n * w
    assert (data[nbytes:] == 0xEE).all(), what                        # nothing past length * width (bool: the last word)
    assert (valid[words * 8:] == 0xEE).all(), what                    # nothing past the last validity word
    vbits = np.unpackbits(valid[: words * 8], bitorder="little")
    assert not vbits[n:].any(), what                                   # pad bits beyond length: zero
    got = pa.Array.from_buffers(want.type, n, [pa.py_buffer(valid[: words * 8].tobytes()), pa.py_buffer(data[:nbytes].tobytes())])
    assert_same(got, want, what)
    is_null = ~vbits[:n].astype(bool)
    if w == 0:
        dbits = np.unpackbits(data[:nbytes], bitorder="little")
        assert not dbits[n:].any() and not dbits[:n][is_null].any(), what
    else:
        assert not data[:nbytes].reshape(n, w)[is_null].any(), what    # null slots: zero
    rc, data2, _ = call(False)
    if nullable:
        assert rc == _lib.ARX_INVALID and needs_text in lib.arx_last_error(), what
        assert (data2 == 0xEE).all(), what
    else:
        assert rc == 0 and (data2 == data).all() and vbits[:n].all(), what


def check_c(amd, t, conds, values, what):
    want = pc.case_when(cond_struct(conds), *values)
    check_raw(lambda v: c_case_when(amd, t, conds, values, with_validity=v), want, len(conds[0]), IE.width_of(t),
              not cannot_be_null(values, len(conds)), b"NULL out_validity", what)


def _c_abi(amd):
    dec = pa.decimal128(38, 4)
    raw_types = {16: dec, 1: pa.uint8(), 2: pa.uint16(), 4: pa.uint32(), 8: pa.uint64(), 0: pa.bool_()}
    for w, t in raw_types.items():
        make = IE.decimal_column if w == 16 else IE.column
        scalar = pa.scalar(True, t) if w == 0 else (pa.scalar(decimal.Decimal("-1234567890123456789012.3456"), t) if w == 16 else pa.scalar(201, t))
        null = pa.scalar(None, t)
        for n in (1, 64, 65, 257, 1001, 2049):
            rng = rng_for("c abi", w, n)
            conds = [IE.column(rng, pa.bool_(), n + 80, 0.1).slice(COND_OFFSETS[j], n) for j in range(3)]
            vals = [make(rng, t, n + 80, 0.1).slice(VALUE_OFFSETS[j], n) for j in range(4)]
            check_c(amd, t, conds, vals, (w, n, "arrays, else"))
            check_c(amd, t, conds, vals[:3], (w, n, "arrays"))
            if n in (65, 1001):
                check_c(amd, t, conds[:1], [vals[0], scalar], (w, n, "array / scalar"))
                check_c(amd, t, conds[:2], [scalar, vals[1], null], (w, n, "scalar / array / null"))
                check_c(amd, t, conds[:2], [null, null], (w, n, "null / null"))
                plain = [make(rng, t, n + 80, 0.0).slice(VALUE_OFFSETS[j], n) for j in range(3)]
                check_c(amd, t, conds[:2], plain, (w, n, "no nulls"))
                check_c(amd, t, conds[:2], plain[:2], (w, n, "no nulls, no else"))      # (a row no cond takes is null)
                check_c(amd, t, conds[:2], [scalar, plain[1], scalar], (w, n, "no nulls, scalars"))


def _invalid_arguments(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n = 100
    rng = rng_for("invalid")
    spans, keep = {}, []
    for which, t, null_p in (("c0", pa.bool_(), 0.1), ("c1", pa.bool_(), 0.0), ("v0", pa.int32(), 0.0), ("v1", pa.int32(), 0.0),
                             ("v2", pa.int32(), 0.0), ("vn", pa.int32(), 0.2), ("b0", pa.bool_(), 0.0), ("w0", pa.int64(), 0.0),
                             ("q0", pa.int8(), 0.0)):
        spans[which], bufs = IE.c_operand(IE.column(rng, t, n, null_p))
        keep.append(bufs)
    spans["short"] = _lib.ArxSpan(None, spans["v0"].data, 0, n - 1, 0)
    spans["nodata"] = _lib.ArxSpan(None, None, 0, n, 0)
    for name in ("c0", "c1", "v0", "v1", "v2"):
        spans[name + "_0"] = _lib.ArxSpan(spans[name].validity, spans[name].data, 0, 0, 0)
    out = to_device(np.full(n * 8 + 64, 0xEE, np.uint8))
    valid = to_device(np.full(16 + 64, 0xEE, np.uint8))
    seven = C.c_int64(7)
    DEFAULT = object()

    def call(width=4, conds=("c0", "c1"), values=("v0", "v1", "v2"), length=n, o=out, v=valid, num_conds=None, num_values=None,
             ctable=DEFAULT, vtable=DEFAULT, both=None):
        if ctable is DEFAULT:
            ctable = (C.POINTER(_lib.ArxSpan) * max(len(conds), 1))(*[C.pointer(spans[k]) if k is not None else None for k in conds])
        if vtable is DEFAULT:
            vtable = (_lib.ArxOperand * max(len(values), 1))()
            for j, k in enumerate(values):
                if isinstance(k, str):
                    vtable[j].span = C.pointer(spans[k])
                elif k is not None:
                    vtable[j].scalar = C.cast(C.pointer(k), C.c_void_p)
            if both is not None:
                vtable[both].scalar = C.cast(C.pointer(seven), C.c_void_p)
        return lib.arx_case_when(width, ctable, len(conds) if num_conds is None else num_conds, vtable,
                                 len(values) if num_values is None else num_values, length, o.data_ptr() if o is not None else None,
                                 v.data_ptr() if v is not None else None, None)

    many = ("c1",) * 17
    for kwargs, text in (({"width": 3}, b"byte_width 3"), ({"width": 32}, b"byte_width 32"), ({"width": -1}, b"byte_width -1"),
                         ({"conds": ()}, b"0 conds; the device kernel takes 1 to 16"),
                         ({"conds": many, "values": ("v0",) * 17}, b"17 conds; the device kernel takes 1 to 16"),
                         ({"values": ("v0",)}, b"1 values for 2 conds"), ({"values": ("v0",) * 4}, b"4 values for 2 conds"),
                         ({"length": -1}, b"negative length"), ({"ctable": None}, b"NULL conds"), ({"vtable": None}, b"NULL values"),
                         ({"conds": ("c0", None)}, b"NULL cond 1"),
                         ({"values": ("v0", "short", "v2")}, b"of value 1 is not length"), ({"length": n - 1}, b"of cond 0 is not length"),
                         ({"both": 2}, b"value 2 is given as an array and as a scalar"),
                         ({"o": None}, b"NULL out_data"), ({"values": ("v0", "nodata", "v2")}, b"NULL data buffer of value 1"),
                         ({"conds": ("c0", "nodata")}, b"NULL data buffer of cond 1"),
                         ({"values": ("v0", "v1"), "v": None}, b"NULL out_validity"),             # no else
                         ({"values": ("v0", "vn", "v2"), "v": None}, b"NULL out_validity"),       # a value with a bitmap
                         ({"values": ("v0", "v1", None), "v": None}, b"NULL out_validity")):      # a null scalar
        assert call(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    untouched = lambda: (out.cpu().numpy()[: n * 8 + 64] == 0xEE).all() and (valid.cpu().numpy()[: 16 + 64] == 0xEE).all()  # noqa: E731
    assert untouched()
    # length 0 succeeds, launches nothing and writes nothing
    count = lambda: tuple(lib.arx_get_counter(name) for name in (b"case_when_launches", b"case_when_packed_launches", b"case_when_bool_launches"))  # noqa: E731
    before = count()
    for width in (0, 1, 4, 16):
        zero = {"conds": ("c0_0", "c1_0"), "values": ("v0_0", "v1_0", "v2_0"), "length": 0}
        assert call(width=width, **zero) == 0 and call(width=width, o=None, v=None, **zero) == 0
    assert count() == before and untouched()
    # one launch of the kernel of its kind per call: widths 8 and 16, widths 1 / 2 / 4, booleans
    assert call() == 0 and count() == (before[0], before[1] + 1, before[2])
    valid[:16] = 0xEE
    assert call(v=None) == 0 and count() == (before[0], before[1] + 2, before[2])      # an else, nothing can be null: no bitmap asked for
    assert (valid.cpu().numpy()[: 16 + 64] == 0xEE).all()
    assert call(width=1, values=("q0", "q0")) == 0 and count() == (before[0], before[1] + 3, before[2])
    assert call(width=8, values=("w0", "w0", seven)) == 0 and count() == (before[0] + 1, before[1] + 3, before[2])
    assert call(width=0, values=("b0", "c1")) == 0 and count() == (before[0] + 1, before[1] + 3, before[2] + 1)


def _mirror(amd):
    from arrow_amd.array import StructArray, bool_, int32, type_from_name

    rng = rng_for("mirror")
    n = 500
    conds = [IE.column(rng, pa.bool_(), n, 0.1) for _ in range(2)]
    v0, v1, v2 = IE.column(rng, pa.int32(), n, 0.1), IE.column(rng, pa.int32(), n, 0.0), IE.column(rng, pa.int32(), n, 0.0)
    dconds = [amd.Array.from_pyarrow(c) for c in conds]
    d0, d1, d2 = (amd.Array.from_pyarrow(a) for a in (v0, v1, v2))
    struct = cond_struct(conds)
    want = pc.case_when(struct, v0, v1, v2)
    assert amd.compute.case_when(dconds, d0, d1, d2).to_pyarrow().equals(want)
    assert amd.compute.case_when(tuple(dconds), d0, d1, d2).to_pyarrow().equals(want)
    assert amd.compute.call_function("case_when", [dconds, d0, d1, d2]).to_pyarrow().equals(want)
    assert amd.compute.case_when(StructArray(struct.type, n, [None], dconds), d0, d1, d2).to_pyarrow().equals(want)
    assert "case_when" in amd.compute.get_function_registry().get_function_names()
    # the pins of the reference: a null cond is false; no else: null where no cond is true
    pin_conds = [pa.array([True, None, False, False]), pa.array([True, True, False, None])]
    pin_values = [pa.array([1, 2, 3, 4], pa.int32()), pa.array([10, 20, 30, 40], pa.int32())]
    pin = lambda *vs: amd.compute.case_when([amd.Array.from_pyarrow(c) for c in pin_conds], *[amd.Array.from_pyarrow(v) for v in vs])  # noqa: E731
    assert pc.case_when(cond_struct(pin_conds), *pin_values).to_pylist() == [1, 20, None, None]
    assert pin(*pin_values).to_pylist() == [1, 20, None, None]
    assert pin(*pin_values, pa.array([7, 7, None, 7], pa.int32())).to_pylist() == [1, 20, None, 7]
    flags = [pa.array([True, False, True, None]), pa.array([False, False, None, True])]
    assert pin(*flags).to_pylist() == pc.case_when(cond_struct(pin_conds), *flags).to_pylist() == [True, False, None, None]
    # Python scalars take the other values' type; None is a null scalar; arrow_amd.Scalar
    s = lambda x: pa.scalar(x, pa.int32())  # noqa: E731
    assert amd.compute.case_when(dconds, d0, 0).to_pyarrow().equals(pc.case_when(struct, v0, s(0)))
    assert amd.compute.case_when(dconds, -5, d1, None).to_pyarrow().equals(pc.case_when(struct, s(-5), v1, s(None)))
    assert amd.compute.case_when(dconds, None, amd.Scalar(9, int32), 3).to_pyarrow().equals(pc.case_when(struct, s(None), s(9), s(3)))
    f64 = IE.column(rng, pa.float64(), n, 0.0)
    assert amd.compute.case_when(dconds, 1.5, amd.Array.from_pyarrow(f64)).to_pyarrow().equals(pc.case_when(struct, pa.scalar(1.5), f64))
    # ---- refusals
    with pytest.raises(amd.ArrowNotImplementedError, match="value 0 is int32, value 1 is double"):
        amd.compute.case_when(dconds, d0, amd.Array.from_pyarrow(f64))
    with pytest.raises(amd.ArrowNotImplementedError, match="value 0 is int32, value 2 is int64"):
        amd.compute.case_when(dconds, d0, d1, amd.Scalar(1, type_from_name("int64")))
    with pytest.raises(amd.ArrowNotImplementedError, match="every cond must be a boolean arrow_amd.Array, not int32"):
        amd.compute.case_when([dconds[0], d0], d0, d1)
    with pytest.raises(amd.ArrowNotImplementedError, match="every cond must be a boolean arrow_amd.Array, not bool"):
        amd.compute.case_when([amd.Scalar(True, bool_)], d0)
    for untyped in ((1, 2), (None, 2, 3), (None, None), (True, False)):
        with pytest.raises(amd.ArrowNotImplementedError, match="carries a type"):
            amd.compute.case_when(dconds, *untyped)
    short_conds = [amd.Array.from_pyarrow(pa.array([True, False, None] * 4))]
    for typ in (pa.string(), pa.binary()):
        strings = amd.Array.from_pyarrow(pa.array(["a", None, "c"] * 4, pa.string()).cast(typ))
        for args in ((strings, strings), (strings, None), (None, strings)):
            with pytest.raises(amd.ArrowNotImplementedError, match="has no kernel matching input types") as err:
                amd.compute.case_when(short_conds, *args)
            assert str(err.value) == f"Function 'case_when' has no kernel matching input types (struct<bool>, {typ}, {typ})"
    with pytest.raises(amd.ArrowInvalid, match="same length"):
        amd.compute.case_when(short_conds, d0, d1)
    # the reference's texts for the struct: top-level nulls, a null scalar, and the field count
    with_nulls = pa.StructArray.from_arrays(conds, ["a", "b"], mask=pa.array(rng.random(n) < 0.1))
    with pytest.raises(pa.ArrowInvalid, match="cond struct must not be a null scalar or have top-level nulls"):
        pc.case_when(with_nulls, v0, v1)
    top_bitmap = amd.Array.from_pyarrow(IE.column(rng, pa.bool_(), n, 0.0)).data
    with pytest.raises(amd.ArrowInvalid, match="cond struct must not be a null scalar or have top-level nulls"):
        amd.compute.case_when(StructArray(struct.type, n, [top_bitmap], dconds, null_count=with_nulls.null_count), d0, d1)
    with pytest.raises(amd.ArrowInvalid, match="cond struct must not be a null scalar or have top-level nulls"):
        amd.compute.case_when(None, d0, d1)
    for values, host in (((d0,), (v0,)), ((d0, d1, d2, d0), (v0, v1, v2, v0))):
        text = f"case_when: number of struct fields must be equal to or one less than count of remaining arguments \\({len(values)}\\), got: 2"
        with pytest.raises(pa.ArrowInvalid, match=text):
            pc.case_when(struct, *host)
        with pytest.raises(amd.ArrowInvalid, match=text):
            amd.compute.case_when(dconds, *values)
    # ---- no validity buffer when nothing can be null; null counts known or lazy
    no_nulls = amd.compute.case_when(dconds, d1, d2, 7)
    assert no_nulls.validity is None and no_nulls.null_count == 0
    lazy = amd.compute.case_when(dconds, d0, d1)
    assert callable(lazy._null_count)
    assert lazy.null_count == pc.case_when(struct, v0, v1).null_count and not callable(lazy._null_count)


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_case_when_grid(emu_ctx, n):
    _grid(emu_ctx, n)


@pytest.mark.emu
def test_case_when_operand_forms(emu_ctx):
    _operand_forms(emu_ctx)


@pytest.mark.emu
def test_case_when_skips_and_early_exit(emu_ctx):
    _skips_and_early_exit(emu_ctx)
    _null_slots_are_zero(emu_ctx)


@pytest.mark.emu
def test_case_when_caps(emu_ctx):
    _caps(emu_ctx)


@pytest.mark.emu
def test_case_when_c_abi_widths_and_written_bytes(emu_ctx):
    _c_abi(emu_ctx)


@pytest.mark.emu
def test_case_when_c_abi_invalid_arguments_length_zero_and_counters(emu_ctx):
    _invalid_arguments(emu_ctx)


@pytest.mark.emu
def test_case_when_mirror(emu_ctx):
    _mirror(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
def test_gpu_case_when_grid(gpu_ctx):
    for n in LENGTHS:
        _grid(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_case_when_forms_skips_and_caps(gpu_ctx):
    _operand_forms(gpu_ctx)
    _skips_and_early_exit(gpu_ctx)
    _null_slots_are_zero(gpu_ctx)
    _caps(gpu_ctx)


@pytest.mark.gpu
def test_gpu_case_when_c_abi(gpu_ctx):
    _c_abi(gpu_ctx)
    _invalid_arguments(gpu_ctx)


@pytest.mark.gpu
def test_gpu_case_when_mirror(gpu_ctx):
    _mirror(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["int8", "int64", "bool"])
def test_gpu_case_when_1e6_rows_from_numpy_buffers(gpu_ctx, name):
    rng = rng_for("1e6", name)
    n = 1_000_000
    t = TYPES[name]

    def from_buffers(typ, offset):
        total = n + offset
        valid = np.packbits(rng.random(total) >= 0.05, bitorder="little")
        if pa.types.is_boolean(typ):
            data = np.packbits(rng.random(total) < 0.5, bitorder="little")
        else:
            dt = np.dtype(typ.to_pandas_dtype())
            data = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, total, dtype=dt, endpoint=True)
        return pa.Array.from_buffers(typ, total, [pa.py_buffer(valid.tobytes()), pa.py_buffer(data.tobytes())]).slice(offset)

    conds = [from_buffers(pa.bool_(), COND_OFFSETS[j]) for j in range(3)]
    values = [from_buffers(t, VALUE_OFFSETS[j]) for j in range(4)]
    check(gpu_ctx, conds, values, ("1e6", name))
    check(gpu_ctx, conds, values[:3], ("1e6, no else", name))
    check(gpu_ctx, conds, [values[0], pa.scalar(True, t) if name == "bool" else pa.scalar(3, t), values[2]], ("1e6, a scalar", name))
