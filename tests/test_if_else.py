"""if_else (arrow_amd.compute.if_else, arx_if_else, csrc/if_else.hip) against pyarrow.compute.if_else on the host copies
of the same arrays: values by `equals`, null_count and result offset 0 — exact equality, no tolerances.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus three columns of 10^6 rows built from numpy buffers.  Width 16 (decimal128) has no mirror type and goes
through the C ABI, as do the checks of what the call may and may not write.  Scalars are typed pyarrow scalars, so the
reference promotes nothing."""
import ctypes as C

import numpy as np
import pytest

from . import util as U

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

# rows one wave takes at a time (csrc/if_else.hip): 64 x kIfElseWords at widths 8 and 16 (and 4: 64 x 2 x kIfElsePackedSteps),
# 512 at width 2, 1024 at width 1
ROWS_PER_WAVE = (256, 512, 1024)
LENGTHS = [0, 1, 63, 64, 65] + [r + d for r in ROWS_PER_WAVE for d in (-1, 1)] + [4097, 100_000]
TYPES = {"int8": pa.int8(), "int16": pa.int16(), "int32": pa.int32(), "float32": pa.float32(), "int64": pa.int64(),
         "float64": pa.float64(), "timestamp[us]": pa.timestamp("us"), "bool": pa.bool_()}
OFFSETS = {"cond": 13, "left": 5, "right": 70}       # four bit alignments at once (the result's is 0)


def rng_for(*key):
    return U.rng_for(0x1FE, *key)


def column(rng, t, n, null_p):
    """n random rows of type t; null slots keep their (random, mostly non-zero) values underneath."""
    mask = (rng.random(n) < null_p) if null_p else None
    if pa.types.is_boolean(t):
        return pa.array(rng.random(n) < 0.5, t, mask=mask)
    if pa.types.is_floating(t):
        return pa.array(rng.standard_normal(n).astype(t.to_pandas_dtype()), t, mask=mask)
    if pa.types.is_timestamp(t):
        return pa.array(rng.integers(-2**62, 2**62, n, dtype=np.int64), pa.int64(), mask=mask).view(t)
    dt = np.dtype(t.to_pandas_dtype())
    return pa.array(rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, n, dtype=dt, endpoint=True), t, mask=mask)


def sliced(rng, t, n, null_p, which):
    off = OFFSETS[which]
    return column(rng, t, n + off + 3, null_p).slice(off, n)


def amd_operand(amd, x):
    """The mirror's twin of a host operand: an Array on the device, or an arrow_amd.Scalar of the same type."""
    from arrow_amd.array import type_from_name

    if isinstance(x, pa.Array):
        return amd.Array.from_pyarrow(x)
    value = None if not x.is_valid else (x.value if pa.types.is_timestamp(x.type) else x.as_py())
    return amd.Scalar(value, type_from_name(str(x.type)), x.is_valid)


def check(amd, cond, left, right, what=()):
    want = pc.if_else(cond, left, right)
    got = amd.compute.if_else(amd.Array.from_pyarrow(cond), amd_operand(amd, left), amd_operand(amd, right))
    assert got.offset == 0 and got.length == len(want), what
    assert got.to_pyarrow().equals(want), (what, str(want.type), len(want))
    assert got.null_count == want.null_count, (what, got.null_count, want.null_count)
    if want.null_count == 0 and not any(isinstance(x, pa.Array) and x.null_count for x in (cond, left, right)) \
            and all(x.is_valid for x in (left, right) if isinstance(x, pa.Scalar)):
        assert got.validity is None, what
    return got


def _grid(amd, n):
    for name, t in TYPES.items():
        for nulls in range(8):
            pc_, pl, pr = (0.1 if nulls & bit else 0.0 for bit in (1, 2, 4))
            rng = rng_for("grid", n, name, nulls)
            check(amd, sliced(rng, pa.bool_(), n, pc_, "cond"), sliced(rng, t, n, pl, "left"), sliced(rng, t, n, pr, "right"),
                  ("grid", n, name, nulls))


def _operand_forms(amd):
    n = 1000
    for name in ("int16", "int64", "bool"):
        t = TYPES[name]
        rng = rng_for("forms", name)
        cond = sliced(rng, pa.bool_(), n, 0.1, "cond")
        one = pa.scalar(True, t) if name == "bool" else pa.scalar(-12345, t)
        two = pa.scalar(False, t) if name == "bool" else pa.scalar(777, t)
        lefts = {"array": sliced(rng, t, n, 0.1, "left"), "scalar": one, "null": pa.scalar(None, t)}
        rights = {"array": sliced(rng, t, n, 0.1, "right"), "scalar": two, "null": pa.scalar(None, t)}
        for lf, left in lefts.items():
            for rf, right in rights.items():
                got = check(amd, cond, left, right, ("forms", name, lf, rf))
                if lf == rf == "null":
                    assert not callable(got._null_count) and got.null_count == n      # known without a read-back
        # no operand can be null: no validity buffer
        plain = sliced(rng, pa.bool_(), n, 0.0, "cond")
        for left, right in ((sliced(rng, t, n, 0.0, "left"), two), (one, sliced(rng, t, n, 0.0, "right")), (one, two)):
            assert check(amd, plain, left, right, ("forms no nulls", name)).validity is None


def _cond_patterns(amd):
    n = 64 * 9 + 37
    words = (n + 63) // 64
    rows = np.arange(n)
    patterns = {"all true": np.ones(n, bool), "all false": np.zeros(n, bool), "alternating words": (rows // 64) % 2 == 0}
    one_false = np.ones(n, bool)
    one_false[[64 * 2 + 63, 64 * 5, n - 1]] = False            # a single differing bit in an otherwise uniform word
    patterns["single false bits"] = one_false
    one_true = np.zeros(n, bool)
    one_true[[0, 64 * 3 + 31, 64 * (words - 1)]] = True
    patterns["single true bits"] = one_true
    for name in ("int8", "int32", "int64", "bool"):
        t = TYPES[name]
        for pname, bits in patterns.items():
            for null_p in (0.0, 0.1):
                rng = rng_for("patterns", name, pname, null_p)
                cond = pa.array(np.concatenate([np.zeros(OFFSETS["cond"], bool), bits])).slice(OFFSETS["cond"])
                check(amd, cond, sliced(rng, t, n, null_p, "left"), sliced(rng, t, n, null_p, "right"), (pname, name, null_p))
                if null_p:
                    # a null side under a uniform word: nothing valid is taken from it
                    check(amd, cond, pa.scalar(None, t), sliced(rng, t, n, null_p, "right"), (pname, name, "null left"))
                    check(amd, cond, sliced(rng, t, n, null_p, "left"), pa.scalar(None, t), (pname, name, "null right"))


def _null_slots(amd):
    n = 300
    rng = rng_for("null slots")
    # null cond slots whose data bit is 1: the result is null there, whatever the bit says
    valid = rng.random(n) >= 0.3
    cond = pa.Array.from_buffers(pa.bool_(), n, [pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()),
                                                 pa.py_buffer(b"\xff" * ((n + 7) // 8))])
    assert cond.null_count == int((~valid).sum()) and cond.fill_null(False).to_pylist() == valid.tolist()
    for name in ("int32", "bool"):
        t = TYPES[name]
        got = check(amd, cond, column(rng, t, n, 0.0), column(rng, t, n, 0.0), ("null cond, data bit 1", name))
        assert got.null_count == cond.null_count
    # null left / right slots holding non-zero garbage
    lvalid, rvalid = rng.random(n) >= 0.3, rng.random(n) >= 0.3
    garbage = lambda v: pa.Array.from_buffers(pa.int32(), n, [pa.py_buffer(np.packbits(v, bitorder="little").tobytes()),  # noqa: E731
                                                              pa.py_buffer(rng.integers(1, 2**31, n, dtype=np.int32).tobytes())])
    left, right = garbage(lvalid), garbage(rvalid)
    c = column(rng, pa.bool_(), n, 0.1)
    got = check(amd, c, left, right, "garbage under nulls")
    data = got.data.cpu().numpy()[: n * 4].view(np.int32)
    assert (data[~np.array(pc.is_valid(pc.if_else(c, left, right)).to_pylist())] == 0).all()      # a null result slot: zero


# ---------------------------------------------------------------- the C ABI directly
def width_of(t):
    return 0 if pa.types.is_boolean(t) else t.byte_width


def c_operand(arr):
    """(ArxSpan, kept device buffers) of a host pyarrow array: its buffers uploaded as they are, offset and all."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    vb, db = arr.buffers()[:2]
    w = width_of(arr.type)
    end = arr.offset + len(arr)
    data = np.frombuffer(db, dtype=np.uint8)[: (end + 7) // 8 if w == 0 else end * w]
    keep = [to_device(np.frombuffer(vb, dtype=np.uint8)[: (end + 7) // 8]) if vb is not None else None, to_device(data)]
    return _lib.ArxSpan(keep[0].data_ptr() if keep[0] is not None else None, keep[1].data_ptr(), arr.offset, len(arr),
                        arr.null_count if vb is not None else 0), keep


def c_scalar_bytes(s):
    """The host bytes arx_if_else takes for a valid scalar (None for a null one)."""
    if not s.is_valid:
        return None
    if pa.types.is_boolean(s.type):
        return bytes([1 if s.as_py() else 0])
    return pa.array([s.as_py()], s.type).buffers()[1].to_pybytes()[: s.type.byte_width]


def c_if_else(amd, t, cond, left, right, with_validity=True, pad=64):
    """arx_if_else on host pyarrow operands (arrays, or typed scalars): (rc, raw data bytes, raw validity bytes | None);
    both output buffers are filled with 0xEE first and carry `pad` bytes after what the call may write."""
    import torch

    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n = len(cond)
    w = width_of(t)
    words = (n + 63) // 64
    keep = []

    def operand(x):
        if isinstance(x, pa.Array):
            span, bufs = c_operand(x)
            keep.extend([span, bufs])
            return C.byref(span), None
        raw = c_scalar_bytes(x)
        if raw is None:
            return None, None
        holder = C.create_string_buffer(raw, len(raw))
        keep.append(holder)
        return None, C.cast(holder, C.c_void_p)

    cspan, cbufs = c_operand(cond)
    (lspan, lsc), (rspan, rsc) = operand(left), operand(right)
    out_bytes, valid_bytes = (words * 8 if w == 0 else n * w) + pad, words * 8 + pad
    out = to_device(np.full(out_bytes, 0xEE, np.uint8))
    valid = to_device(np.full(valid_bytes, 0xEE, np.uint8)) if with_validity else None
    rc = lib.arx_if_else(w, C.byref(cspan), lspan, lsc, rspan, rsc, n, out.data_ptr(), valid.data_ptr() if with_validity else None, None)
    if out.is_cuda:
        torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:out_bytes], (valid.cpu().numpy()[:valid_bytes] if with_validity else None)


def can_be_null(*operands):
    return any((x.null_count != 0 and x.buffers()[0] is not None) if isinstance(x, pa.Array) else not x.is_valid for x in operands)


def check_c(amd, t, cond, left, right, what):
    """The raw outputs of arx_if_else equal the reference, null slots are zero, and nothing else is written."""
    from arrow_amd import _lib

    lib = _lib.get_lib()
    n, w = len(cond), width_of(t)
    words = (n + 63) // 64
    want = pc.if_else(cond, left, right)
    nullable = can_be_null(cond, left, right)
    rc, data, valid = c_if_else(amd, t, cond, left, right)
    assert rc == 0, (what, lib.arx_last_error())
    nbytes = words * 8 if w == 0 else n * w
    assert (data[nbytes:] == 0xEE).all(), what                        # nothing past length * width (bool: the last word)
    assert (valid[words * 8:] == 0xEE).all(), what                    # nothing past the last validity word
    vbits = np.unpackbits(valid[: words * 8], bitorder="little")
    assert not vbits[n:].any(), what                                   # pad bits beyond length: zero
    got = pa.Array.from_buffers(want.type, n, [pa.py_buffer(valid[: words * 8].tobytes()), pa.py_buffer(data[:nbytes].tobytes())])
    assert got.equals(want) and got.null_count == want.null_count, what
    is_null = ~vbits[:n].astype(bool)
    if w == 0:
        dbits = np.unpackbits(data[:nbytes], bitorder="little")
        assert not dbits[n:].any() and not dbits[:n][is_null].any(), what
    else:
        assert not data[:nbytes].reshape(n, w)[is_null].any(), what    # null slots: zero
    # out_validity = NULL is accepted exactly when nothing can be null, and then leaves no trace
    rc, data2, _ = c_if_else(amd, t, cond, left, right, with_validity=False)
    if nullable:
        assert rc == _lib.ARX_INVALID and b"NULL out_validity" in lib.arx_last_error(), what
        assert (data2 == 0xEE).all(), what
    else:
        assert rc == 0 and (data2 == data).all() and vbits[:n].all(), what


def decimal_column(rng, t, n, null_p):
    """decimal128 rows with random 128-bit patterns (if_else moves bits; it validates no precision)."""
    valid = rng.random(n) >= null_p
    raw = rng.integers(0, 256, n * 16, dtype=np.uint8)
    return pa.Array.from_buffers(t, n, [pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if null_p else None,
                                        pa.py_buffer(raw.tobytes())])


def _c_abi(amd):
    dec = pa.decimal128(38, 4)
    raw_types = {16: dec, 1: pa.uint8(), 2: pa.uint16(), 4: pa.uint32(), 8: pa.uint64(), 0: pa.bool_()}
    for w, t in raw_types.items():
        make = decimal_column if w == 16 else column
        scalar = pa.scalar(True, t) if w == 0 else (pa.scalar(__import__("decimal").Decimal("-1234567890123456789012.3456"), t)
                                                    if w == 16 else pa.scalar(201, t))
        for n in (1, 64, 65, 257, 1001, 1025):
            rng = rng_for("c abi", w, n)
            cut = lambda a, which: a.slice(OFFSETS[which], n)  # noqa: E731
            cond = cut(column(rng, pa.bool_(), n + 80, 0.1), "cond")
            left, right = cut(make(rng, t, n + 80, 0.1), "left"), cut(make(rng, t, n + 80, 0.1), "right")
            check_c(amd, t, cond, left, right, (w, n, "array / array"))
            if n in (65, 1001):
                check_c(amd, t, cond, left, scalar, (w, n, "array / scalar"))
                check_c(amd, t, cond, scalar, right, (w, n, "scalar / array"))
                check_c(amd, t, cond, pa.scalar(None, t), right, (w, n, "null / array"))
                check_c(amd, t, cond, scalar, pa.scalar(None, t), (w, n, "scalar / null"))
                check_c(amd, t, cond, pa.scalar(None, t), pa.scalar(None, t), (w, n, "null / null"))
                # nothing can be null
                c0 = cut(column(rng, pa.bool_(), n + 80, 0.0), "cond")
                l0, r0 = cut(make(rng, t, n + 80, 0.0), "left"), cut(make(rng, t, n + 80, 0.0), "right")
                check_c(amd, t, c0, l0, r0, (w, n, "no nulls"))
                check_c(amd, t, c0, scalar, r0, (w, n, "no nulls, scalar / array"))
                check_c(amd, t, c0, scalar, scalar, (w, n, "no nulls, scalar / scalar"))


def _invalid_arguments(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n = 100
    rng = rng_for("invalid")
    spans = {}
    keep = []
    for which, t, null_p in (("cond", pa.bool_(), 0.1), ("left", pa.int32(), 0.0), ("right", pa.int32(), 0.0), ("plain", pa.bool_(), 0.0)):
        spans[which], bufs = c_operand(column(rng, t, n, null_p))
        keep.append(bufs)
    out = to_device(np.full(n * 4 + 64, 0xEE, np.uint8))
    valid = to_device(np.full(16 + 64, 0xEE, np.uint8))
    seven = C.c_int32(7)

    def call(width=4, cond="cond", left="left", right="right", lsc=None, length=n, o=out, v=valid):
        ref = lambda k: C.byref(spans[k]) if k is not None else None  # noqa: E731
        return lib.arx_if_else(width, ref(cond), ref(left), lsc, ref(right), None, length, o.data_ptr() if o is not None else None,
                               v.data_ptr() if v is not None else None, None)

    spans["short"] = _lib.ArxSpan(None, keep[1][1].data_ptr(), 0, n - 1, 0)
    spans["half"] = _lib.ArxSpan(spans["cond"].validity, spans["cond"].data, 0, n // 2, -1)
    for kwargs, text in (({"width": 3}, b"byte_width 3"), ({"width": 32}, b"byte_width 32"), ({"width": -1}, b"byte_width -1"),
                         ({"length": -1}, b"negative length"), ({"left": "short"}, b"of left is not length"),
                         ({"right": "short"}, b"of right is not length"), ({"length": n - 1}, b"of cond is not length"),
                         ({"cond": None}, b"NULL cond"), ({"o": None}, b"NULL out_data"),
                         ({"v": None}, b"NULL out_validity"),                                  # cond has a bitmap
                         ({"cond": "plain", "left": None, "v": None}, b"NULL out_validity"),   # left is a null scalar
                         ({"lsc": C.byref(seven)}, b"left is given as an array and as a scalar")):
        assert call(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    untouched = lambda: (out.cpu().numpy()[: n * 4 + 64] == 0xEE).all() and (valid.cpu().numpy()[: 16 + 64] == 0xEE).all()  # noqa: E731
    assert untouched()
    # length 0 succeeds, launches nothing and writes nothing
    count = lambda: tuple(lib.arx_get_counter(name) for name in (b"if_else_launches", b"if_else_packed_launches", b"if_else_bool_launches"))  # noqa: E731
    before = count()
    for name in ("cond", "left", "right"):
        spans[name + "0"] = _lib.ArxSpan(spans[name].validity, spans[name].data, 0, 0, 0)
    for width in (0, 1, 4, 16):
        assert call(width=width, cond="cond0", left="left0", right="right0", length=0) == 0
        assert call(width=width, cond="cond0", left="left0", right="right0", length=0, o=None, v=None) == 0
    assert count() == before
    assert untouched()
    # one launch of the kernel of its kind per call: widths 8 and 16, widths 1 / 2 / 4, booleans
    assert call() == 0 and count() == (before[0], before[1] + 1, before[2])
    valid[:16] = 0xEE
    assert call(cond="plain", v=None) == 0 and count() == (before[0], before[1] + 2, before[2])    # nothing can be null: no bitmap asked for
    assert (valid.cpu().numpy()[: 16 + 64] == 0xEE).all()
    spans["wide"], b8 = c_operand(column(rng, pa.int64(), n // 2, 0.0))
    assert call(width=8, left="wide", right="wide", length=n // 2, cond="half") == 0 and count() == (before[0] + 1, before[1] + 2, before[2])
    spans["bl"], b1 = c_operand(column(rng, pa.bool_(), n, 0.0))
    assert call(width=0, left="bl", right="plain") == 0 and count() == (before[0] + 1, before[1] + 2, before[2] + 1)


def _mirror(amd):
    from arrow_amd.array import bool_, int32, type_from_name

    rng = rng_for("mirror")
    n = 500
    cond, left, right = column(rng, pa.bool_(), n, 0.1), column(rng, pa.int32(), n, 0.1), column(rng, pa.int32(), n, 0.0)
    dc, dl, dr = (amd.Array.from_pyarrow(a) for a in (cond, left, right))
    want = pc.if_else(cond, left, right)
    direct = amd.compute.if_else(dc, dl, dr)
    routed = amd.compute.call_function("if_else", [dc, dl, dr])
    assert direct.to_pyarrow().equals(want) and routed.to_pyarrow().equals(want)
    assert "if_else" in amd.compute.get_function_registry().get_function_names()
    # Python scalars take the other side's type; None is a null scalar; arrow_amd.Scalar
    assert amd.compute.if_else(dc, dl, 0).to_pyarrow().equals(pc.if_else(cond, left, pa.scalar(0, pa.int32())))
    assert amd.compute.if_else(dc, -5, dr).to_pyarrow().equals(pc.if_else(cond, pa.scalar(-5, pa.int32()), right))
    assert amd.compute.if_else(dc, dl, None).to_pyarrow().equals(pc.if_else(cond, left, pa.scalar(None, pa.int32())))
    assert amd.compute.if_else(dc, None, dr).to_pyarrow().equals(pc.if_else(cond, pa.scalar(None, pa.int32()), right))
    assert amd.compute.if_else(dc, amd.Scalar(9, int32), 3).to_pyarrow().equals(pc.if_else(cond, pa.scalar(9, pa.int32()), pa.scalar(3, pa.int32())))
    assert amd.compute.if_else(dc, None, amd.Scalar(4, int32)).to_pyarrow().equals(pc.if_else(cond, pa.scalar(None, pa.int32()), pa.scalar(4, pa.int32())))
    flags, dflags = column(rng, pa.bool_(), n, 0.1), None
    dflags = amd.Array.from_pyarrow(flags)
    assert amd.compute.if_else(dc, dflags, True).to_pyarrow().equals(pc.if_else(cond, flags, pa.scalar(True)))
    f64 = column(rng, pa.float64(), n, 0.0)
    assert amd.compute.if_else(dc, 1.5, amd.Array.from_pyarrow(f64)).to_pyarrow().equals(pc.if_else(cond, pa.scalar(1.5), f64))
    # ---- refusals
    with pytest.raises(amd.ArrowNotImplementedError, match="left is int32, right is double"):
        amd.compute.if_else(dc, dl, amd.Array.from_pyarrow(f64))
    with pytest.raises(amd.ArrowNotImplementedError, match="left is int32, right is int64"):
        amd.compute.if_else(dc, dl, amd.Scalar(1, type_from_name("int64")))
    with pytest.raises(amd.ArrowNotImplementedError, match="cond must be a boolean arrow_amd.Array, not int32"):
        amd.compute.if_else(dl, dl, dr)
    with pytest.raises(amd.ArrowNotImplementedError, match="cond must be a boolean arrow_amd.Array, not bool"):
        amd.compute.if_else(amd.Scalar(True, bool_), dl, dr)
    for untyped in ((1, 2), (None, 2), (None, None), (True, False)):
        with pytest.raises(amd.ArrowNotImplementedError, match="carries a type"):
            amd.compute.if_else(dc, *untyped)
    short_cond = amd.Array.from_pyarrow(pa.array([True, False, None] * 4))
    for typ in (pa.string(), pa.binary()):
        s = amd.Array.from_pyarrow(pa.array(["a", None, "c"] * 4, pa.string()).cast(typ))
        for args in ((s, s), (s, None), (None, s)):
            with pytest.raises(amd.ArrowNotImplementedError, match="has no kernel matching input types") as err:
                amd.compute.if_else(short_cond, *args)
            assert str(err.value) == f"Function 'if_else' has no kernel matching input types (bool, {typ}, {typ})"
    with pytest.raises(amd.ArrowInvalid, match="same length"):
        amd.compute.if_else(short_cond, dl, dr)
    # ---- no validity buffer when nothing can be null; null counts known or lazy
    plain = amd.Array.from_pyarrow(column(rng, pa.bool_(), n, 0.0))
    no_nulls = amd.compute.if_else(plain, dr, 7)
    assert no_nulls.validity is None and no_nulls.null_count == 0
    # a slice does not know its null count: the result's is counted on first use, and right
    sl = amd.compute.if_else(dc.slice(3), dl.slice(3), dr.slice(3))
    assert callable(sl._null_count)
    want_sl = pc.if_else(cond.slice(3), left.slice(3), right.slice(3))
    assert sl.null_count == want_sl.null_count and not callable(sl._null_count)
    assert sl.to_pyarrow().equals(want_sl)


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_if_else_grid(emu_ctx, n):
    _grid(emu_ctx, n)


@pytest.mark.emu
def test_if_else_operand_forms(emu_ctx):
    _operand_forms(emu_ctx)


@pytest.mark.emu
def test_if_else_cond_patterns(emu_ctx):
    _cond_patterns(emu_ctx)


@pytest.mark.emu
def test_if_else_null_cond_bits_and_garbage_under_nulls(emu_ctx):
    _null_slots(emu_ctx)


@pytest.mark.emu
def test_if_else_c_abi_widths_and_written_bytes(emu_ctx):
    _c_abi(emu_ctx)


@pytest.mark.emu
def test_if_else_c_abi_invalid_arguments_length_zero_and_counters(emu_ctx):
    _invalid_arguments(emu_ctx)


@pytest.mark.emu
def test_if_else_mirror(emu_ctx):
    _mirror(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
def test_gpu_if_else_grid(gpu_ctx):
    for n in LENGTHS:
        _grid(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_if_else_forms_and_patterns(gpu_ctx):
    _operand_forms(gpu_ctx)
    _cond_patterns(gpu_ctx)
    _null_slots(gpu_ctx)


@pytest.mark.gpu
def test_gpu_if_else_c_abi(gpu_ctx):
    _c_abi(gpu_ctx)
    _invalid_arguments(gpu_ctx)


@pytest.mark.gpu
def test_gpu_if_else_mirror(gpu_ctx):
    _mirror(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["int8", "int64", "bool"])
def test_gpu_if_else_1e6_rows_from_numpy_buffers(gpu_ctx, name):
    rng = rng_for("1e6", name)
    n = 1_000_000
    t = TYPES[name]

    def from_buffers(typ, which):
        total = n + OFFSETS[which]
        valid = np.packbits(rng.random(total) >= 0.05, bitorder="little")
        if pa.types.is_boolean(typ):
            data = np.packbits(rng.random(total) < 0.5, bitorder="little")
        else:
            dt = np.dtype(typ.to_pandas_dtype())
            data = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, total, dtype=dt, endpoint=True)
        return pa.Array.from_buffers(typ, total, [pa.py_buffer(valid.tobytes()), pa.py_buffer(data.tobytes())]).slice(OFFSETS[which])

    cond, left, right = from_buffers(pa.bool_(), "cond"), from_buffers(t, "left"), from_buffers(t, "right")
    check(gpu_ctx, cond, left, right, ("1e6", name))
    check(gpu_ctx, cond, left, pa.scalar(True, t) if name == "bool" else pa.scalar(3, t), ("1e6 array / scalar", name))
