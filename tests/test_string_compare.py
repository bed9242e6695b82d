"""equal / not_equal / greater / greater_equal / less / less_equal of utf8 / binary columns (arrow_amd.compute,
csrc/string_compare.hip) against pyarrow.compute on the host copies of the same operands: values, validity, null_count
and offset 0, exact equality.  Every case runs all six functions on both forms of the kernel (compute.STRING_COMPARE_PATH:
1 = one lane per row pair, 2 = one wave per row pair).

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus one column pair of 10^6 rows built from numpy buffers.  Large offsets, the guard words, the refusals and the
launch counters go through the C ABI, since the mirror's Array carries no large offsets."""
import ctypes as C
import operator

import numpy as np
import pytest

from . import string_util
from .string_util import c_buffers, path_set, sync

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

LENGTHS = [0, 1, 63, 64, 65, 4097]
OPS = ["equal", "not_equal", "greater", "greater_equal", "less", "less_equal"]      # ARX_CMP_* in this order
PY_OPS = [operator.eq, operator.ne, operator.gt, operator.ge, operator.lt, operator.le]
AUTO, ROWS, WAVES = 0, 1, 2
ROW_COUNTER, WAVE_COUNTER = b"string_compare_row_launches", b"string_compare_wave_launches"
PREFIXES = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]   # 1024 = one step of the wave form
ALIGNMENTS = [0, 1, 7, 8, 15]
LITERAL_SIZES = [0, 1, 16, 1024, 1025, 5000]                                        # 1024 = the LDS cap of a literal
SEED = 0xC09A
KNOB = "STRING_COMPARE_PATH"              # the global of arrow_amd.compute that selects the kernel form


def rng_for(*key):
    return string_util.rng_for(SEED, *key)


def pattern(k, salt=0):
    """k bytes below 0x80 without a period that divides 8 or 16."""
    return bytes((i * 7 + i // 13 + salt) % 0x7F + 1 for i in range(k))


def row_pool():
    rows = ["", "a", "ab", "abc", "b", "a\x00", "\x00", "é", "ée", "日本", "日本語", "\x7f", "z" * 7, "z" * 8, "z" * 9]
    rows += [pattern(k).decode() for k in (15, 16, 17, 31, 32, 33, 100)]
    rows += [pattern(32).decode() + t for t in ("a", "b", "\x00", "é")] + [pattern(100).decode()[:-1] + "~"]
    return rows


def column(rng, n, null_p, typ, pool=None):
    pool = pool or row_pool()
    mask = (rng.random(n) < null_p) if null_p else None
    return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask).cast(typ)


def as_scalar(x, typ):
    return pa.scalar(x if pa.types.is_string(typ) or x is None else x.encode() if isinstance(x, str) else x, typ)


def same(got, want, hosts, what):
    """The device result equals the reference's: rows, null count, offset 0, and no bitmap when no operand can be null."""
    assert got.to_pyarrow().equals(want), what
    assert got.null_count == want.null_count, what
    assert got.offset == 0, what
    if all(isinstance(h, pa.Array) and h.buffers()[0] is None or isinstance(h, pa.Scalar) and h.is_valid for h in hosts):
        assert got.validity is None, what


def check(amd, left, right, dleft, dright, what, paths=(ROWS, WAVES)):
    """All six functions on both forms; left / right: a pyarrow array or scalar, dleft / dright their device twins (a
    scalar goes as the str / bytes / None it holds)."""
    for name in OPS:
        want = getattr(pc, name)(left, right)
        for path in paths:
            with path_set(amd, KNOB, path):
                got = getattr(amd.compute, name)(dleft, dright)
            same(got, want, (left, right), (name, path, what))


def check_literal(amd, host, dev, literal, what):
    """array x literal and literal x array"""
    sc = as_scalar(literal, host.type)
    value = sc.as_py()
    check(amd, host, sc, dev, value, (what, "array x literal"))
    check(amd, sc, host, value, dev, (what, "literal x array"))


def _grid(amd, n, types=(pa.string(), pa.binary())):
    """Both types, both null shares; the left side is slice(13) of n + 13 rows, the right side the first n rows and
    slice(5) of n + 5, so the two validity bit offsets differ; array x array, array x literal, literal x array."""
    for typ in types:
        for null_p in (0.0, 0.1):
            rng = rng_for("grid", n, typ, null_p)
            left, right = column(rng, n + 13, null_p, typ), column(rng, n + 5, null_p, typ)
            dleft, dright = amd.Array.from_pyarrow(left), amd.Array.from_pyarrow(right)
            check(amd, left.slice(13), right.slice(0, n), dleft.slice(13), dright.slice(0, n), (n, typ, null_p, 0))
            check(amd, left.slice(13), right.slice(5), dleft.slice(13), dright.slice(5), (n, typ, null_p, 5))
            check_literal(amd, left.slice(13), dleft.slice(13), pattern(32).decode(), (n, typ, null_p))


def edge_pairs(x, y):
    """(left row, right row) for every prefix length p: differing at byte p (x on the left, y on the right, and what
    follows would answer the other way), one row ending at p on either side, and equal rows."""
    out = []
    for p in PREFIXES:
        head = pattern(p, p)
        out += [(head + bytes([x]) + b"\xff\xff\xff", head + bytes([y]) + b"\x00"),
                (head, head + bytes([y]) + b"tail"), (head + bytes([x]), head), (head + bytes([x]), head + bytes([x]))]
    return out


def aligned_column(rows, alignments):
    """A binary column in which row 2 i + 1 is rows[i] and starts at alignments[i] modulo 16 in the data buffer, set by
    the filler row 2 i in front of it."""
    out, at = [], 0
    for row, want in zip(rows, alignments):
        filler = b"#" * ((want - at) % 16)
        out += [filler, row]
        at += len(filler) + len(row)
    return pa.array(out, pa.binary())


def _edges(amd, x, y):
    pairs = edge_pairs(x, y)
    combos = [(a, b) for a in ALIGNMENTS for b in ALIGNMENTS]
    lrows = [l for l, r in pairs for _ in combos]
    rrows = [r for l, r in pairs for _ in combos]
    left = aligned_column(lrows, [a for _ in pairs for a, b in combos])
    right = aligned_column(rrows, [b for _ in pairs for a, b in combos])
    dleft, dright = amd.Array.from_pyarrow(left), amd.Array.from_pyarrow(right)
    for host, dev, want in ((left, dleft, [a for _ in pairs for a, b in combos]), (right, dright, [b for _ in pairs for a, b in combos])):
        assert dev.buffers[2].data_ptr() % 16 == 0                   # the fillers set the alignment of the ADDRESSES
        starts = np.frombuffer(host.buffers()[1], np.int32)[1: 2 * len(want): 2]
        assert (starts % 16 == np.array(want)).all()
    check(amd, left, right, dleft, dright, ("edges", x, y))


def _specials(amd):
    for typ in (pa.string(), pa.binary()):
        left = pa.array(["", "", "\x00", "a\x00b", "a\x00b", "a\x00", "a", "ab\x00", None, "x"], pa.string()).cast(typ)
        right = pa.array(["", "\x00", "", "a\x00c", "a\x00b", "a", "a\x00", "ab", "x", None], pa.string()).cast(typ)
        check(amd, left, right, amd.Array.from_pyarrow(left), amd.Array.from_pyarrow(right), ("specials", typ))
        for lit in ("", "\x00", "a\x00b", "a"):
            check_literal(amd, left, amd.Array.from_pyarrow(left), lit, ("specials", typ, lit))
        # all-null and all-empty columns
        for arr in (pa.array([None] * 70, typ), pa.array([""] * 70, pa.string()).cast(typ)):
            other = column(rng_for("specials", typ), 70, 0.1, typ)
            check(amd, arr, other, amd.Array.from_pyarrow(arr), amd.Array.from_pyarrow(other), ("all", typ))
            check_literal(amd, arr, amd.Array.from_pyarrow(arr), "", ("all", typ))
    # slices whose neighbours outside would change the answer
    a, b = pa.array(["zz", "m", "m", "aa"]), pa.array(["aa", "m", "n", "zz"])
    da, db = amd.Array.from_pyarrow(a), amd.Array.from_pyarrow(b)
    check(amd, a.slice(1, 2), b.slice(1, 2), da.slice(1, 2), db.slice(1, 2), "neighbours")
    check(amd, a.slice(1, 2), b.slice(2, 2), da.slice(1, 2), db.slice(2, 2), "neighbours, offsets apart")


def _null_row_spanning_bytes(amd):
    """A null row whose offsets span bytes that would answer true: its bit is 0 in the values too, on either side."""
    plain = pa.array(["aaa", "zzz", "mmm", "b"], pa.string())
    holed = pa.Array.from_buffers(pa.string(), 4, [pa.py_buffer(bytes([0b1101])), plain.buffers()[1], plain.buffers()[2]])
    other = pa.array(["aaa", "zzz", "mmx", "a"], pa.string())
    assert holed.to_pylist()[1] is None
    for left, right in ((holed, other), (other, holed)):
        check(amd, left, right, amd.Array.from_pyarrow(left), amd.Array.from_pyarrow(right), "null row")
        for path in (ROWS, WAVES):
            for code, op in enumerate(PY_OPS):
                bits = c_compare(amd, code, left, right, 4, None, path)
                want = [bool(l is not None and r is not None and op(l, r)) for l, r in zip(left.to_pylist(), right.to_pylist())]
                assert bits.tolist() == want and not bits[1], (code, path)
    check_literal(amd, holed, amd.Array.from_pyarrow(holed), "zzz", "null row")


def _literals(amd):
    """Literals around the LDS cap against rows that are the literal, its prefixes and its neighbours; 5000 bytes is longer
    than every row."""
    for size in LITERAL_SIZES:
        lit = pattern(size, size)
        rows = [b"", b"\x01", lit[:7], lit[:size // 2], pattern(40, 3)]
        if size:
            rows += [lit[:-1]]
        if size > 1:                                                                 # one byte up and down, a row one byte shorter
            rows += [lit[:-2] + bytes([lit[-2] + 1]), lit[:-2] + bytes([lit[-2] - 1])]
        if size < 5000:
            rows += [lit, lit + b"\x00", lit + b"a", b"#" * 3 + lit]
        if 0 < size < 5000:                                                          # the same in the literal's last byte
            rows += [lit[:-1] + bytes([lit[-1] + 1]), lit[:-1] + bytes([lit[-1] - 1])]
        rng = rng_for("literals", size)
        arr = pa.array([rows[i] for i in rng.integers(0, len(rows), 150)], pa.binary(), mask=rng.random(150) < 0.1)
        assert max(len(r) for r in rows) < 5000
        check_literal(amd, arr.slice(3), amd.Array.from_pyarrow(arr).slice(3), lit, ("literal", size))
    s = pa.array(["héllo", None, "wörld", "héllo wörld"] * 20, pa.string())
    check_literal(amd, s, amd.Array.from_pyarrow(s), "héllo w", "utf8 literal")


def _null_scalar_and_mirror(amd):
    from arrow_amd import _lib

    lib = _lib.get_lib()
    cp = amd.compute
    for typ in (pa.string(), pa.binary()):
        arr = column(rng_for("mirror", typ), 100, 0.1, typ)
        dev = amd.Array.from_pyarrow(arr)
        before = lib.arx_get_counter(ROW_COUNTER), lib.arx_get_counter(WAVE_COUNTER)
        check_literal(amd, arr, dev, None, ("null scalar", typ))                     # all null ...
        assert (lib.arx_get_counter(ROW_COUNTER), lib.arx_get_counter(WAVE_COUNTER)) == before      # ... without a launch
        got = cp.equal(dev, None)
        assert got.null_count == 100 and got.to_pyarrow().to_pylist() == [None] * 100
    s = pa.array(["a", None, "b", "ab"], pa.string())
    ds = amd.Array.from_pyarrow(s)
    b = s.cast(pa.binary())
    db = amd.Array.from_pyarrow(b)
    # the forms of the other operand: str, bytes, Scalar, through call_function too
    assert cp.less(ds, "ab").to_pyarrow().equals(pc.less(s, "ab"))
    assert cp.less(db, b"ab").to_pyarrow().equals(pc.less(b, b"ab"))
    assert cp.less(db, "ab").to_pyarrow().equals(pc.less(b, b"ab"))                  # a str is UTF-8 encoded
    assert cp.greater("ab", ds).to_pyarrow().equals(pc.greater(pa.scalar("ab"), s))
    assert cp.call_function("not_equal", [ds, amd.Scalar("b", ds.type, True)]).to_pyarrow().equals(pc.not_equal(s, "b"))
    assert cp.equal(ds, amd.Scalar(None, ds.type, False)).null_count == 4
    sliced = cp.equal(ds.slice(1), ds.slice(1))                                      # the null count of a slice is not known: counted
    assert sliced.null_count == 1 and sliced.to_pyarrow().to_pylist() == [None, True, True]
    # refusals as the numeric kernels make them
    for name in OPS:
        with pytest.raises(amd.ArrowNotImplementedError, match=f"Function '{name}' has no kernel matching input types \\(string, binary\\)"):
            getattr(cp, name)(ds, db)
        with pytest.raises(amd.ArrowNotImplementedError, match="has no kernel matching input types"):
            cp.call_function(name, [ds, amd.Scalar(b"a", db.type, True)])
        with pytest.raises(amd.ArrowInvalid, match="Array arguments must all be the same length"):
            getattr(cp, name)(ds, ds.slice(1))
    with pytest.raises(amd.ArrowNotImplementedError, match="equal of two scalars"):
        cp.call_function("equal", [amd.Scalar("a", ds.type, True), amd.Scalar("a", ds.type, True)])
    # a numeric comparison is what it was
    ints = pa.array([1, 2, None, 4])
    assert cp.less(amd.Array.from_pyarrow(ints), 2).to_pyarrow().equals(pc.less(ints, 2))


# ---------------------------------------------------------------- the C ABI directly
def c_compare(amd, op, left, right, owidth, literal, path, hint=None):
    """arx_compare_binary on pyarrow arrays (None: the literal's side): the answers as a bool array; the 0xEE guard words
    after out_bits survive and the bits past the length are 0."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    spans, keep, nbytes = [], [], 0
    for arr in (left, right):
        if arr is None:
            spans.append(None)
            continue
        span, alive, size = c_buffers(arr, owidth)
        spans.append(span)
        keep.append(alive)
        nbytes += size
    n = len(left if left is not None else right)
    dlit = to_device(np.frombuffer(literal, np.uint8).copy()) if literal else None
    words = (n + 63) // 64
    out = to_device(np.full(words * 8 + 16, 0xEE, np.uint8))
    rc = lib.arx_compare_binary(op, *[None if s is None else C.byref(s) for s in spans], owidth, None if dlit is None else dlit.data_ptr(),
                                len(literal) if literal is not None else 0, nbytes if hint is None else hint, path, out.data_ptr(), None)
    assert rc == 0, lib.arx_last_error()
    sync(out)
    raw = out.cpu().numpy()
    assert (raw[words * 8: words * 8 + 16] == 0xEE).all()
    bits = np.unpackbits(raw[: words * 8], bitorder="little").astype(bool)
    assert not bits[n:].any()
    return bits[:n]


def _large_offsets(amd):
    """offset_width 8 equals offset_width 4 and Python's comparison of the bytes."""
    rng = rng_for("large")
    left, right = column(rng, 1000, 0.1, pa.binary()), column(rng, 1004, 0.1, pa.binary())
    l4, r4 = left.slice(5), right.slice(9, 995)
    l8, r8 = left.cast(pa.large_binary()).slice(5), right.cast(pa.large_binary()).slice(9, 995)
    lit = pattern(32)
    lrows, rrows = l4.to_pylist(), r4.to_pylist()
    for code, op in enumerate(PY_OPS):
        for path in (ROWS, WAVES):
            for a4, b4, a8, b8, literal, pairs in ((l4, r4, l8, r8, None, zip(lrows, rrows)), (l4, None, l8, None, lit, ((l, lit) for l in lrows)),
                                                   (None, r4, None, r8, lit, ((lit, r) for r in rrows))):
                want = [bool(a is not None and b is not None and op(a, b)) for a, b in pairs]
                assert c_compare(amd, code, a8, b8, 8, literal, path).tolist() == want, (code, path)
                assert c_compare(amd, code, a4, b4, 4, literal, path).tolist() == want, (code, path)


def _c_abi_contract(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    arr = pa.array(["héllo", "b", "ab"], pa.string())
    span, keep, nbytes = c_buffers(arr, 4)
    span2, keep2, _ = c_buffers(arr.slice(1), 4)
    out = to_device(np.full(64, 0xEE, np.uint8))
    lit = to_device(np.frombuffer(b"ab", np.uint8).copy())
    counters = lambda: (lib.arx_get_counter(ROW_COUNTER), lib.arx_get_counter(WAVE_COUNTER))  # noqa: E731

    def call(op=0, left=span, right=None, width=4, literal=lit.data_ptr(), m=2, hint=nbytes, path=ROWS, o=out):
        return lib.arx_compare_binary(op, C.byref(left) if left is not None else None, C.byref(right) if right is not None else None, width,
                                      literal, m, hint, path, o.data_ptr() if o is not None else None, None)

    neg = _lib.ArxBinarySpan(None, keep[1].data_ptr(), keep[2].data_ptr(), 0, -1, 0)
    no_offsets = _lib.ArxBinarySpan(None, None, keep[2].data_ptr(), 0, 3, 0)
    cases = [({"left": None}, b"both sides are NULL"), ({"op": -1}, b"op -1"), ({"op": 6}, b"op 6"), ({"path": -1}, b"path -1"),
             ({"path": 3}, b"path 3"), ({"width": 2}, b"offset_width 2"), ({"width": 16}, b"offset_width 16"),
             ({"right": span2}, b"unequal lengths 3 and 2"), ({"left": neg}, b"negative length"), ({"left": None, "right": neg}, b"negative length"),
             ({"literal": None}, b"NULL literal"), ({"m": -1}, b"negative literal_length"), ({"o": None}, b"NULL out_bits or NULL offsets"),
             ({"left": no_offsets}, b"NULL out_bits or NULL offsets"), ({"left": None, "right": no_offsets}, b"NULL out_bits or NULL offsets"),
             ({"right": no_offsets}, b"NULL out_bits or NULL offsets")]
    before = counters()
    for kwargs, text in cases:
        assert call(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    # length 0 succeeds and launches nothing, with NULL offsets and out_bits too
    empty = _lib.ArxBinarySpan(None, None, None, 0, 0, 0)
    assert call(left=empty) == 0 and call(left=empty, right=empty) == 0 and call(left=None, right=empty, o=None) == 0
    sync(out)
    assert (out.cpu().numpy()[:64] == 0xEE).all()                        # a refused call writes nothing
    assert counters() == before
    # one launch of the form asked for a call with length > 0; auto: rows without a hint and below the threshold
    for i, (kwargs, want, rows, waves) in enumerate([({}, [0, 0, 1], 1, 0), ({"path": WAVES, "op": 4}, [0, 0, 0], 1, 1),
                                                    ({"path": AUTO, "hint": -1, "op": 2}, [1, 1, 0], 2, 1),
                                                    ({"path": AUTO, "op": 3, "left": None, "right": span}, [0, 0, 1], 3, 1),
                                                    ({"path": AUTO, "hint": 1 << 40, "right": span, "literal": None, "m": 0}, [1, 1, 1], 3, 2),
                                                    ({"literal": None, "m": 0, "op": 1}, [1, 1, 1], 4, 2)]):
        assert call(**kwargs) == 0, lib.arx_last_error()
        assert counters() == (before[0] + rows, before[1] + waves), kwargs
        sync(out)
        raw = out.cpu().numpy()[:64]
        assert np.unpackbits(raw[:8], bitorder="little")[:3].tolist() == want and (raw[8:] == 0xEE).all(), kwargs
        out[:8] = 0xEE


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("typ", [pa.string(), pa.binary()], ids=str)
@pytest.mark.parametrize("n", LENGTHS)
def test_string_compare_grid(emu_ctx, n, typ):
    _grid(emu_ctx, n, (typ,))


@pytest.mark.emu
@pytest.mark.parametrize("x,y", [(0x7F, 0x80), (0x00, 0x01)])
def test_string_compare_edges(emu_ctx, x, y):
    _edges(emu_ctx, x, y)


@pytest.mark.emu
def test_string_compare_specials(emu_ctx):
    _specials(emu_ctx)


@pytest.mark.emu
def test_string_compare_null_row_spanning_bytes(emu_ctx):
    _null_row_spanning_bytes(emu_ctx)


@pytest.mark.emu
def test_string_compare_literals(emu_ctx):
    _literals(emu_ctx)


@pytest.mark.emu
def test_string_compare_null_scalar_and_mirror(emu_ctx):
    _null_scalar_and_mirror(emu_ctx)


@pytest.mark.emu
def test_string_compare_c_abi_large_offsets(emu_ctx):
    _large_offsets(emu_ctx)


@pytest.mark.emu
def test_string_compare_c_abi_contract(emu_ctx):
    _c_abi_contract(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_gpu_string_compare_grid(gpu_ctx, n):
    _grid(gpu_ctx, n)


@pytest.mark.gpu
@pytest.mark.parametrize("x,y", [(0x7F, 0x80), (0x00, 0x01)])
def test_gpu_string_compare_edges(gpu_ctx, x, y):
    _edges(gpu_ctx, x, y)


@pytest.mark.gpu
def test_gpu_string_compare_specials_and_literals(gpu_ctx):
    _specials(gpu_ctx)
    _null_row_spanning_bytes(gpu_ctx)
    _literals(gpu_ctx)
    _null_scalar_and_mirror(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_compare_c_abi(gpu_ctx):
    _large_offsets(gpu_ctx)
    _c_abi_contract(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_compare_1e6_rows_from_numpy_buffers(gpu_ctx):
    """10^6 row pairs, mean row 16 bytes, 5 % nulls a side, 20 pairs of 30 000 bytes that share all but their last byte;
    the right column is the left one with rows cut short and single bytes changed."""
    rng = rng_for("1e6")
    n = 1_000_000
    lens = rng.integers(0, 33, n)                                  # mean row size 16
    long_rows = rng.choice(n, 20, replace=False)
    lens[long_rows] = 30_000
    loff = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=loff[1:])
    ldata = rng.integers(97, 101, int(loff[-1])).astype(np.uint8)  # a small alphabet: shared prefixes are common
    rlens = np.maximum(lens - rng.integers(0, 3, n) * (rng.random(n) < 0.3), 0)
    rlens[long_rows] = 30_000
    roff = np.zeros(n + 1, np.int64)
    np.cumsum(rlens, out=roff[1:])
    row_of = np.repeat(np.arange(n), rlens)
    at = np.arange(int(roff[-1])) - roff[row_of]
    rdata = ldata[loff[row_of] + at]
    change = (rng.random(n) < 0.5) & (rlens > 0)                   # one byte of half the rows, up or down
    change[long_rows] = False
    where = roff[:-1][change] + rng.integers(0, 1 << 30, int(change.sum())) % rlens[change]
    rdata[where] = (rdata[where].astype(np.int64) + rng.choice([-1, 1], len(where))).astype(np.uint8)
    last = roff[1:][long_rows] - 1                                 # the long pairs: 10 equal, 10 differing in their last byte
    rdata[last[:10]] = ldata[loff[1:][long_rows[:10]] - 1] + 1

    def make(offsets, data):
        valid = np.packbits(rng.random(n) >= 0.05, bitorder="little")
        return pa.Array.from_buffers(pa.string(), n, [pa.py_buffer(valid.tobytes()), pa.py_buffer(offsets.astype(np.int32).tobytes()),
                                                     pa.py_buffer(data.tobytes())])

    left, right = make(loff, ldata), make(roff, rdata)
    dleft, dright = gpu_ctx.Array.from_pyarrow(left), gpu_ctx.Array.from_pyarrow(right)
    check(gpu_ctx, left.slice(13), right.slice(13), dleft.slice(13), dright.slice(13), "1e6", paths=(ROWS, WAVES, AUTO))
    check_literal(gpu_ctx, left.slice(13), dleft.slice(13), "abcabcabcabcabca", "1e6")
