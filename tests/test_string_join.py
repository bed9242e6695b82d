"""binary_join_element_wise (arrow_amd.compute, csrc/string_join.hip) against pyarrow.compute on the host copies of the
same operands: values, validity, null_count, offset 0 and type, exact equality; no bitmap when no row is null.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same helpers on the
MI355X plus one column pair of 10^6 rows built from numpy buffers.  The large types, the refused arguments, int64 offsets
above 2^31 and the int32 overflow go through the C ABI.

ONE DEPARTURE from the reference, restated here and checked against this restatement, not against pyarrow: under
null_handling="skip" a row whose values are all null and whose separator is valid is the EMPTY STRING, valid.  pyarrow
25.0.0 drops such a row (its result is shorter than its inputs); test_reference_skip_still_drops_all_null_rows notices a
pyarrow that no longer does.  Wherever a skip result is compared with pyarrow, the operands are constructed so that no
such row exists, and the test asserts that on the host copy."""
import ctypes as C

import numpy as np
import pytest

from . import string_util
from .string_util import c_buffers, sync

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

ROW_COUNTS = [0, 1, 63, 64, 65, 4095, 4096, 4097]            # the ballot word and kBinRows edges
VALUE_BYTES = [0, 1, 7, 8, 9, 15, 16, 17, 63, 65]
LONG_ROW = 40_000                                             # spans several 16 KiB output chunks
LONG = "".join(chr(65 + (i * 7 + i // 26) % 26) for i in range(1025))     # 1025 bytes: past the LDS cap
MODES = [("emit_null", ""), ("replace", ""), ("replace", "NA"), ("replace", LONG), ("skip", "")]
COUNTER = b"string_join_launches"
CAP = 32                                                      # ARX_JOIN_MAX_OPERANDS, the separator included
SEED = 0x10E5
EMIT_NULL, SKIP, REPLACE = 0, 1, 2
COLUMN, LITERAL, NULL = 0, 1, 2


def rng_for(*key):
    return string_util.rng_for(SEED, *key)


# ---------------------------------------------------------------- operands
def row_bytes(rng, size, binary):
    """A row of exactly `size` bytes: any byte with '\\0' and 0xff frequent (binary), or UTF-8 with '\\0' and 2- / 3-byte
    characters padded to the size (utf8)."""
    if binary:
        raw = rng.integers(0, 256, size).astype(np.uint8)
        raw[rng.random(size) < 0.2] = 0
        raw[rng.random(size) < 0.2] = 0xFF
        return raw.tobytes()
    out, alphabet = b"", ["a", "\0", "é", "日", "z", "ß"]
    while True:
        ch = alphabet[int(rng.integers(0, len(alphabet)))].encode()
        if len(out) + len(ch) > size:
            return out + b"x" * (size - len(out))
        out += ch


def column(rng, n, typ, null_p=0.1, sizes=VALUE_BYTES, offset=0, mask=None):
    """n rows (after slicing off `offset` leading ones) with lengths from `sizes`; null_p None: no bitmap."""
    binary = pa.types.is_binary(typ) or pa.types.is_large_binary(typ)
    total = n + offset
    rows = [row_bytes(rng, int(s), binary) for s in rng.choice(sizes, total)]
    if mask is None and null_p is not None:
        mask = rng.random(total) < null_p
    if mask is not None and len(mask) < total:
        mask = np.concatenate([np.zeros(total - len(mask), bool), mask])
    arr = pa.array(rows, pa.binary(), mask=mask).cast(typ)
    return arr.slice(offset)


def as_literal(x, typ):
    binary = pa.types.is_binary(typ) or pa.types.is_large_binary(typ)
    return x.encode() if binary and isinstance(x, str) else x


def no_row_without_a_value(ops):
    """True when no row has every value null under a valid separator (literals count in every row)."""
    *values, sep = ops
    n = next(len(o) for o in ops if isinstance(o, pa.Array))
    every = np.ones(n, bool)
    for v in values:
        every &= np.asarray(pc.is_null(v)) if isinstance(v, pa.Array) else np.full(n, v is None)
    sep_valid = ~np.asarray(pc.is_null(sep)) if isinstance(sep, pa.Array) else np.full(n, sep is not None)
    return not (every & sep_valid).any()


def reference(ops, typ, mode, rep):
    """pyarrow's result on the host operands; a python None stands for a null literal of the operands' type."""
    args = [o if isinstance(o, pa.Array) else pa.scalar(o, typ) for o in ops]
    return pc.binary_join_element_wise(*args, null_handling=mode, null_replacement=as_literal(rep, typ))


def same_join(got, want, what):
    assert got.to_pyarrow().equals(want), what
    assert got.null_count == want.null_count, what
    assert got.offset == 0 and got.to_pyarrow().type == want.type, what
    assert (got.validity is None) == (want.null_count == 0), what


def check(amd, ops, typ, modes=MODES, what=None):
    """ops: host arrays and literals (str / bytes / None), the separator last.  Every mode against pyarrow; the operands
    of a skip comparison hold no row the reference would drop."""
    dev = [amd.Array.from_pyarrow(o) if isinstance(o, pa.Array) else o for o in ops]
    _check_dev(amd, ops, dev, typ, modes, what)


def _check_dev(amd, ops, dev, typ, modes, what):
    ops = [as_literal(o, typ) if isinstance(o, str) else o for o in ops]
    dev = [as_literal(o, typ) if isinstance(o, str) else o for o in dev]
    for mode, rep in modes:
        if mode == "skip":
            assert no_row_without_a_value(ops), what
        want = reference(ops, typ, mode, rep)
        got = amd.compute.binary_join_element_wise(*dev, null_handling=mode, null_replacement=as_literal(rep, typ))
        same_join(got, want, (what, str(typ), mode, rep[:8], len(want)))


def sliced_pair(amd, rng, n, typ, offset, null_p=0.1, sizes=VALUE_BYTES, mask=None):
    """(host, device) of a column of n rows that sits at `offset` inside its buffers."""
    host = column(rng, n, typ, null_p, sizes, offset, mask)
    assert host.offset == offset
    return host, amd.Array.from_pyarrow(host)          # (the device array keeps the slice offset)


def masks_with_a_value_in_every_row(rng, n, k, null_p):
    """k null masks of n rows of which no row is null in all k."""
    masks = [rng.random(n) < null_p for _ in range(k)]
    every = np.logical_and.reduce(masks)
    masks[int(rng.integers(0, k))][every] = False
    return masks


def check_pairs(amd, pairs, typ, modes=MODES, what=None):
    """pairs: (host, device) tuples and literals."""
    ops = [p[0] if isinstance(p, tuple) else p for p in pairs]
    dev = [p[1] if isinstance(p, tuple) else p for p in pairs]
    _check_dev(amd, ops, dev, typ, modes, what)


# ---------------------------------------------------------------- helpers of both tiers
def _grid(amd, n):
    """Two value columns at slice offsets 7 and 64 (the separator column at 0), with nulls and without a bitmap, a literal
    and a column separator, every mode; utf8 and binary."""
    for typ in (pa.string(), pa.binary()):
        rng = rng_for("grid", n, typ)
        m = masks_with_a_value_in_every_row(rng, n, 2, 0.1)
        a = sliced_pair(amd, rng, n, typ, 7, mask=m[0])
        b = sliced_pair(amd, rng, n, typ, 64, mask=m[1])
        plain = sliced_pair(amd, rng, n, typ, 0, null_p=None)
        sep = sliced_pair(amd, rng, n, typ, 0, null_p=0.1, sizes=[0, 1, 3])
        check_pairs(amd, [a, b, "-"], typ, what=("grid", n))
        check_pairs(amd, [a, plain, b, sep], typ, modes=MODES[:1] + MODES[2:3] + MODES[4:], what=("grid column separator", n))
        check_pairs(amd, [plain, plain, ", "], typ, modes=MODES[:1] + MODES[4:], what=("grid no bitmap", n))


def _operand_counts(amd):
    """k = 1, 2, 3, 9 and the cap's 31 values; one operand more is refused with nothing launched."""
    from arrow_amd import _lib

    lib = _lib.get_lib()
    typ, n = pa.string(), 130
    rng = rng_for("counts")
    for k in (1, 2, 3, 9, CAP - 1):
        masks = masks_with_a_value_in_every_row(rng, n, k, 0.15)
        cols = [sliced_pair(amd, rng, n, typ, (0, 7, 64)[j % 3], mask=masks[j], sizes=[0, 1, 7, 9, 17]) for j in range(k)]
        check_pairs(amd, cols + ["-"], typ, modes=[MODES[0], MODES[2], MODES[4]], what=("k", k))
    assert len(cols) + 1 == CAP
    before = lib.arx_get_counter(COUNTER)
    for mode in ("emit_null", "skip", "replace"):
        with pytest.raises(amd.ArrowNotImplementedError, match=f"binary_join_element_wise of {CAP + 1} operands.*{CAP}"):
            amd.compute.binary_join_element_wise(*[c[1] for c in cols], cols[0][1], "-", null_handling=mode)
    assert lib.arx_get_counter(COUNTER) == before
    got = amd.compute.binary_join_element_wise(*[c[1] for c in cols], "-")
    assert lib.arx_get_counter(COUNTER) == before + 2             # one launch in each of the two calls
    assert got.length == n


def _separators(amd):
    """Literal separators of 0, 1, 3, 17 and 1025 bytes, a separator column with nulls, a null literal."""
    n = 200
    for typ in (pa.string(), pa.binary()):
        rng = rng_for("separators", typ)
        masks = masks_with_a_value_in_every_row(rng, n, 3, 0.2)
        cols = [sliced_pair(amd, rng, n, typ, (7, 0, 64)[j], mask=masks[j]) for j in range(3)]
        for sep in ("", "-", "é|", "0123456789abcdefg", LONG):
            check_pairs(amd, cols + [sep], typ, modes=[MODES[0], MODES[3], MODES[4]], what=("separator", len(sep)))
        sep_col = sliced_pair(amd, rng, n, typ, 7, null_p=0.3, sizes=[0, 1, 2, 17])
        check_pairs(amd, cols + [sep_col], typ, what="separator column")
        check_pairs(amd, cols + [None], typ, what="null separator")          # every row null in every mode


def _operand_kinds(amd):
    """Columns and literals mixed, a null literal value, a literal value past the LDS cap, more literals than the LDS
    pool has room for."""
    n = 150
    for typ in (pa.string(), pa.binary()):
        rng = rng_for("kinds", typ)
        a = sliced_pair(amd, rng, n, typ, 7, null_p=0.2)
        b = sliced_pair(amd, rng, n, typ, 0, null_p=0.2)
        check_pairs(amd, ["<", a, "日本", b, ">", ", "], typ, what="literals and columns")
        check_pairs(amd, [a, None, b, "-"], typ, modes=MODES[:4], what="null literal value")       # emit_null: every row null
        check_pairs(amd, ["x", None, a, "-"], typ, what="null literal value beside a literal")
        check_pairs(amd, [a, LONG, b, LONG[::-1]], typ, modes=[MODES[0], MODES[3], MODES[4]], what="literals past the LDS cap")
        check_pairs(amd, [LONG[:1000], a, LONG[:999], LONG[:998], b, LONG[:997], LONG[:996], "+"], typ,
                    modes=[MODES[2], MODES[3], MODES[4]], what="more literals than the pool holds")
        check_pairs(amd, ["only a literal value", b], typ, what="literal value, column separator")


def _long_rows(amd):
    """One row of about 40 000 bytes among short ones, first, in the middle and last: it spans several output chunks."""
    n = 101
    for typ, place in ((pa.string(), 0), (pa.binary(), n // 2), (pa.string(), n - 1)):
        rng = rng_for("long", place)
        binary = pa.types.is_binary(typ)
        rows = [row_bytes(rng, int(s), binary) for s in rng.choice(VALUE_BYTES, n)]
        rows[place] = row_bytes(rng, LONG_ROW + 13, binary)
        a = pa.array(rows, pa.binary()).cast(typ)
        b = column(rng, n, typ, null_p=0.1)
        b = pa.array([v if i != place else rows[(place + 1) % n] for i, v in enumerate(b.to_pylist())], b.type)
        assert b[place].is_valid
        check(amd, [a, b, "--"], typ, what=("long row", place))
        check(amd, [b, a, b, "é"], typ, modes=[MODES[0], MODES[2]], what=("long row in the middle piece", place))


def _validity(amd):
    """Mostly null, all null, no bitmap; one value operand alone."""
    n = 300
    for typ in (pa.string(), pa.binary()):
        rng = rng_for("validity", typ)
        masks = masks_with_a_value_in_every_row(rng, n, 2, 0.9)
        sparse = [sliced_pair(amd, rng, n, typ, (7, 0)[j], mask=masks[j]) for j in range(2)]
        check_pairs(amd, sparse + ["-"], typ, what="p = 0.9")
        nulls = sliced_pair(amd, rng, n, typ, 7, mask=np.ones(n, bool))
        plain = sliced_pair(amd, rng, n, typ, 64, null_p=None)
        check_pairs(amd, [nulls, plain, "-"], typ, what="an all-null column")
        check_pairs(amd, [nulls, nulls, "-"], typ, modes=MODES[:4], what="all-null columns")
        check_pairs(amd, [plain, "-"], typ, what="one value, no bitmap")
        check_pairs(amd, [sparse[0], "-"], typ, modes=MODES[:4], what="one value")
        check_pairs(amd, [plain, nulls], typ, what="an all-null separator column")


def rule(values, sep, mode, rep):
    """The rows the device produces, restated (the module docstring): python values, None = null."""
    if sep is None:
        return None
    if mode == "emit_null":
        return None if any(v is None for v in values) else sep.join(values)
    if mode == "replace":
        return sep.join(rep if v is None else v for v in values)
    return sep.join(v for v in values if v is not None)       # skip; no value kept: the empty string


def _skip_rows_without_a_value(amd):
    """Rows whose values are all null under a valid separator: the empty string, valid (the restated rule); the other
    rows equal pyarrow's result on those rows alone."""
    n = 500
    for typ in (pa.string(), pa.binary()):
        rng = rng_for("skip all null", typ)
        a = sliced_pair(amd, rng, n, typ, 7, null_p=0.6)
        b = sliced_pair(amd, rng, n, typ, 0, null_p=0.6)
        sep = sliced_pair(amd, rng, n, typ, 64, null_p=0.2, sizes=[0, 1, 3])
        for ops in ([a, b, as_literal("-", typ)], [a, b, sep], [a, as_literal("-", typ)], [a, None, b, sep]):
            host = [o[0] if isinstance(o, tuple) else o for o in ops]
            dev = [o[1] if isinstance(o, tuple) else o for o in ops]
            assert not no_row_without_a_value(host)
            got = amd.compute.binary_join_element_wise(*dev, null_handling="skip")
            rows = got.to_pyarrow().to_pylist()
            lists = [o.to_pylist() if isinstance(o, pa.Array) else [o] * n for o in host]
            want = [rule([col[i] for col in lists[:-1]], lists[-1][i], "skip", None) for i in range(n)]
            assert rows == want
            empty = [i for i in range(n) if all(col[i] is None for col in lists[:-1]) and lists[-1][i] is not None]
            assert len(empty) > 20 and all(rows[i] is not None and len(rows[i]) == 0 for i in empty)
            assert got.null_count == sum(r is None for r in want) and got.offset == 0
            keep = pa.array([i for i in range(n) if i not in set(empty)], pa.int64())
            kept = [o.take(keep) if isinstance(o, pa.Array) else o for o in host]
            assert no_row_without_a_value(kept)
            assert got.to_pyarrow().take(keep).equals(reference(kept, typ, "skip", ""))
        # the restated rule is pyarrow's in the two other modes (and in skip where pyarrow is well-formed)
        lists = [a[0].to_pylist(), b[0].to_pylist()]
        for mode, rep in (("emit_null", ""), ("replace", "NA")):
            rep_lit = as_literal(rep, typ)
            want = [rule([col[i] for col in lists], as_literal("-", typ), mode, rep_lit) for i in range(n)]
            assert reference([a[0], b[0], as_literal("-", typ)], typ, mode, rep).to_pylist() == want


def _mirror(amd):
    cp = amd.compute
    s = pa.array(["héllo", None, "", "日本"], pa.string())
    t = pa.array(["x", "y", None, "z"], pa.string())
    ds, dt = amd.Array.from_pyarrow(s), amd.Array.from_pyarrow(t)
    want = pc.binary_join_element_wise(s, t, " ", null_handling="replace", null_replacement="NA")
    same_join(cp.call_function("binary_join_element_wise", [ds, dt, amd.Scalar(" ", ds.type, True)], cp.JoinOptions("replace", "NA")), want, "options")
    same_join(cp.call_function("binary_join_element_wise", [ds, dt, amd.Scalar(" ", ds.type, True)]),
              pc.binary_join_element_wise(s, t, " "), "default options")
    same_join(cp.binary_join_element_wise(ds, amd.Scalar("q", ds.type, True), dt, amd.Scalar(None, ds.type, False)),
              pc.binary_join_element_wise(s, "q", t, pa.scalar(None, pa.string())), "scalars")
    assert cp.binary_join_element_wise(ds, dt, "-").to_pyarrow().to_pylist() == ["héllo-x", None, None, "日本-z"]
    assert cp.binary_join_element_wise(ds, dt, "-", null_handling="replace", null_replacement="NA").to_pyarrow().to_pylist() == \
        ["héllo-x", "NA-y", "-NA", "日本-z"]
    assert cp.binary_join_element_wise(ds, dt, "-", null_handling="skip").to_pyarrow().to_pylist() == ["héllo-x", "y", "", "日本-z"]
    sliced = cp.binary_join_element_wise(ds.slice(1), dt.slice(1), "+")
    assert sliced.null_count == 2 and sliced.to_pyarrow().to_pylist() == [None, None, "日本+z"]
    # operands of different types, columns of different lengths: the reference's wording
    db = amd.Array.from_pyarrow(s.cast(pa.binary()))
    for host, dev in (([s, s.cast(pa.binary()), "-"], [ds, db, "-"]), ([s, b"-"], [ds, b"-"]), ([s.cast(pa.binary()), "-"], [db, "-"])):
        with pytest.raises(pa.ArrowNotImplementedError) as want_err:
            pc.binary_join_element_wise(*host)
        with pytest.raises(amd.ArrowNotImplementedError) as got_err:
            cp.binary_join_element_wise(*dev)
        assert str(got_err.value) == str(want_err.value) and "has no kernel matching input types" in str(got_err.value)
    with pytest.raises(pa.ArrowInvalid, match="Array arguments must all be the same length"):
        pc.binary_join_element_wise(s, t.slice(1), "-")
    with pytest.raises(amd.ArrowInvalid, match="Array arguments must all be the same length"):
        cp.binary_join_element_wise(ds, dt.slice(1), "-")
    with pytest.raises(ValueError, match='"keep" is not a valid null handling'):
        cp.JoinOptions("keep")
    with pytest.raises(ValueError, match='"keep" is not a valid null handling'):
        pc.JoinOptions("keep")
    with pytest.raises(TypeError, match="at least one operand must be an arrow_amd.Array"):
        cp.binary_join_element_wise("a", "b", "-")
    with pytest.raises(TypeError, match="an operand must be"):
        cp.binary_join_element_wise(ds, 3, "-")
    with pytest.raises(TypeError, match="null_replacement must be"):
        cp.binary_join_element_wise(ds, "-", null_handling="replace", null_replacement=3)
    with pytest.raises(amd.ArrowNotImplementedError, match="scalars only"):
        cp.call_function("binary_join_element_wise", [amd.Scalar("a", ds.type, True), amd.Scalar("-", ds.type, True)])


# ---------------------------------------------------------------- the C ABI directly
def device_bytes(raw):
    from arrow_amd.array import to_device

    return to_device(np.frombuffer(bytes(raw) or b"\0", np.uint8).copy())


class COperands:
    """The ArxJoinOperand table of host operands (arrays, bytes literals, None) and the device buffers behind it."""

    def __init__(self, ops, owidth):
        from arrow_amd import _lib

        self.table = (_lib.ArxJoinOperand * len(ops))()
        self.keep = []
        for slot, o in zip(self.table, ops):
            if isinstance(o, pa.Array):
                span, keep, _ = c_buffers(o, owidth)
                slot.kind, slot.column = COLUMN, span
                self.keep.append(keep)
            elif o is None:
                slot.kind = NULL
            else:
                d = device_bytes(o)
                slot.kind, slot.literal, slot.literal_length = LITERAL, d.data_ptr() if len(o) else None, len(o)
                self.keep.append(d)


def c_join(amd, ops, owidth, mode, rep=b""):
    """arx_binary_join_offsets + _data: (rows as bytes or None, offsets, null count).  The 0xEE guard words after the
    offsets, the validity words and the data survive."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    n = next(len(o) for o in ops if isinstance(o, pa.Array))
    t = COperands(ops, owidth)
    ws_bytes = lib.arx_binary_join_workspace_bytes(n, owidth)
    ws = to_device(np.zeros(ws_bytes, np.uint8))
    words = (n + 63) // 64
    out_offsets = to_device(np.full((n + 1) * owidth + 8, 0xEE, np.uint8))
    out_valid = to_device(np.full(words * 8 + 8, 0xEE, np.uint8))
    total, nulls = C.c_int64(-1), C.c_int64(-1)
    drep = device_bytes(rep)
    rc = lib.arx_binary_join_offsets(t.table, len(ops), n, owidth, mode, len(rep), ws.data_ptr(), ws_bytes, out_offsets.data_ptr(),
                                     out_valid.data_ptr(), C.byref(nulls), C.byref(total), None)
    assert rc == 0, lib.arx_last_error()
    out_data = to_device(np.full(total.value + 8, 0xEE, np.uint8))
    rc = lib.arx_binary_join_data(t.table, len(ops), n, owidth, mode, drep.data_ptr() if rep else None, len(rep), out_offsets.data_ptr(),
                                  total.value, out_data.data_ptr(), None)
    assert rc == 0, lib.arx_last_error()
    sync(out_data)
    raw_o, raw_v, raw_d = out_offsets.cpu().numpy(), out_valid.cpu().numpy(), out_data.cpu().numpy()
    for raw, used in ((raw_o, (n + 1) * owidth), (raw_v, words * 8), (raw_d, total.value)):
        assert (raw[used: used + 8] == 0xEE).all()
    offsets = raw_o[: (n + 1) * owidth].view(np.int32 if owidth == 4 else np.int64).copy()
    assert offsets[0] == 0 and offsets[-1] == total.value and (np.diff(offsets) >= 0).all()
    valid = np.unpackbits(raw_v[: words * 8], bitorder="little").astype(bool)
    assert not valid[n:].any() and nulls.value == n - int(valid[:n].sum())
    rows = [raw_d[offsets[i]: offsets[i + 1]].tobytes() if valid[i] else None for i in range(n)]
    assert all(offsets[i] == offsets[i + 1] for i in range(n) if not valid[i])                  # a null row holds no bytes
    return rows, offsets, nulls.value


def _large_types(amd):
    """large_utf8 / large_binary (offset_width 8) and the same rows with int32 offsets: the reference's rows for all."""
    n = 700
    rng = rng_for("large")
    masks = masks_with_a_value_in_every_row(rng, n, 2, 0.15)
    a = column(rng, n, pa.string(), mask=masks[0], offset=5)
    b = column(rng, n, pa.string(), mask=masks[1], offset=64)
    sep = column(rng, n, pa.string(), null_p=0.1, sizes=[0, 1, 3])
    for mode, name, rep in ((EMIT_NULL, "emit_null", ""), (SKIP, "skip", ""), (REPLACE, "replace", "NA"), (REPLACE, "replace", LONG)):
        for ops in ([a, b, "-"], [a, "é", b, sep], [a, None, b, LONG]):
            if name == "skip":
                assert no_row_without_a_value(ops)
            got = {}
            for typ, width in ((pa.string(), 4), (pa.large_string(), 8), (pa.large_binary(), 8), (pa.binary(), 4)):
                cast = [o.cast(typ) if isinstance(o, pa.Array) else o for o in ops]
                binary = pa.types.is_large_binary(typ) or pa.types.is_binary(typ)
                ref_ops = [o.encode() if binary and isinstance(o, str) else o for o in cast]
                want = reference(ref_ops, typ, name, rep)
                assert want.type == typ
                rows, offsets, nulls = c_join(amd, [o.encode() if isinstance(o, str) else o for o in cast], width, mode, rep.encode())
                assert rows == want.cast(pa.large_binary()).to_pylist() and nulls == want.null_count, (name, typ)
                assert offsets.dtype == (np.int64 if width == 8 else np.int32)
                got[typ] = offsets
            assert (got[pa.string()] == got[pa.large_string()]).all() and (got[pa.binary()] == got[pa.large_binary()]).all()


def _null_rows_spanning_bytes(amd):
    """Null rows whose offsets span bytes: they contribute nothing (skip), the replacement (replace) or a null row."""
    plain = pa.array(["xabx", "ababab", "ab", "b"], pa.string())
    a = pa.Array.from_buffers(pa.string(), 4, [pa.py_buffer(bytes([0b1101])), plain.buffers()[1], plain.buffers()[2]])
    b = pa.Array.from_buffers(pa.string(), 4, [pa.py_buffer(bytes([0b0111])), plain.buffers()[1], plain.buffers()[2]])
    assert a.to_pylist()[1] is None and b.to_pylist()[3] is None
    assert c_join(amd, [a, b, b"-"], 4, EMIT_NULL)[0] == [b"xabx-xabx", None, b"ab-ab", None]
    assert c_join(amd, [a, b, b"-"], 4, SKIP)[0] == [b"xabx-xabx", b"ababab", b"ab-ab", b"b"]
    assert c_join(amd, [a, b, b"-"], 4, REPLACE, b"NA")[0] == [b"xabx-xabx", b"NA-ababab", b"ab-ab", b"b-NA"]
    assert c_join(amd, [a, b, a], 4, REPLACE, b"NA")[0] == [b"xabxxabxxabx", None, b"ababab", b"bbNA"]
    assert c_join(amd, [a, b"-"], 4, SKIP)[0] == [b"xabx", b"", b"ab", b"b"]                   # (the departure: row 1)
    assert c_join(amd, [a], 4, EMIT_NULL)[0] == [b"", None, b"", b""]                          # the separator alone


def _c_abi_contract(amd):
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    arr = pa.array(["xabx", "ab"], pa.string())
    good = COperands([arr, arr, b"-"], 4)
    ws_bytes = lib.arx_binary_join_workspace_bytes(2, 4)
    ws = to_device(np.zeros(ws_bytes + 8, np.uint8))
    out, valid, data = (to_device(np.full(64, 0xEE, np.uint8)) for _ in range(3))
    total, nulls = C.c_int64(-1), C.c_int64(-1)
    rep = device_bytes(b"NA")

    def offsets(t=good.table, num=3, n=2, width=4, mode=EMIT_NULL, r=0, w=ws.data_ptr(), wb=ws_bytes, o=out, v=valid, nc=nulls, tb=total):
        return lib.arx_binary_join_offsets(t, num, n, width, mode, r, w, wb, o.data_ptr() if o is not None else None,
                                           v.data_ptr() if v is not None else None, C.byref(nc) if nc is not None else None,
                                           C.byref(tb) if tb is not None else None, None)

    def write(t=good.table, num=3, n=2, width=4, mode=EMIT_NULL, rp=None, r=0, o=out, tb=14, d=data):
        return lib.arx_binary_join_data(t, num, n, width, mode, rp, r, o.data_ptr() if o is not None else None, tb,
                                        d.data_ptr() if d is not None else None, None)

    def altered(**fields):
        t = COperands([arr, arr, b"-"], 4)
        t.keep.append(good)
        for name, (slot, value) in fields.items():
            obj = t.table[slot]
            if name.startswith("column_"):
                setattr(obj.column, name[len("column_"):], value)
            else:
                setattr(obj, name, value)
        return t

    short = altered(column_length=(1, 1))
    negative = altered(column_length=(0, -1))
    bad_kind = altered(kind=(2, 3))
    no_offsets = altered(column_offsets=(1, None))
    neg_literal = altered(literal_length=(2, -1))
    null_literal = altered(literal=(2, None))
    shared = [({"t": None}, b"NULL operands"), ({"width": 2}, b"offset_width 2"), ({"width": 16}, b"offset_width 16"),
              ({"n": -1}, b"negative length"), ({"num": 0}, b"at least the separator"), ({"mode": 3}, b"null_handling 3"),
              ({"mode": -1}, b"null_handling -1"), ({"r": -1}, b"negative null_replacement_length -1"),
              ({"t": short.table}, b"operand 1 is a column of 1 rows in a call of 2"), ({"t": negative.table}, b"operand 0 is a column of -1 rows"),
              ({"t": bad_kind.table}, b"kind 3 of operand 2"), ({"t": no_offsets.table}, b"NULL offsets of operand 1"),
              ({"t": neg_literal.table}, b"negative literal_length -1"), ({"t": null_literal.table}, b"NULL literal of 1 bytes")]
    before = lib.arx_get_counter(COUNTER)
    for kwargs, text in shared + [({"o": None}, b"NULL out_offsets"), ({"v": None}, b"NULL out_offsets, out_validity"),
                                  ({"nc": None}, b"out_null_count"), ({"tb": None}, b"out_total_bytes"),
                                  ({"wb": ws_bytes - 1}, b"ws of"), ({"w": None}, b"ws of"), ({"w": ws.data_ptr() + 4}, b"ws of")]:
        assert offsets(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    for kwargs, text in shared + [({"r": 2}, b"NULL null_replacement of 2 bytes"), ({"tb": -1}, b"negative total_bytes -1"),
                                  ({"o": None}, b"NULL out_offsets or out_data"), ({"d": None}, b"NULL out_offsets or out_data")]:
        assert write(**kwargs) == _lib.ARX_INVALID, kwargs
        assert text in lib.arx_last_error(), (kwargs, lib.arx_last_error())
    # more operands than the cap: ARX_NOT_IMPLEMENTED, naming the count and the cap
    many = COperands([arr] * CAP + [b"-"], 4)
    for call in (offsets, write):
        assert call(t=many.table, num=CAP + 1) == _lib.ARX_NOT_IMPLEMENTED
        assert f"{CAP + 1} operands".encode() in lib.arx_last_error() and f"takes {CAP}".encode() in lib.arx_last_error()
    sync(out)
    for buf in (out, valid, data):
        assert (buf.cpu().numpy() == 0xEE).all()
    assert total.value == -1 and nulls.value == -1 and lib.arx_get_counter(COUNTER) == before        # nothing written or launched
    # length 0: success, nothing launched, nothing written but out_offsets[0], the total and the null count
    empty = COperands([arr.slice(0, 0), arr.slice(2, 0), b"-"], 4)
    for width in (4, 8):
        total.value = nulls.value = -1
        assert offsets(t=empty.table, n=0, width=width, w=None, wb=0) == 0 and total.value == 0 and nulls.value == 0
        assert write(t=empty.table, n=0, width=width, tb=0) == 0
        sync(out)
        raw = out.cpu().numpy()
        assert (raw[:width] == 0).all() and (raw[width:] == 0xEE).all()
        assert (data.cpu().numpy() == 0xEE).all() and (valid.cpu().numpy() == 0xEE).all()
        out[:64] = 0xEE
    assert write(tb=0) == 0                                       # nothing to write: nothing launched
    assert lib.arx_get_counter(COUNTER) == before
    # the good call; a NULL replacement of length 0 is taken
    assert offsets(mode=REPLACE) == 0 and total.value == 14 and nulls.value == 0, lib.arx_last_error()
    assert write(mode=REPLACE) == 0, lib.arx_last_error()
    assert offsets(mode=REPLACE, r=2) == 0 and write(mode=REPLACE, rp=rep.data_ptr(), r=2) == 0, lib.arx_last_error()
    sync(data)
    assert out.cpu().numpy()[:12].view(np.int32).tolist() == [0, 9, 14] and data.cpu().numpy()[:15].tobytes() == b"xabx-xabxab-ab\xee"
    assert valid.cpu().numpy()[:8].view(np.uint64)[0] == 3
    assert lib.arx_get_counter(COUNTER) == before + 4


def _offsets_past_int32(amd):
    """Two columns whose offsets claim 2^30 + 1 bytes a row over a 16-byte data buffer, through the offsets call alone,
    which reads no data byte.  int32 offsets: "offset overflow while joining", out_offsets unwritten; int64 offsets: the
    offsets above 2^31, exact."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    lib = _lib.get_lib()
    size = 2**30 + 1
    data = to_device(np.zeros(16, np.uint8))
    sep = device_bytes(b"-")
    for width, n_rows in ((4, 1), (8, 3)):        # (int32 offsets hold one such row a column; two columns overflow the result)
        offs = to_device((np.arange(n_rows + 1, dtype=np.int64) * size).astype(np.int64 if width == 8 else np.int32))
        table = (_lib.ArxJoinOperand * 3)()
        for slot in table[:2]:
            slot.kind = COLUMN
            slot.column = _lib.ArxBinarySpan(None, offs.data_ptr(), data.data_ptr(), 0, n_rows, 0)
        table[2].kind, table[2].literal, table[2].literal_length = LITERAL, sep.data_ptr(), 1
        ws_bytes = lib.arx_binary_join_workspace_bytes(n_rows, width)
        ws = to_device(np.zeros(ws_bytes, np.uint8))
        out_offsets = to_device(np.full((n_rows + 1) * width, 0xEE, np.uint8))
        valid = to_device(np.zeros(8, np.uint8))
        total, nulls = C.c_int64(-1), C.c_int64(-1)
        rc = lib.arx_binary_join_offsets(table, 3, n_rows, width, EMIT_NULL, 0, ws.data_ptr(), ws_bytes, out_offsets.data_ptr(),
                                         valid.data_ptr(), C.byref(nulls), C.byref(total), None)
        sync(out_offsets)
        if width == 4:
            assert rc == _lib.ARX_INVALID and b"offset overflow while joining" in lib.arx_last_error(), lib.arx_last_error()
            assert (out_offsets.cpu().numpy()[: (n_rows + 1) * width] == 0xEE).all()           # out_offsets unwritten
            assert total.value <= 0 and nulls.value == -1
        else:
            assert rc == 0, lib.arx_last_error()
            row = 2 * size + 1
            assert total.value == n_rows * row and row > 2**31 and nulls.value == 0
            assert out_offsets.cpu().numpy()[: (n_rows + 1) * 8].view(np.int64).tolist() == [0, row, 2 * row, 3 * row]
    # the mirror reports the overflow as ArrowInvalid
    arr = amd.Array.from_pyarrow(pa.array([""], pa.string()))
    big = amd.Array(arr.type, 1, [None, to_device(np.array([0, 2**30 + 1], np.int32)), data], 0, 0)
    with pytest.raises(amd.ArrowInvalid, match="offset overflow while joining"):
        amd.compute.binary_join_element_wise(big, big, "-")


def test_reference_skip_still_drops_all_null_rows():
    """The reference defect the device does not reproduce (the module docstring): a pyarrow that keeps the row fails here,
    and the skip comparisons above can then take such rows in."""
    got = pc.binary_join_element_wise(pa.array(["a", None, "c", ""]), "-", null_handling="skip")
    assert len(got) == 3 and got.to_pylist() == ["a", "c", ""]


# ---------------------------------------------------------------- emu tier
@pytest.mark.emu
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_string_join_grid(emu_ctx, n):
    _grid(emu_ctx, n)


@pytest.mark.emu
def test_string_join_operand_counts(emu_ctx):
    _operand_counts(emu_ctx)


@pytest.mark.emu
def test_string_join_separators(emu_ctx):
    _separators(emu_ctx)


@pytest.mark.emu
def test_string_join_operand_kinds(emu_ctx):
    _operand_kinds(emu_ctx)


@pytest.mark.emu
def test_string_join_long_rows(emu_ctx):
    _long_rows(emu_ctx)


@pytest.mark.emu
def test_string_join_validity(emu_ctx):
    _validity(emu_ctx)


@pytest.mark.emu
def test_string_join_skip_rows_without_a_value(emu_ctx):
    _skip_rows_without_a_value(emu_ctx)


@pytest.mark.emu
def test_string_join_mirror(emu_ctx):
    _mirror(emu_ctx)


@pytest.mark.emu
def test_string_join_c_abi_large_types(emu_ctx):
    _large_types(emu_ctx)


@pytest.mark.emu
def test_string_join_c_abi_null_rows_spanning_bytes(emu_ctx):
    _null_rows_spanning_bytes(emu_ctx)


@pytest.mark.emu
def test_string_join_c_abi_contract(emu_ctx):
    _c_abi_contract(emu_ctx)


@pytest.mark.emu
def test_string_join_offsets_past_int32(emu_ctx):
    _offsets_past_int32(emu_ctx)


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_gpu_string_join_grid(gpu_ctx, n):
    _grid(gpu_ctx, n)


@pytest.mark.gpu
def test_gpu_string_join_operand_counts_and_kinds(gpu_ctx):
    _operand_counts(gpu_ctx)
    _operand_kinds(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_join_separators_and_long_rows(gpu_ctx):
    _separators(gpu_ctx)
    _long_rows(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_join_validity_skip_and_mirror(gpu_ctx):
    _validity(gpu_ctx)
    _skip_rows_without_a_value(gpu_ctx)
    _mirror(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_join_c_abi(gpu_ctx):
    _large_types(gpu_ctx)
    _null_rows_spanning_bytes(gpu_ctx)
    _c_abi_contract(gpu_ctx)
    _offsets_past_int32(gpu_ctx)


@pytest.mark.gpu
def test_gpu_string_join_1e6_rows_from_numpy_buffers(gpu_ctx):
    rng = rng_for("1e6")
    n = 1_000_000

    def numpy_column(mean, null_p, long_rows):
        lens = rng.integers(0, 2 * mean + 1, n)
        lens[rng.integers(0, n, long_rows)] = 30_000                  # a few long rows among the short ones
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=offsets[1:])
        data = rng.integers(97, 123, int(offsets[-1])).astype(np.uint8)
        valid = rng.random(n) >= null_p
        return pa.Array.from_buffers(pa.string(), n, [pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()),
                                                      pa.py_buffer(offsets.astype(np.int32).tobytes()), pa.py_buffer(data.tobytes())]), valid

    a, va = numpy_column(10, 0.05, 20)
    b, vb = numpy_column(6, 0.05, 5)
    keep = va | vb                                                    # the rows the reference does not drop under skip
    rows = pa.array(np.flatnonzero(keep))
    da, db = gpu_ctx.Array.from_pyarrow(a), gpu_ctx.Array.from_pyarrow(b)
    check_pairs(gpu_ctx, [(a.slice(13), da.slice(13)), (b.slice(13), db.slice(13)), ", "], pa.string(), modes=MODES[:3], what="1e6")
    got = gpu_ctx.compute.binary_join_element_wise(da, db, ", ", null_handling="skip")
    assert got.null_count == 0 and got.validity is None
    host = got.to_pyarrow()
    assert host.take(rows).equals(pc.binary_join_element_wise(a.take(rows), b.take(rows), ", ", null_handling="skip"))
    dropped = pa.array(np.flatnonzero(~keep))
    assert len(dropped) > 1000 and pc.all(pc.equal(host.take(dropped), "")).as_py()
