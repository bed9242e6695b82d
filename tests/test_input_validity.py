"""The validity of a one-operand kernel's result (compute._under_input_validity, and the temporal kernels that write theirs
themselves): one policy for the string families, the one-operand arithmetic and the date / time fields.

No bitmap when the input has none or is known to hold no null; the input's own bitmap, shared, when the input is at
offset 0; a copy re-based to offset 0 otherwise.  Whichever it is, the result equals pyarrow.compute's on the host copy
of the same array, with its null count, at offset 0, and the input's bitmap is left as it was.

77 rows, and slice(7) of them: the smallest sizes at which a bitmap crosses a 64-bit word at an odd bit offset."""
import functools

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

N = 77
# name -> (the column it takes, the call on either module)
CALLS = {
    "binary_length": ("string", lambda m, a: m.binary_length(a)),
    "utf8_length": ("string", lambda m, a: m.utf8_length(a)),
    "utf8_slice_codeunits": ("string", lambda m, a: m.utf8_slice_codeunits(a, 1, 3)),
    "utf8_trim_whitespace": ("string", lambda m, a: m.utf8_trim_whitespace(a)),
    "replace_substring": ("string", lambda m, a: m.replace_substring(a, "a", "bb")),
    "match_substring": ("string", lambda m, a: m.match_substring(a, "a")),
    "negate": ("int32", lambda m, a: m.negate(a)),
    "year": ("timestamp", lambda m, a: m.year(a)),
}
SHAPES = ("whole", "slice(7)", "all valid", "no bitmap")


@functools.lru_cache(maxsize=None)
def columns(kind):
    """shape -> the host column: 77 rows with about a tenth of them null, slice(7) of it, the same rows under a bitmap of
    all ones, and without a bitmap."""
    rng = np.random.default_rng([0x1A11D, len(kind)])
    mask = rng.random(N) < 0.1
    mask[[3, 40, 70]] = True                                        # a null before the slice's start, and in either word
    if kind == "string":
        pool = ["", "a", " banana\t", "　café a la carte ", "xyz", "  aa  ", "日本語a"]
        rows, typ = [pool[i] for i in rng.integers(0, len(pool), N)], pa.string()
    elif kind == "int32":
        rows, typ = [int(v) for v in rng.integers(-1000, 1000, N)], pa.int32()
    else:
        rows, typ = [int(v) for v in rng.integers(-2**31, 2**32, N)], pa.timestamp("s")
    nulls = pa.array(rows, typ, mask=mask)
    plain = pa.array(rows, typ)
    ones = pa.Array.from_buffers(typ, N, [pa.py_buffer(b"\xff" * ((N + 7) // 8)), *plain.buffers()[1:]])
    assert nulls.null_count == int(mask.sum()) and ones.null_count == 0 and plain.buffers()[0] is None
    return {"whole": nulls, "slice(7)": nulls.slice(7), "all valid": ones, "no bitmap": plain}


@functools.lru_cache(maxsize=None)
def reference(name, shape):
    kind, call = CALLS[name]
    return call(pc, columns(kind)[shape])


def _check(amd, name):
    from arrow_amd.array import kUnknownNullCount

    kind, call = CALLS[name]
    for shape in SHAPES:
        host = columns(kind)[shape]
        dev = amd.Array.from_pyarrow(columns(kind)["whole"]).slice(7) if shape == "slice(7)" else amd.Array.from_pyarrow(host)
        # what each shape is there for
        assert dev.length == (N - 7 if shape == "slice(7)" else N)
        assert (dev.validity is None) == (shape == "no bitmap")
        assert dev._null_count == {"whole": host.null_count, "slice(7)": kUnknownNullCount, "all valid": 0, "no bitmap": 0}[shape]
        before = None if dev.validity is None else dev.validity.cpu().numpy().copy()
        got = call(amd.compute, dev)
        want = reference(name, shape)
        assert got.to_pyarrow().equals(want), (name, shape)
        assert got.null_count == want.null_count, (name, shape)
        assert got.offset == 0, (name, shape)
        if shape in ("all valid", "no bitmap"):
            assert got.validity is None, (name, shape)
        if shape == "whole":
            assert before is not None and (dev.validity.cpu().numpy() == before).all(), (name, shape)
            assert before[:(N + 7) // 8].tobytes() == host.buffers()[0].to_pybytes()[:(N + 7) // 8], (name, shape)


@pytest.mark.emu
@pytest.mark.parametrize("name", list(CALLS))
def test_result_under_input_validity(emu_ctx, name):
    _check(emu_ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CALLS))
def test_gpu_result_under_input_validity(gpu_ctx, name):
    _check(gpu_ctx, name)
