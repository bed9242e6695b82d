"""Host-side mirror of the arrow::compute API surface for the hot path, over device arrays.

Same names, argument meaning and error behaviour as the reference:
  FunctionRegistry / Function / Kernel        cpp/src/arrow/compute/registry.h:46, function.h:146-378,
                                              kernel.h:556-769
  CallFunction                                cpp/src/arrow/compute/exec.cc:1362-1390
  Filter / Take / SortIndices / Cast wrappers cpp/src/arrow/compute/api_vector.cc:334-423, cast.cc:239
  FilterOptions / TakeOptions / ...           cpp/src/arrow/compute/api_vector.h:37-104,
                                              api_aggregate.h:48-59
Every kernel `exec` here only allocates outputs, applies the reference's host-side decisions
(output validity allocation, null_count bookkeeping, shape dispatch) and calls the C ABI of
libarrow_amd.so (include/arrow_amd.h).  There is no CPU compute path.
"""
from __future__ import annotations

import builtins
import ctypes as C
import threading

import numpy as np
import torch

from . import _lib, tracing
from ._lib import (ArrowIndexError, ArrowInvalid, ArrowNotImplementedError, check)  # noqa: F401
from .array import (Array, DataType, RunEndEncoded, Scalar, alloc, bitmap_nbytes, bool_, current_stream, float32,
                    float64, int8, int16, int32, int64, kUnknownNullCount, uint8, uint16, uint32, uint64,
                    INDEX_TYPE_ID, is_base_binary)

# --------------------------------------------------------------------------- options
class FunctionOptions:
    pass


class FilterOptions(FunctionOptions):
    """api_vector.h:37-52.  null_selection_behavior: 'drop' | 'emit_null'."""

    def __init__(self, null_selection_behavior: str = "drop"):
        if null_selection_behavior not in ("drop", "emit_null"):
            raise ArrowInvalid(f"invalid null_selection_behavior {null_selection_behavior!r}")
        self.null_selection_behavior = null_selection_behavior

    @property
    def code(self) -> int:
        return _lib.FILTER_EMIT_NULL if self.null_selection_behavior == "emit_null" else _lib.FILTER_DROP


class TakeOptions(FunctionOptions):
    """api_vector.h:54-63."""

    def __init__(self, boundscheck: bool = True):
        self.boundscheck = bool(boundscheck)


class CastOptions(FunctionOptions):
    def __init__(self, to_type: DataType, allow_float_truncate: bool = False, allow_int_overflow: bool = False):
        self.to_type = to_type
        self.allow_float_truncate = allow_float_truncate
        self.allow_int_overflow = allow_int_overflow        # CastOptions::Unsafe sets it (cast.h:60-75)


class ArraySortOptions(FunctionOptions):
    """api_vector.h:93-104."""

    def __init__(self, order: str = "ascending", null_placement: str = "at_end"):
        if order not in ("ascending", "descending"):
            raise ArrowInvalid(f"invalid sort order {order!r}")
        if null_placement not in ("at_start", "at_end"):
            raise ArrowInvalid(f"invalid null placement {null_placement!r}")
        self.order = order
        self.null_placement = null_placement


class SortOptions(FunctionOptions):
    """api_vector.h:106-: sort_keys = [(name, order)]; for a plain Array only the order is used."""

    def __init__(self, sort_keys=(("", "ascending"),), null_placement: str = "at_end"):
        self.sort_keys = list(sort_keys)
        self.null_placement = null_placement


class ScalarAggregateOptions(FunctionOptions):
    """api_aggregate.h:48-59."""

    def __init__(self, skip_nulls: bool = True, min_count: int = 1):
        self.skip_nulls = bool(skip_nulls)
        self.min_count = int(min_count)


class MatchSubstringOptions(FunctionOptions):
    """api_scalar.h MatchSubstringOptions: the literal `pattern` (str, UTF-8 encoded, or bytes) and ignore_case."""

    def __init__(self, pattern="", ignore_case: bool = False):
        self.pattern = pattern
        self.ignore_case = bool(ignore_case)


class SliceOptions(FunctionOptions):
    """api_scalar.h SliceOptions: start, stop (None: to the row's end) and step, as Python's slice takes them."""

    def __init__(self, start: int = 0, stop=None, step: int = 1):
        self.start = int(start)
        self.stop = None if stop is None else int(stop)
        self.step = int(step)


class TrimOptions(FunctionOptions):
    """api_scalar.h TrimOptions: the `characters` to trim (str, UTF-8 encoded, or bytes)."""

    def __init__(self, characters=""):
        self.characters = characters


class ReplaceSubstringOptions(FunctionOptions):
    """api_scalar.h ReplaceSubstringOptions: the literal `pattern` and its `replacement` (str, UTF-8 encoded, or bytes) and
    max_replacements, the matches replaced in each row (None or negative: all of them)."""

    def __init__(self, pattern="", replacement="", max_replacements=None):
        self.pattern = pattern
        self.replacement = replacement
        self.max_replacements = None if max_replacements is None else int(max_replacements)


class JoinOptions(FunctionOptions):
    """api_scalar.h JoinOptions: null_handling ("emit_null": a null value makes the row null, "skip": it is left out with
    one separator, "replace": it contributes `null_replacement`, str, UTF-8 encoded, or bytes)."""

    def __init__(self, null_handling="emit_null", null_replacement=""):
        if null_handling not in _lib.JOIN_NULL_HANDLING:
            raise ValueError(f'"{null_handling}" is not a valid null handling')
        self.null_handling = null_handling
        self.null_replacement = null_replacement


class ElementWiseAggregateOptions(FunctionOptions):
    """api_scalar.h ElementWiseAggregateOptions: skip_nulls (a row is null only where every operand is null)."""

    def __init__(self, skip_nulls: bool = True):
        self.skip_nulls = bool(skip_nulls)


class DayOfWeekOptions(FunctionOptions):
    """api_scalar.h DayOfWeekOptions: count_from_zero (Monday = 0 rather than 1 at the defaults) and week_start, the ISO
    weekday (Monday = 1 .. Sunday = 7) the numbering starts at."""

    def __init__(self, count_from_zero: bool = True, week_start: int = 1):
        self.count_from_zero = bool(count_from_zero)
        self.week_start = int(week_start)


# RoundMode of api_scalar.h, in the enum's order (= ARX_ROUND_*)
_ROUND_MODES = ("down", "up", "towards_zero", "towards_infinity", "half_down", "half_up", "half_towards_zero",
                "half_towards_infinity", "half_to_even", "half_to_odd")


def _round_mode(round_mode) -> str:
    if round_mode not in _ROUND_MODES:
        raise ArrowInvalid(f'"{round_mode}" is not a valid round mode')
    return round_mode


class RoundOptions(FunctionOptions):
    """api_scalar.h RoundOptions: ndigits (negative: to tens, hundreds, ...) and one of the ten round modes."""

    def __init__(self, ndigits: int = 0, round_mode: str = "half_to_even"):
        self.ndigits = int(ndigits)
        self.round_mode = _round_mode(round_mode)


class RoundToMultipleOptions(FunctionOptions):
    """api_scalar.h RoundToMultipleOptions: multiple (a Python number or an arrow_amd.Scalar; cast to the column's type
    by the function) and one of the ten round modes."""

    def __init__(self, multiple=1.0, round_mode: str = "half_to_even"):
        self.multiple = multiple
        self.round_mode = _round_mode(round_mode)


# --------------------------------------------------------------------------- scratch space
_tls = threading.local()


def _workspace(device: torch.device, nbytes: int, slot: str = "ws") -> torch.Tensor:
    """Per-thread, per-device scratch buffer (the C ABI never allocates)."""
    cache = getattr(_tls, "cache", None)
    if cache is None:
        cache = _tls.cache = {}
    key = (slot, str(device))
    buf = cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = cache[key] = alloc(max(nbytes, 1 << 16), device)
    return buf


def _lib_and_stream(device: torch.device):
    return _lib.get_lib(), current_stream(device)


def copy_buffer(src: torch.Tensor, dst: torch.Tensor | None = None) -> torch.Tensor:
    """Device-to-device copy of a uint8 buffer with the HIP kernel (arx_buffer_copy) — the kROCM -> kROCM leg of
    MemoryManager::CopyBufferTo (cpp/src/arrow/device.h:214-222).  Returns `dst` (allocated when None)."""
    lib, stream = _lib_and_stream(src.device)
    if dst is None:
        dst = alloc(src.numel(), src.device)
    if dst.numel() < src.numel():
        raise ValueError("copy_buffer: destination smaller than source")
    check(lib.arx_buffer_copy(src.data_ptr(), dst.data_ptr(), src.numel(), stream))
    return dst


# --------------------------------------------------------------------------- kernels (exec)
def _propagate_validity(args, length: int, device):
    """NullHandling::INTERSECTION (PropagateNullsSpans, exec.cc:1222-1281) on the device.
    Returns (validity buffer or None, null_count)."""
    arrs = [a for a in args if isinstance(a, Array) and a.may_have_nulls()]
    for a in args:
        if isinstance(a, Scalar) and not a.is_valid:
            buf = alloc(bitmap_nbytes(length), device, zero=True)  # all null
            return buf, length
    if not arrs:
        return None, 0
    lib, stream = _lib_and_stream(device)
    if len(arrs) == 1 and arrs[0].offset == 0:
        return arrs[0].validity, arrs[0].null_count  # zero-copy share
    out = alloc(bitmap_nbytes(length), device)
    first = arrs[0]
    if len(arrs) == 1:
        check(lib.arx_bitmap_copy(first.validity.data_ptr(), first.offset, length, out.data_ptr(), stream))
        return out, first.null_count
    check(lib.arx_bitmap_and(first.validity.data_ptr(), first.offset, arrs[1].validity.data_ptr(),
                             arrs[1].offset, length, out.data_ptr(), stream))
    for a in arrs[2:]:
        check(lib.arx_bitmap_and(out.data_ptr(), 0, a.validity.data_ptr(), a.offset, length,
                                 out.data_ptr(), stream))
    return out, kUnknownNullCount


def _exec_array_filter(args, options):
    """PrimitiveFilterExec (vector_selection_filter_internal.cc:445-510)."""
    values, mask = args
    options = options or FilterOptions()
    if mask.type != bool_:
        raise ArrowNotImplementedError("filter: the selection must be a boolean array")
    if values.type == bool_:
        return _exec_boolean_filter(args, options)
    if values.length != mask.length:  # ExecSpanIterator::Init, exec.cc:349-355
        raise ArrowInvalid("Array arguments must all be the same length")
    dev = values.device
    lib, stream = _lib_and_stream(dev)
    n = mask.length
    ws_bytes = lib.arx_filter_workspace_bytes(n)
    ws = _workspace(dev, ws_bytes)
    mspan, vspan = mask.span(), values.span()
    out_len = C.c_int64(0)
    check(lib.arx_filter_count(C.byref(mspan), options.code, ws.data_ptr(), ws.numel(),
                               C.byref(out_len), stream))
    s = out_len.value
    filter_null_count_is_zero = mask.null_count == 0
    drop = options.code == _lib.FILTER_DROP
    null_count = 0 if (values.null_count == 0 and (drop or filter_null_count_is_zero)) else kUnknownNullCount
    allocate_validity = values.null_count != 0 or not filter_null_count_is_zero
    w = values.type.byte_width
    out_data = alloc(s * w, dev)
    out_valid = alloc(bitmap_nbytes(s), dev) if allocate_validity else None
    with tracing.span("arx_filter_exec"):
        check(lib.arx_filter_exec(C.byref(vspan), w, C.byref(mspan), options.code, ws.data_ptr(), s,
                                  out_data.data_ptr(),
                                  None if out_valid is None else out_valid.data_ptr(), stream))
    return Array(values.type, s, [out_valid, out_data], null_count, 0)


def get_take_indices(mask: Array, null_selection_behavior: str = "drop") -> Array:
    """GetTakeIndices (vector_selection_take_internal.cc:258-305): uint16 for <= 65535 rows."""
    options = FilterOptions(null_selection_behavior)
    if mask.type != bool_:
        raise ArrowNotImplementedError("GetTakeIndices needs a boolean array")
    dev = mask.device
    lib, stream = _lib_and_stream(dev)
    n = mask.length
    if n > 0xFFFFFFFF:
        raise ArrowNotImplementedError(
            "Filter length exceeds UINT32_MAX, consider a different strategy for selecting elements")
    ws = _workspace(dev, lib.arx_filter_workspace_bytes(n))
    mspan = mask.span()
    out_len = C.c_int64(0)
    check(lib.arx_filter_count(C.byref(mspan), options.code, ws.data_ptr(), ws.numel(),
                               C.byref(out_len), stream))
    s = out_len.value
    itype = uint16 if n <= 65535 else uint32
    emit = options.code == _lib.FILTER_EMIT_NULL and mask.may_have_nulls()
    out = alloc(s * itype.byte_width, dev)
    out_valid = alloc(bitmap_nbytes(s), dev) if emit else None
    with tracing.span("arx_mask_to_indices"):
        check(lib.arx_mask_to_indices(C.byref(mspan), options.code, ws.data_ptr(), s, itype.byte_width,
                                      out.data_ptr(),
                                      None if out_valid is None else out_valid.data_ptr(), stream))
    return Array(itype, s, [out_valid, out], kUnknownNullCount if emit else 0, 0)


class _LazyCount:
    """null_count = length - valid_count, resolved on first read (take sets it exactly, :377)."""

    def __init__(self, length, counter):
        self.length, self.counter = length, counter

    def __call__(self):
        return int(self.length - int(self.counter.cpu().view(torch.int64)[0]))


def _exec_array_take(args, options):
    """FixedWidthTakeExec (vector_selection_take_internal.cc:405-468)."""
    values, indices = args
    options = options or TakeOptions()
    if indices.type.name not in INDEX_TYPE_ID:
        raise ArrowNotImplementedError(f"take: unsupported index type {indices.type.name}")
    dev = values.device
    lib, stream = _lib_and_stream(dev)
    tid = INDEX_TYPE_ID[indices.type.name]
    ispan, vspan = indices.span(), values.span()
    if values.type == bool_:
        return _take_boolean(values, indices, options, lib, stream, tid, ispan, vspan)
    if options.boundscheck:
        ws = _workspace(dev, lib.arx_take_workspace_bytes(), "take")
        check(lib.arx_check_index_bounds(C.byref(ispan), tid, values.length, ws.data_ptr(), ws.numel(),
                                         stream))
    m = indices.length
    w = values.type.byte_width
    allocate_validity = values.may_have_nulls() or indices.may_have_nulls()
    out_data = alloc(m * w, dev)
    out_valid = alloc(bitmap_nbytes(m), dev) if allocate_validity else None
    counter = None
    if allocate_validity:
        counter = torch.zeros(8, dtype=torch.uint8, device=dev)
    with tracing.span("arx_take"):
        check(lib.arx_take(C.byref(vspan), w, C.byref(ispan), tid, out_data.data_ptr(),
                           None if out_valid is None else out_valid.data_ptr(),
                           None if counter is None else counter.data_ptr(), stream))
    out = Array(values.type, m, [out_valid, out_data], 0, 0)
    if allocate_validity:
        out.set_lazy_null_count(_LazyCount(m, counter))
    return out


def _take_boolean(values, indices, options, lib, stream, tid, ispan, vspan):
    """Take on bit-packed boolean values (the 1-bit Gather of gather_internal.h)."""
    dev = values.device
    if options.boundscheck:
        ws = _workspace(dev, lib.arx_take_workspace_bytes(), "take")
        check(lib.arx_check_index_bounds(C.byref(ispan), tid, values.length, ws.data_ptr(), ws.numel(), stream))
    m = indices.length
    allocate_validity = values.may_have_nulls() or indices.may_have_nulls()
    out_bits = alloc(bitmap_nbytes(m), dev, zero=True)
    out_valid = alloc(bitmap_nbytes(m), dev, zero=True) if allocate_validity else None
    counter = torch.zeros(8, dtype=torch.uint8, device=dev) if allocate_validity else None
    check(lib.arx_take_bits(C.byref(vspan), C.byref(ispan), tid, out_bits.data_ptr(),
                            None if out_valid is None else out_valid.data_ptr(),
                            None if counter is None else counter.data_ptr(), stream))
    out = Array(bool_, m, [out_valid, out_bits], 0, 0)
    if allocate_validity:
        out.set_lazy_null_count(_LazyCount(m, counter))
    return out


def _exec_boolean_filter(args, options):
    """Filter on boolean values = take of GetTakeIndices(mask), like the var-width types."""
    values, mask = args
    options = options or FilterOptions()
    if values.length != mask.length:
        raise ArrowInvalid("Array arguments must all be the same length")
    indices = get_take_indices(mask, options.null_selection_behavior)
    return _exec_array_take([values, indices], TakeOptions(boundscheck=False))


def _exec_binary_take(args, options):
    """TakeExec for base binary (vector_selection_take_internal.cc, VarBinary take): offsets,
    validity and the byte total first (the reference grows a builder), then the bytes."""
    values, indices = args
    options = options or TakeOptions()
    if indices.type.name not in INDEX_TYPE_ID:
        raise ArrowNotImplementedError(f"take: unsupported index type {indices.type.name}")
    dev = values.device
    lib, stream = _lib_and_stream(dev)
    tid = INDEX_TYPE_ID[indices.type.name]
    ispan, vspan = indices.span(), values.binary_span()
    if options.boundscheck:
        ws = _workspace(dev, lib.arx_take_workspace_bytes(), "take")
        check(lib.arx_check_index_bounds(C.byref(ispan), tid, values.length, ws.data_ptr(), ws.numel(),
                                         stream))
    m = indices.length
    allocate_validity = values.may_have_nulls() or indices.may_have_nulls()
    out_offsets = alloc((m + 1) * 4, dev)
    out_valid = alloc(bitmap_nbytes(m), dev) if allocate_validity else None
    counter = torch.zeros(8, dtype=torch.uint8, device=dev) if allocate_validity else None
    ws = _workspace(dev, lib.arx_binary_take_workspace_bytes(m), "binary_take")
    total = C.c_int64(0)
    with tracing.span("arx_binary_take_offsets"):
        check(lib.arx_binary_take_offsets(C.byref(vspan), C.byref(ispan), tid, ws.data_ptr(), ws.numel(),
                                          out_offsets.data_ptr(),
                                          None if out_valid is None else out_valid.data_ptr(),
                                          None if counter is None else counter.data_ptr(),
                                          C.byref(total), stream))
    out_data = alloc(total.value, dev)
    with tracing.span("arx_binary_take_data"):
        check(lib.arx_binary_take_data(C.byref(vspan), m, ws.data_ptr(), ws.numel(), out_offsets.data_ptr(),
                                       total.value, out_data.data_ptr(), stream))
    out = Array(values.type, m, [out_valid, out_offsets, out_data], 0, 0)
    if allocate_validity:
        out.set_lazy_null_count(_LazyCount(m, counter))
    return out


def _exec_binary_filter(args, options):
    """BinaryFilterImpl (vector_selection_filter_internal.cc:517-800) as take(GetTakeIndices(mask)):
    the same output by construction (GetTakeIndices emits exactly the slots the filter keeps, with
    nulls for EMIT_NULL)."""
    values, mask = args
    options = options or FilterOptions()
    if mask.type != bool_:
        raise ArrowNotImplementedError("filter: the selection must be a boolean array")
    if values.length != mask.length:
        raise ArrowInvalid("Array arguments must all be the same length")
    indices = get_take_indices(mask, options.null_selection_behavior)
    return _exec_binary_take([values, indices], TakeOptions(boundscheck=False))


# ARX_NUM_* of include/arrow_amd.h
_NUM_TYPE_ID = {"int8": 0, "uint8": 1, "int16": 2, "uint16": 3, "int32": 4, "uint32": 5, "int64": 6, "uint64": 7,
                "float": 8, "double": 9}
_NUMERIC = lambda t: t.name in _NUM_TYPE_ID  # noqa: E731


def _make_exec_cast_numeric(to_type: DataType):
    def _exec(args, options):
        """Any numeric pair (scalar_cast_numeric.cc:46-60, 190-207, 270-279): static_cast on every slot + the mode's
        check on the valid ones (arx_cast_numeric)."""
        (arr,) = args
        dev = arr.device
        lib, stream = _lib_and_stream(dev)
        n = arr.length
        out = alloc(n * to_type.byte_width, dev)
        ws = _workspace(dev, 64, "cast")
        sp = arr.span()
        with tracing.span("arx_cast_numeric"):
            check(lib.arx_cast_numeric(C.byref(sp), _NUM_TYPE_ID[arr.type.name], _NUM_TYPE_ID[to_type.name],
                                       int(bool(getattr(options, "allow_int_overflow", False))),
                                       int(bool(getattr(options, "allow_float_truncate", False))),
                                       ws.data_ptr(), ws.numel(), out.data_ptr(), stream))
        validity, nc = _propagate_validity([arr], n, dev)
        return Array(to_type, n, [validity, out], nc, 0)
    return _exec


def _scalar_value(x):
    return x.value if isinstance(x, Scalar) else x


_ARITH_CODE = {"add": 0, "subtract": 1, "multiply": 2}
_CMP_CODE = {"equal": 0, "not_equal": 1, "greater": 2, "greater_equal": 3, "less": 4, "less_equal": 5}


def _numeric_operands(left, right):
    """(array operand, n, left ptr | None, right ptr | None, host scalar holders) for the *_numeric entry points."""
    arr = left if isinstance(left, Array) else right
    n = arr.length
    if isinstance(left, Array) and isinstance(right, Array) and left.length != right.length:
        raise ArrowInvalid("Array arguments must all be the same length")
    dt = arr.type.np_dtype

    def scalar_ptr(x):
        if isinstance(x, Array):
            return None, None
        v = _scalar_value(x)
        holder = np.zeros(1, dtype=dt)
        if v is not None:
            holder[0] = dt.type(v)
        return holder, holder.ctypes.data

    lh, lsp = scalar_ptr(left)
    rh, rsp = scalar_ptr(right)
    lp = left.values_ptr() if isinstance(left, Array) else None
    rp = right.values_ptr() if isinstance(right, Array) else None
    return arr, n, lp, lsp, rp, rsp, (lh, rh)


def _validity_ptr(a):
    """(validity bitmap pointer | None, bit offset) of an operand: None for a scalar and for an array without nulls."""
    return (a.validity.data_ptr(), a.offset) if isinstance(a, Array) and a.may_have_nulls() else (None, 0)


def _has_null_scalar(left, right) -> bool:
    """A null scalar operand makes every slot of the result null: ScalarBinaryNotNull visits none, so no slot can fail
    a check (codegen_internal.h; the all-null validity itself comes from _propagate_validity)."""
    return any(isinstance(a, Scalar) and not a.is_valid for a in (left, right))


def _num_type_id(t: DataType) -> int:
    """ARX_NUM_* of a numeric type, or of the physical integer of a temporal one (timestamp / duration / time / date)."""
    if t.name in _NUM_TYPE_ID:
        return _NUM_TYPE_ID[t.name]
    from .array import is_temporal

    if is_temporal(t):
        return _NUM_TYPE_ID["int64" if t.bit_width == 64 else "int32"]
    raise ArrowNotImplementedError(f"no numeric kernel for {t.name}")


def _exec_compare_numeric(op_name):
    code = _CMP_CODE[op_name]

    def run(args, options):
        """CompareKernel<Type, Op>::Exec (scalar_compare.cc:259-298) for every numeric Type (registration :398-446)."""
        left, right = args
        arr, n, lp, lsp, rp, rsp, _keep = _numeric_operands(left, right)
        dev = arr.device
        lib, stream = _lib_and_stream(dev)
        out = alloc(bitmap_nbytes(n), dev, zero=True)
        with tracing.span("arx_compare_numeric"):
            check(lib.arx_compare_numeric(code, _num_type_id(arr.type), lp, lsp, rp, rsp, n, out.data_ptr(), stream))
        validity, nc = _propagate_validity([left, right], n, dev)
        return Array(bool_, n, [validity, out], nc, 0)
    return run


def _exec_arith_numeric(op_name, checked):
    code = _ARITH_CODE[op_name]

    def run(args, options):
        """ScalarBinary<T, T, T, Add|Subtract|Multiply> / ScalarBinaryNotNull<..., *Checked> for every numeric T
        (base_arithmetic_internal.h:45-150,290-364)."""
        left, right = args
        arr, n, lp, lsp, rp, rsp, _keep = _numeric_operands(left, right)
        dev = arr.device
        lib, stream = _lib_and_stream(dev)
        out = alloc(n * arr.type.byte_width, dev)
        validity, nc = _propagate_validity([left, right], n, dev)
        is_f = arr.type.name in ("float", "double")
        do_check = checked and not is_f and not _has_null_scalar(left, right)
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if do_check else None
        (lvp, lvo), (rvp, rvo) = _validity_ptr(left), _validity_ptr(right)
        with tracing.span("arx_arith_numeric"):
            check(lib.arx_arith_numeric(code, 1 if do_check else 0, _NUM_TYPE_ID[arr.type.name], lp, lsp, lvp, lvo, rp, rsp,
                                        rvp, rvo, n, out.data_ptr(), None if flag is None else flag.data_ptr(), stream))
        if flag is not None and int(flag.cpu()[0]) != 0:
            raise ArrowInvalid("overflow")   # AddChecked::Call, base_arithmetic_internal.h:77
        return Array(arr.type, n, [validity, out], nc, 0)
    return run


def _exec_divide_numeric(checked: bool):
    def run(args, options):
        """ScalarBinaryNotNull<T, T, T, Divide | DivideChecked> for every numeric T (base_arithmetic_internal.h:366-424,
        DivideWithOverflowGeneric util/int_util_overflow.h:124-138): only slots where both operands are valid are
        visited; the last failing slot names the error."""
        left, right = args
        arr, n, lp, lsp, rp, rsp, _keep = _numeric_operands(left, right)
        dev = arr.device
        lib, stream = _lib_and_stream(dev)
        null_scalar = _has_null_scalar(left, right)
        if null_scalar and rp is None:      # nothing is visited: keep the kernel away from a 0 divisor
            _keep[1][0] = 1
        out = alloc(n * arr.type.byte_width, dev)
        validity, nc = _propagate_validity([left, right], n, dev)
        errors = torch.zeros(2, dtype=torch.int64, device=dev)
        (lvp, lvo), (rvp, rvo) = _validity_ptr(left), _validity_ptr(right)
        with tracing.span("arx_divide_numeric"):
            check(lib.arx_divide_numeric(1 if checked else 0, _NUM_TYPE_ID[arr.type.name], lp, lsp, lvp, lvo, rp, rsp, rvp, rvo, n,
                                         out.data_ptr(), errors.data_ptr(), stream))
        if not null_scalar:
            last_overflow, last_zero = errors.cpu().tolist()
            if last_zero > last_overflow:
                raise ArrowInvalid("divide by zero")
            if last_overflow:
                raise ArrowInvalid("overflow")
        return Array(arr.type, n, [validity, out], nc, 0)
    return run


def _exec_kleene(op_code):
    def run(args, options):
        """KleeneAndOp / KleeneOrOp (scalar_boolean.cc:138-260), array x array."""
        left, right = args
        if not (isinstance(left, Array) and isinstance(right, Array)):
            raise ArrowNotImplementedError("and_kleene / or_kleene with a scalar operand is not on the gfx950 path")
        if left.length != right.length:
            raise ArrowInvalid("Array arguments must all be the same length")
        dev = left.device
        lib, stream = _lib_and_stream(dev)
        n = left.length
        out = alloc(bitmap_nbytes(n), dev, zero=True)
        nulls = left.may_have_nulls() or right.may_have_nulls()
        validity = alloc(bitmap_nbytes(n), dev, zero=True) if nulls else None
        ls, rs = left.span(), right.span()
        check(lib.arx_boolean_kleene(op_code, C.byref(ls), C.byref(rs), out.data_ptr(),
                                     None if validity is None else validity.data_ptr(), stream))
        return Array(bool_, n, [validity, out], kUnknownNullCount if nulls else 0, 0)
    return run


def _exec_invert(args, options):
    """InvertOp (scalar_boolean.cc:39-50): data inverted, validity propagated."""
    (arr,) = args
    dev = arr.device
    lib, stream = _lib_and_stream(dev)
    n = arr.length
    out = alloc(bitmap_nbytes(n), dev, zero=True)
    check(lib.arx_boolean_invert(arr.data.data_ptr(), arr.offset, n, out.data_ptr(), stream))
    validity, nc = _propagate_validity([arr], n, dev)
    return Array(bool_, n, [validity, out], nc, 0)


# ARX_KEY_* of include/arrow_amd.h
_SORT_KEY_TYPE = {"uint64": 0, "int64": 1, "uint32": 2, "int32": 3, "double": 4, "float": 5}


def _exec_array_sort_indices(args, options):
    """ArraySortIndices::Exec (vector_array_sort.cc:524-540): uint64 indices, never null."""
    (arr,) = args
    options = options or ArraySortOptions()
    dev = arr.device
    lib, stream = _lib_and_stream(dev)
    n = arr.length
    ws_bytes = lib.arx_sort_indices_workspace_bytes(n)
    ws = _workspace(dev, ws_bytes + 256, "sort")
    base = ws.data_ptr()
    aligned = (base + 255) & ~255
    out = alloc(n * 8, dev)
    span = arr.span()
    check(lib.arx_sort_indices(C.byref(span), _SORT_KEY_TYPE[arr.type.name],
                                  _lib.SORT_DESCENDING if options.order == "descending" else _lib.SORT_ASCENDING,
                                  _lib.NULLS_AT_START if options.null_placement == "at_start" else _lib.NULLS_AT_END,
                                  aligned, ws.numel() - (aligned - base), out.data_ptr(), stream))
    return Array(uint64, n, [None, out], 0, 0)


def _exec_array_sort_indices_bool(args, options):
    """array_sort_indices(boolean): the reference counts (ArrayCountSorter<BooleanType>, vector_array_sort.cc:360-400) —
    the rows of the falses, of the trues (descending: trues first) and of the nulls at their end, each class in row
    order: three GetTakeIndices over the value bitmap, its inverse and the inverted validity."""
    (arr,) = args
    options = options or ArraySortOptions()
    n = arr.length
    if n == 0:
        return Array(uint64, 0, [None, alloc(8, arr.device)], 0, 0)
    trues = indices_nonzero(arr)
    falses = indices_nonzero(invert(arr))
    parts = [trues, falses] if options.order == "descending" else [falses, trues]
    if arr.validity is not None and arr.null_count != 0:
        nulls = indices_nonzero(invert(Array(bool_, n, [None, arr.validity], 0, arr.offset)))
        parts = [nulls] + parts if options.null_placement == "at_start" else parts + [nulls]
    out = torch.cat([p.data[: p.length * 8] for p in parts])
    assert out.numel() == n * 8
    return Array(uint64, n, [None, out], 0, 0)


# --------------------------------------------------------------------------- registry
class Kernel:
    """arrow::compute::Kernel twin: a signature (tuple of DataType or None = any) + exec."""

    def __init__(self, in_types, exec_fn, out_type=None, is_varargs: bool = False):
        self.in_types = tuple(in_types)
        self.exec = exec_fn
        self.out_type = out_type
        self.is_varargs = is_varargs    # KernelSignature::is_varargs: the last in_type takes every further argument

    def matches(self, types) -> bool:
        if getattr(self, "is_varargs", False):         # (HashAggregateKernel borrows this method and has no such field)
            want = self.in_types + self.in_types[-1:] * (len(types) - len(self.in_types))
            return len(types) >= len(self.in_types) and all(w is None or (callable(w) and w(t)) or w == t for w, t in zip(want, types))
        if len(types) != len(self.in_types):
            return False
        return all(want is None or (callable(want) and want(t)) or want == t
                   for want, t in zip(self.in_types, types))


class Function:
    SCALAR, VECTOR, SCALAR_AGGREGATE, HASH_AGGREGATE, META = range(5)  # function.h:146-168

    def __init__(self, name: str, kind: int, arity: int, default_options=None, meta_impl=None, is_varargs: bool = False):
        self.name = name
        self.kind = kind
        self.arity = arity              # Arity::VarArgs(arity) when is_varargs: at least that many
        self.is_varargs = is_varargs
        self.default_options = default_options
        self.kernels: list[Kernel] = []
        self._meta_impl = meta_impl

    def add_kernel(self, kernel: Kernel) -> None:
        if len(kernel.in_types) != self.arity:  # function.cc:448-455
            raise ArrowInvalid(f"Added kernel accepts {len(kernel.in_types)} arguments but the "
                               f"function {self.name} accepts {self.arity}")
        self.kernels.append(kernel)

    @property
    def num_kernels(self) -> int:
        return len(self.kernels)

    def dispatch_exact(self, types) -> Kernel:
        """DispatchExactImpl (function.cc:122-157): the LAST matching kernel wins."""
        for k in reversed(self.kernels):
            if k.matches(types):
                return k
        names = ", ".join(t.name for t in types)
        raise ArrowNotImplementedError(
            f"Function '{self.name}' has no kernel matching input types ({names})")

    def execute(self, args, options=None):
        if self.is_varargs and len(args) < self.arity:      # function.cc CheckArity
            raise ArrowInvalid(f"VarArgs function '{self.name}' needs at least {self.arity} arguments but only "
                               f"{len(args)} passed")
        if not self.is_varargs and len(args) != self.arity:
            raise ArrowInvalid(f"Function '{self.name}' accepts {self.arity} arguments but "
                               f"{len(args)} passed")
        options = options if options is not None else self.default_options
        if self.kind == Function.META:
            return self._meta_impl(args, options)
        if self.kind == Function.HASH_AGGREGATE:  # function.cc:325-326
            raise ArrowNotImplementedError("Direct execution of HASH_AGGREGATE functions")
        types = [a.type for a in args]
        return self.dispatch_exact(types).exec(args, options)


class FunctionRegistry:
    """registry.h:46: name -> Function, aliases, no overwrite unless asked."""

    def __init__(self):
        self._fns: dict[str, Function] = {}
        self._lock = threading.Lock()

    def add_function(self, fn: Function, allow_overwrite: bool = False) -> None:
        with self._lock:
            if fn.name in self._fns and not allow_overwrite:
                raise KeyError(f"Already have a function registered with name: {fn.name}")
            self._fns[fn.name] = fn

    def add_alias(self, target: str, source: str) -> None:
        with self._lock:
            if source not in self._fns:
                raise KeyError(f"No function registered with name: {source}")
            self._fns[target] = self._fns[source]

    def get_function(self, name: str) -> Function:
        try:
            return self._fns[name]
        except KeyError:
            raise KeyError(f"No function registered with name: {name}") from None

    def get_function_names(self):
        return sorted(self._fns)

    @property
    def num_functions(self) -> int:
        return len(self._fns)


# --------------------------------------------------------------------------- hash_sum kernel
class GroupedSumInt64State:
    """KernelState of hash_sum(int64, uint32): the device twin of
    GroupedReducingAggregator<Int64Type, GroupedSumImpl> (hash_aggregate_numeric.cc:44-187).
    Dense per-group arrays in HBM: sums, counts, null_seen (the complement of `no_nulls_`)."""

    def __init__(self, options: ScalarAggregateOptions | None, device):
        self.options = options or ScalarAggregateOptions()
        self.device = torch.device(device)
        self.num_groups = 0
        self.sums = torch.zeros(0, dtype=torch.int64, device=self.device)
        self.counts = torch.zeros(0, dtype=torch.int64, device=self.device)
        self.null_seen = torch.zeros(0, dtype=torch.int32, device=self.device)


def _hash_sum_init(options, device=None):
    """HashAggregateInit<Impl> (hash_aggregate_internal.h:54-63)."""
    from .array import default_device

    return GroupedSumInt64State(options, device if device is not None else default_device())


def _grow(t: torch.Tensor, n: int) -> torch.Tensor:
    if t.numel() >= n:
        return t
    out = torch.zeros(max(n, 2 * t.numel()), dtype=t.dtype, device=t.device)
    out[: t.numel()].copy_(t)  # device-to-device buffer growth (TypedBufferBuilder::Append)
    return out


def _hash_sum_resize(state: GroupedSumInt64State, new_num_groups: int) -> None:
    """Resize (:61-68): new groups start at sum 0, count 0, no nulls seen."""
    state.sums = _grow(state.sums, new_num_groups)
    state.counts = _grow(state.counts, new_num_groups)
    state.null_seen = _grow(state.null_seen, new_num_groups)
    state.num_groups = new_num_groups


def _hash_sum_consume(state: GroupedSumInt64State, batch) -> None:
    """Consume (:70-83): batch = [values (Array | Scalar), group_ids (uint32 Array)]."""
    values, gids = batch[0], batch[1]
    if gids.type != uint32:
        raise ArrowInvalid("hash_sum: group ids must be uint32")
    lib, stream = _lib_and_stream(state.device)
    n = gids.length
    if isinstance(values, Scalar):
        span = _lib.ArxSpan(None, None, 0, n, 0 if values.is_valid else n)
        is_scalar, sv = 1, int(values.value or 0)
    else:
        if values.type != int64:
            raise ArrowNotImplementedError("hash_sum on the gfx950 path takes int64 values")
        if values.length != n:
            raise ArrowInvalid("Array arguments must all be the same length")
        span, is_scalar, sv = values.span(), 0, 0
    # with scratch the library partitions by group id and aggregates in LDS (large batches); without it every row is
    # a device atomic
    ws_bytes = lib.arx_hash_sum_consume_workspace_bytes(n, state.num_groups)
    ws_ptr, ws_len = None, 0
    if ws_bytes:
        ws = _workspace(state.device, ws_bytes + 256, "groupby")
        ws_ptr = (ws.data_ptr() + 255) & ~255
        ws_len = ws.numel() - (ws_ptr - ws.data_ptr())
    check(lib.arx_hash_sum_i64_consume_ws(C.byref(span), is_scalar, sv, gids.values_ptr(), n, state.num_groups,
                                          state.sums.data_ptr(), state.counts.data_ptr(),
                                          state.null_seen.data_ptr(), ws_ptr, ws_len, stream))


def _hash_sum_merge(state: GroupedSumInt64State, other: GroupedSumInt64State, group_id_mapping) -> None:
    """Merge (:85-107): group_id_mapping[other_g] = group id in `state` (uint32 Array)."""
    lib, stream = _lib_and_stream(state.device)
    g = group_id_mapping.length
    if g != other.num_groups:
        raise ArrowInvalid("group_id_mapping length must equal the other state's group count")
    check(lib.arx_hash_sum_i64_merge(state.sums.data_ptr(), state.counts.data_ptr(),
                                     state.null_seen.data_ptr(), other.sums.data_ptr(),
                                     other.counts.data_ptr(), other.null_seen.data_ptr(),
                                     group_id_mapping.values_ptr(), g, stream))


def _hash_sum_finalize(state: GroupedSumInt64State) -> Array:
    """Finalize (:130-152): int64 Array of num_groups sums; the validity bitmap is only
    materialised when a group is null (Finish :109-128) or skip_nulls is false."""
    lib, stream = _lib_and_stream(state.device)
    g = state.num_groups
    bits = alloc(bitmap_nbytes(g), state.device, zero=True)
    counter = torch.zeros(8, dtype=torch.uint8, device=state.device)
    check(lib.arx_hash_sum_i64_finalize(state.counts.data_ptr(), state.null_seen.data_ptr(), g,
                                        int(state.options.skip_nulls), state.options.min_count,
                                        bits.data_ptr(), counter.data_ptr(), stream))
    data = state.sums[:g].contiguous().view(torch.uint8)
    nulls = g - int(counter.cpu().view(torch.int64)[0])
    if state.options.skip_nulls and nulls == 0:
        return Array(int64, g, [None, data], 0, 0)
    return Array(int64, g, [bits, data], nulls if state.options.skip_nulls else kUnknownNullCount, 0)


class HashAggregateKernel:
    """compute/kernel.h:739-769: {signature, init, resize, consume, merge, finalize}."""

    def __init__(self, in_types, init, resize, consume, merge, finalize, out_type=None):
        self.in_types = tuple(in_types)
        self.init, self.resize, self.consume = init, resize, consume
        self.merge, self.finalize = merge, finalize
        self.out_type = out_type
        self.exec = None

    matches = Kernel.matches


class ExecBatch:
    """exec.h:174-261: a list of equal-length Arrays / Scalars plus the length."""

    def __init__(self, values, length: int | None = None):
        self.values = list(values)
        if length is None:
            lens = [v.length for v in self.values if isinstance(v, Array)]
            length = lens[0] if lens else 1
        self.length = length

    def __getitem__(self, i):
        return self.values[i]

    @property
    def num_values(self):
        return len(self.values)


class RecordBatch:
    """Just enough of arrow::RecordBatch for the Filter/Take meta-function shape dispatch."""

    def __init__(self, columns: dict):
        self.columns = dict(columns)
        lens = {c.length for c in self.columns.values()}
        if len(lens) > 1:
            raise ArrowInvalid("columns of a RecordBatch must have equal length")
        self.num_rows = lens.pop() if lens else 0


_FIXED_WIDTH = lambda t: t.bit_width >= 8  # noqa: E731
_INTEGER = lambda t: t.name in INDEX_TYPE_ID  # noqa: E731
_BASE_BINARY = lambda t: t.name in ("binary", "string")  # noqa: E731


def _filter_meta(args, options):
    """FilterMetaFunction::ExecuteImpl (vector_selection_filter_internal.cc:1043-1072)."""
    values, mask = args
    options = options or FilterOptions()
    if isinstance(values, RecordBatch):
        # FilterRecordBatch :925-960 — mask -> indices once, then Take per column
        if mask.length != values.num_rows:
            raise ArrowInvalid("Filter inputs must all be the same length")
        indices = get_take_indices(mask, options.null_selection_behavior)
        take_opts = TakeOptions(boundscheck=False)
        return RecordBatch({k: call_function("take", [c, indices], take_opts)
                            for k, c in values.columns.items()})
    if isinstance(mask, RunEndEncoded):
        mask = ree_mask_to_boolean(mask)
    return call_function("array_filter", [values, mask], options)


def ree_mask_to_boolean(mask: RunEndEncoded) -> Array:
    """A run_end_encoded<boolean> filter (the ree_filter input type of PopulateFilterKernels,
    vector_selection_filter_internal.cc:1090) expanded on the device into the plain boolean layout: every row carries
    its run's (valid, selected) pair, which is all VisitPlainxREEFilterOutputSegments reads."""
    if mask.values.type != bool_:
        raise ArrowNotImplementedError("filter: run-end-encoded masks must have boolean values")
    dev = mask.device
    lib, stream = _lib_and_stream(dev)
    n = mask.length
    bits = alloc(bitmap_nbytes(n), dev)
    has_nulls = mask.values.may_have_nulls()
    valid = alloc(bitmap_nbytes(n), dev) if has_nulls else None
    vs = mask.values.span()
    nruns = mask.run_ends.length
    re_ptr = mask.run_ends.values_ptr()
    check(lib.arx_ree_bool_expand(re_ptr, mask.run_ends.type.byte_width, nruns, C.byref(vs), mask.offset, n,
                                  bits.data_ptr(), None if valid is None else valid.data_ptr(), stream))
    return Array(bool_, n, [valid, bits], kUnknownNullCount if has_nulls else 0, 0)


def _take_meta(args, options):
    """TakeMetaFunction::ExecuteImpl (vector_selection_take_internal.cc:660-701), AAA and RAR."""
    values, indices = args
    options = options or TakeOptions()
    if isinstance(values, RecordBatch):
        # RAR (TakeRAR :619-633 runs TakeAAA per column): the fixed-width columns go through ONE launch that reads
        # the indices once (arx_take_columns, groups of 16); boolean / var-width columns keep their own kernels
        fused = {k: c for k, c in values.columns.items() if isinstance(c, Array) and c.type != bool_ and _FIXED_WIDTH(c.type)
                 and c.type.byte_width in (1, 2, 4, 8, 16, 32)}
        out = dict.fromkeys(values.columns)
        if len(fused) >= 2 and isinstance(indices, Array) and indices.type.name in INDEX_TYPE_ID:
            names = list(fused)
            for b in range(0, len(names), 16):
                part = names[b:b + 16]
                for k, col in zip(part, take_columns([fused[k] for k in part], indices, options.boundscheck)):
                    out[k] = col
        for k, c in values.columns.items():
            if out[k] is None:
                out[k] = call_function("array_take", [c, indices], options)
        return RecordBatch(out)
    return call_function("array_take", [values, indices], options)


def take_columns(columns, indices: Array, boundscheck: bool = True):
    """`take` of up to 16 fixed-width columns of equal length by one index array in one launch (arx_take_columns);
    per column the result of array_take.  One bounds check for all columns."""
    columns = list(columns)
    n = columns[0].length
    if any(c.length != n for c in columns):
        raise ArrowInvalid("columns of a RecordBatch must have equal length")
    dev = columns[0].device
    lib, stream = _lib_and_stream(dev)
    tid = INDEX_TYPE_ID[indices.type.name]
    ispan = indices.span()
    if boundscheck:
        ws = _workspace(dev, lib.arx_take_workspace_bytes(), "take")
        check(lib.arx_check_index_bounds(C.byref(ispan), tid, n, ws.data_ptr(), ws.numel(), stream))
    m, k = indices.length, len(columns)
    spans = (_lib.ArxSpan * k)(*[c.span() for c in columns])
    widths = (C.c_int32 * k)(*[c.type.byte_width for c in columns])
    out_data = [alloc(m * c.type.byte_width, dev) for c in columns]
    need = [c.may_have_nulls() or indices.may_have_nulls() for c in columns]
    out_valid = [alloc(bitmap_nbytes(m), dev) if nd else None for nd in need]
    counters = torch.zeros(k, dtype=torch.int64, device=dev)
    data_ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in out_data])
    valid_ptrs = (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in out_valid])
    with tracing.span("arx_take_columns"):
        check(lib.arx_take_columns(spans, widths, k, C.byref(ispan), tid, data_ptrs, valid_ptrs, counters.data_ptr(),
                                   stream))
    outs = []
    for j, c in enumerate(columns):
        a = Array(c.type, m, [out_valid[j], out_data[j]], 0, 0)
        if need[j]:
            a.set_lazy_null_count(_LazyColumnCount(m, counters, j))
        outs.append(a)
    return outs


class _LazyColumnCount:
    """null_count of column j from the per-column valid counters of arx_take_columns (read on first use)."""

    def __init__(self, length, counters, j):
        self.length, self.counters, self.j = length, counters, j

    def __call__(self):
        return self.length - int(self.counters[self.j].item())


def _cast_meta(args, options):
    """CastMetaFunction::ExecuteImpl (cast.cc:95-126): dispatch on the target type."""
    (arr,) = args
    if options is None or options.to_type is None:
        raise ArrowInvalid("Cast requires that options.to_type is set")
    if arr.type == options.to_type:
        return arr
    return _cast_table_lookup(options.to_type).execute([arr], options)


_cast_table: dict[str, Function] = {}


def _cast_table_lookup(to_type: DataType) -> Function:
    """GetCastFunction (cast.cc:207-214): casts live in a private table, not the registry."""
    try:
        return _cast_table[to_type.name]
    except KeyError:
        raise ArrowNotImplementedError(f"Unsupported cast to {to_type.name} (no available cast "
                                       "function for target type)") from None


def _sort_indices_meta(args, options):
    """SortIndicesMetaFunction::ExecuteImpl (vector_sort.cc:856-924) for Array input."""
    (arr,) = args
    options = options or SortOptions()
    order = options.sort_keys[0][1] if options.sort_keys else "ascending"
    return call_function("array_sort_indices", [arr], ArraySortOptions(order, options.null_placement))


def _build_registry() -> FunctionRegistry:
    reg = FunctionRegistry()

    f = Function("array_filter", Function.VECTOR, 2, FilterOptions())
    f.add_kernel(Kernel((_FIXED_WIDTH, bool_), _exec_array_filter))
    f.add_kernel(Kernel((bool_, bool_), _exec_boolean_filter))
    f.add_kernel(Kernel((_BASE_BINARY, bool_), _exec_binary_filter))
    reg.add_function(f)
    reg.add_function(Function("filter", Function.META, 2, FilterOptions(), _filter_meta))

    f = Function("array_take", Function.VECTOR, 2, TakeOptions())
    f.add_kernel(Kernel((_FIXED_WIDTH, _INTEGER), _exec_array_take))
    f.add_kernel(Kernel((bool_, _INTEGER), _exec_array_take))
    f.add_kernel(Kernel((_BASE_BINARY, _INTEGER), _exec_binary_take))
    reg.add_function(f)
    reg.add_function(Function("take", Function.META, 2, TakeOptions(), _take_meta))

    # one cast function per numeric target (GetCastFunction, cast.cc:207-214; kernels of
    # scalar_cast_numeric.cc:797-858); arx_cast_numeric picks the kernel for the pair
    for to in (int8, uint8, int16, uint16, int32, uint32, int64, uint64, float32, float64):
        c = Function("cast_" + to.name, Function.SCALAR, 1)
        c.add_kernel(Kernel((_NUMERIC,), _make_exec_cast_numeric(to), to))
        _cast_table[to.name] = c
    reg.add_function(Function("cast", Function.META, 1, None, _cast_meta))

    from .array import type_from_name
    numeric_types = [type_from_name(nm) for nm in _NUM_TYPE_ID]
    # temporal operands (timestamp / duration / time / date): the comparisons of their physical integers; both sides of
    # the same type and unit — the reference unifies units by implicit casts before dispatch (DispatchBest), and compares
    # a zoned timestamp only with a zoned one (scalar_compare.cc:299-313)
    from .array import is_temporal

    def _temporal_pair_kernel(name):
        run = _exec_compare_numeric(name)

        def checked(args, options):
            types = [a.type for a in args if isinstance(a, (Array, Scalar))]
            if len({t.name.split(", tz=")[0].rstrip("]") for t in types}) > 1:
                raise ArrowNotImplementedError(f"{name}: temporal operands of different types / units ({', '.join(t.name for t in types)})")
            zoned = {", tz=" in t.name for t in types if t.name.startswith("timestamp")}
            if len(zoned) > 1:
                raise ArrowInvalid("Cannot compare timestamp with timezone to timestamp without timezone, got: "
                                   + " and ".join(t.name for t in types))
            return run(args, options)
        return Kernel((is_temporal, is_temporal), checked, bool_)

    # one kernel per (function, numeric type) — which device kernel runs is the library's choice — plus the temporal pair
    for name in _CMP_CODE:
        f = Function(name, Function.SCALAR, 2)
        for t in numeric_types:
            f.add_kernel(Kernel((t, t), _exec_compare_numeric(name), bool_))
        f.add_kernel(_temporal_pair_kernel(name))
        for t in (type_from_name("string"), type_from_name("binary")):      # csrc/string_compare.hip
            f.add_kernel(Kernel((t, t), _exec_compare_binary(name), bool_))
        reg.add_function(f)

    for name, op, checked in (("add", "add", False), ("subtract", "subtract", False), ("multiply", "multiply", False),
                              ("add_checked", "add", True), ("subtract_checked", "subtract", True),
                              ("multiply_checked", "multiply", True)):
        f = Function(name, Function.SCALAR, 2)
        for t in numeric_types:
            f.add_kernel(Kernel((t, t), _exec_arith_numeric(op, checked), t))
        reg.add_function(f)

    for name, checked in (("divide", False), ("divide_checked", True)):
        f = Function(name, Function.SCALAR, 2)
        for t in numeric_types:
            f.add_kernel(Kernel((t, t), _exec_divide_numeric(checked), t))
        reg.add_function(f)

    for name, code in (("and_kleene", 0), ("or_kleene", 1)):
        f = Function(name, Function.SCALAR, 2)
        f.add_kernel(Kernel((bool_, bool_), _exec_kleene(code), bool_))
        reg.add_function(f)
    f = Function("invert", Function.SCALAR, 1)
    f.add_kernel(Kernel((bool_,), _exec_invert, bool_))
    reg.add_function(f)

    f = Function("array_sort_indices", Function.VECTOR, 1, ArraySortOptions())
    for key_type in (uint64, int64, uint32, int32, float64, float32):
        f.add_kernel(Kernel((key_type,), _exec_array_sort_indices, uint64))
    f.add_kernel(Kernel((bool_,), _exec_array_sort_indices_bool, uint64))
    reg.add_function(f)
    reg.add_function(Function("sort_indices", Function.META, 1, SortOptions(), _sort_indices_meta))

    for name in _MATCH_OPS:
        f = Function(name, Function.SCALAR, 1, MatchSubstringOptions())
        f.add_kernel(Kernel((_BASE_BINARY,), _exec_match_substring(name), bool_))
        reg.add_function(f)

    # lengths and slices of utf8 / binary rows (csrc/string_slice.hip)
    for name in ("binary_length", "utf8_length"):
        f = Function(name, Function.SCALAR, 1)
        f.add_kernel(Kernel((_STRING_INPUT[name],), _exec_string_length(name), int32))
        reg.add_function(f)
    for name in ("binary_slice", "utf8_slice_codeunits"):
        f = Function(name, Function.SCALAR, 1, SliceOptions())
        f.add_kernel(Kernel((_STRING_INPUT[name],), _exec_string_slice(name)))
        reg.add_function(f)
    # replace_substring of utf8 / binary rows (csrc/string_replace.hip)
    f = Function("replace_substring", Function.SCALAR, 1)
    for t in (type_from_name("string"), type_from_name("binary")):
        f.add_kernel(Kernel((t,), _exec_replace_substring))
    reg.add_function(f)
    # binary_join_element_wise(v_1, ..., v_k, separator) of utf8 / binary operands of one type (csrc/string_join.hip)
    f = Function("binary_join_element_wise", Function.SCALAR, 1, JoinOptions(), is_varargs=True)
    for t in (type_from_name("string"), type_from_name("binary")):
        f.add_kernel(Kernel((t,), _exec_binary_join_element_wise, t, is_varargs=True))
    reg.add_function(f)
    # the twelve trims of utf8 rows (csrc/string_trim.hip)
    for name in _TRIMS:
        f = Function(name, Function.SCALAR, 1)
        f.add_kernel(Kernel((_UTF8_ONLY,), _exec_string_trim(name)))
        reg.add_function(f)

    # if_else(cond, left, right): left / right of ONE type, boolean or 1 / 2 / 4 / 8 bytes wide (csrc/if_else.hip)
    f = Function("if_else", Function.SCALAR, 3)
    f.add_kernel(Kernel((bool_, _IF_ELSE_VALUE, _IF_ELSE_VALUE), _exec_if_else))
    reg.add_function(f)

    # case_when(conds, v_0 .. v_{k-1} [, else]): values of ONE type, as if_else takes them (csrc/case_when.hip).  conds is a
    # list of boolean Arrays (or a StructArray of them), not a typed argument: the function checks its arguments itself.
    reg.add_function(Function("case_when", Function.META, 2, None, lambda args, options: case_when(args[0], *args[1:]), is_varargs=True))
    # min_element_wise / max_element_wise of 1 .. 32 operands of ONE numeric or physically-integer temporal type (csrc/element_wise.hip)
    for name in _ELEMENT_WISE_OPS:
        f = Function(name, Function.SCALAR, 1, ElementWiseAggregateOptions(), is_varargs=True)
        f.add_kernel(Kernel((_ELEMENT_WISE_VALUE,), _exec_min_max_element_wise(name), is_varargs=True))
        reg.add_function(f)

    # year .. iso_week of dates and timestamps, hour .. nanosecond of timestamps and times (csrc/temporal.hip)
    for name in _TEMPORAL_COMPONENTS:
        f = Function(name, Function.SCALAR, 1, DayOfWeekOptions() if name == "day_of_week" else None)
        f.add_kernel(Kernel((_temporal_input(name),), _exec_temporal(name), int64))
        reg.add_function(f)

    # negate .. trunc, round and round_to_multiple of the numeric types (csrc/unary_arith.hip)
    for name in _UNARY_OPS:
        f = Function(name, Function.SCALAR, 1)
        for t in numeric_types:
            if _unary_input(name)(t):
                f.add_kernel(Kernel((t,), _exec_unary_arith(name), int8 if name == "sign" and not _FLOATING(t) else t))
        reg.add_function(f)
    for name, default in (("round", RoundOptions()), ("round_to_multiple", RoundToMultipleOptions())):
        f = Function(name, Function.SCALAR, 1, default)
        for t in numeric_types:
            f.add_kernel(Kernel((t,), _exec_round(name), t))
        reg.add_function(f)

    f = Function("hash_sum", Function.HASH_AGGREGATE, 2, ScalarAggregateOptions())
    f.add_kernel(HashAggregateKernel((int64, uint32), _hash_sum_init, _hash_sum_resize,
                                     _hash_sum_consume, _hash_sum_merge, _hash_sum_finalize, int64))
    reg.add_function(f)
    return reg


_registry = None


def get_function_registry() -> FunctionRegistry:
    """GetFunctionRegistry (registry.cc:301-304): the process-wide singleton."""
    global _registry
    if _registry is None:
        _registry = _build_registry()
    return _registry


def call_function(name: str, args, options=None, registry: FunctionRegistry | None = None):
    """CallFunction (exec.cc:1362-1370): registry lookup + Function::Execute."""
    reg = registry or get_function_registry()
    return reg.get_function(name).execute(list(args), options)


# --------------------------------------------------------------------------- typed wrappers
def filter(values, mask, null_selection_behavior: str = "drop"):  # noqa: A001
    """compute::Filter (api_vector.cc:412-416)."""
    return call_function("filter", [values, mask], FilterOptions(null_selection_behavior))


def take(values, indices, boundscheck: bool = True):
    """compute::Take (api_vector.cc:419-423)."""
    return call_function("take", [values, indices], TakeOptions(boundscheck))


def cast(arr, to_type: DataType, safe: bool = True):
    """compute::Cast (cast.cc:239-248); safe=False = CastOptions::Unsafe."""
    return call_function("cast", [arr], CastOptions(to_type, allow_float_truncate=not safe, allow_int_overflow=not safe))


def _wrap_scalar(x, like: Array):
    if isinstance(x, (Array, Scalar)):
        return x
    return Scalar(x, like.type, x is not None)


def greater(left, right):
    like = left if isinstance(left, Array) else right
    left, right = _wrap_scalar(left, like), _wrap_scalar(right, like)
    return call_function("greater", [left, right])


def _compare_wrapper(name):
    def fn(left, right):
        like = left if isinstance(left, Array) else right
        return call_function(name, [_wrap_scalar(left, like), _wrap_scalar(right, like)])
    fn.__name__ = name
    fn.__doc__ = f"compute::CallFunction(\"{name}\") (scalar_compare.cc:391-445)."
    return fn


equal, not_equal, greater_equal, less, less_equal = (_compare_wrapper(n) for n in
                                                     ("equal", "not_equal", "greater_equal", "less", "less_equal"))
subtract, multiply, add_checked, subtract_checked, multiply_checked = (
    _compare_wrapper(n) for n in ("subtract", "multiply", "add_checked", "subtract_checked", "multiply_checked"))
divide, divide_checked = (_compare_wrapper(n) for n in ("divide", "divide_checked"))


def add(left, right):
    like = left if isinstance(left, Array) else right
    left, right = _wrap_scalar(left, like), _wrap_scalar(right, like)
    return call_function("add", [left, right])


def and_kleene(left, right):
    return call_function("and_kleene", [left, right])


def or_kleene(left, right):
    return call_function("or_kleene", [left, right])


def invert(arr):
    return call_function("invert", [arr])


def sort_indices(arr, order: str = "ascending", null_placement: str = "at_end"):
    """compute::SortIndices (api_vector.cc:334-347)."""
    return call_function("sort_indices", [arr], SortOptions([("", order)], null_placement))


def concat_arrays(arrays) -> Array:
    """arrow::Concatenate (array/concatenate.cc: ConcatenateBitmaps, ConcatenateBuffers, PutOffsets) for
    fixed-width, boolean and utf8/binary arrays: one output array, chunks glued at arbitrary bit positions.
    What an operator that must see its whole input does first (OrderByNode, acero/order_by_node.cc:100-108)."""
    arrays = list(arrays)
    if not arrays:
        raise ArrowInvalid("Must pass at least one array")
    t = arrays[0].type
    if any(a.type != t for a in arrays):
        raise ArrowInvalid("arrays to be concatenated must be identically typed")
    dev = arrays[0].device
    lib, stream = _lib_and_stream(dev)
    n = builtins.sum(a.length for a in arrays)
    have_validity = any(a.validity is not None and a.null_count != 0 for a in arrays)
    out_valid = alloc(bitmap_nbytes(n), dev, zero=True) if have_validity else None
    pos = 0
    if have_validity:
        for a in arrays:
            check(lib.arx_bitmap_copy_at((a.validity.data_ptr() if a.validity is not None and a.null_count != 0 else None), a.offset, a.length,
                                         out_valid.data_ptr(), pos, stream))
            pos += a.length
    if is_base_binary(t):
        # (two offsets per chunk come back to the host: where its bytes start and end)
        ends = [a.buffers[1].view(torch.int32)[[a.offset, a.offset + a.length]].cpu().tolist() if a.length else [0, 0]
                for a in arrays]
        total = builtins.sum(e - b for b, e in ends)
        if total > 2**31 - 1:
            raise ArrowInvalid("offset overflow while concatenating arrays")
        out_off = alloc((n + 1) * 4, dev, zero=True)
        out_data = alloc(total, dev)
        pos, base = 0, 0
        for a, (b, e) in zip(arrays, ends):
            if a.length == 0:
                continue
            check(lib.arx_binary_rebase_offsets(a.buffers[1].data_ptr() + a.offset * 4, a.length, base,
                                                out_off.data_ptr() + pos * 4, stream))
            if e > b:
                out_data[base:base + e - b].copy_(a.buffers[2][b:e])
            pos += a.length
            base += e - b
        out = Array(t, n, [out_valid, out_off, out_data], kUnknownNullCount if have_validity else 0, 0)
    elif t == bool_:
        out_bits = alloc(bitmap_nbytes(n), dev, zero=True)
        pos = 0
        for a in arrays:
            check(lib.arx_bitmap_copy_at(a.data.data_ptr(), a.offset, a.length, out_bits.data_ptr(), pos, stream))
            pos += a.length
        out = Array(t, n, [out_valid, out_bits], kUnknownNullCount if have_validity else 0, 0)
    else:
        w = t.byte_width
        out_data = alloc(n * w, dev)
        pos = 0
        for a in arrays:
            out_data[pos * w:(pos + a.length) * w].copy_(a.data[a.offset * w:(a.offset + a.length) * w])
            pos += a.length
        out = Array(t, n, [out_valid, out_data], kUnknownNullCount if have_validity else 0, 0)
    if have_validity:
        known = [a.null_count for a in arrays]
        if all(k >= 0 for k in known):
            out._null_count = builtins.sum(known)
    return out


def sort_indices_by_keys(keys, orders=None, null_placement="at_end") -> Array:
    """SortIndices(Table, SortOptions) for several sort keys (TableSorter / MultipleKeyRecordBatchSorter,
    kernels/vector_sort.cc:850-954): lexicographic, stable, every key with its own order and its own null
    placement (SortKey::null_placement, compute/ordering.h:50-61; one string = the SortOptions-wide override,
    api_vector.h:132-143).  Least-significant key first, one stable device sort per key: perm = sort(k_last);
    then perm = take(perm, sort(take(k, perm))) for each earlier key."""
    keys = list(keys)
    orders = list(orders) if orders is not None else ["ascending"] * len(keys)
    places = [null_placement] * len(keys) if isinstance(null_placement, str) else list(null_placement)
    if not keys or len(keys) != len(orders) or len(keys) != len(places):
        raise ArrowInvalid("Must specify one or more sort keys")
    perm = None
    for key, order, place in zip(reversed(keys), reversed(orders), reversed(places)):
        opts = ArraySortOptions(order, place)
        if perm is None:
            perm = call_function("array_sort_indices", [key], opts)
        else:
            step = call_function("array_sort_indices", [take(key, perm, boundscheck=False)], opts)
            perm = take(perm, step, boundscheck=False)
    return perm


# RankOptions::Tiebreaker (api_vector.h:201-212) = ARX_RANK_* of include/arrow_amd.h; "quantile": rank_quantile, "normal":
# rank_normal
_RANK_TIEBREAKER = {"min": 0, "max": 1, "first": 2, "dense": 3, "quantile": 4, "normal": 5}


def _rank(arr: Array, order: str, null_placement: str, tiebreaker: str) -> Array:
    """RankMetaFunctionBase::Rank (kernels/vector_rank.cc:386-420): sort the indices with the array sorter, then one
    walk of the sorted order (arx_rank)."""
    if arr.type.name not in _SORT_KEY_TYPE:
        raise ArrowNotImplementedError(f"rank: {arr.type.name} values")
    if tiebreaker not in _RANK_TIEBREAKER:
        raise ArrowInvalid(f"rank: tiebreaker {tiebreaker!r}")
    dev = arr.device
    lib, stream = _lib_and_stream(dev)
    n = arr.length
    sorted_rows = call_function("array_sort_indices", [arr], ArraySortOptions(order, null_placement))
    out = alloc(n * 8, dev)
    ws_bytes = lib.arx_rank_workspace_bytes(n)
    ws = _workspace(dev, ws_bytes + 256, "rank")
    base = ws.data_ptr()
    aligned = (base + 255) & ~255
    span = arr.span()
    check(lib.arx_rank(C.byref(span), _SORT_KEY_TYPE[arr.type.name], sorted_rows.data.data_ptr(), _RANK_TIEBREAKER[tiebreaker],
                       aligned, ws.numel() - (aligned - base), out.data_ptr(), stream))
    return Array(float64 if tiebreaker in ("quantile", "normal") else uint64, n, [None, out], 0, 0)


def rank(arr: Array, order: str = "ascending", null_placement: str = "at_end", tiebreaker: str = "first") -> Array:
    """compute "rank" (RankMetaFunction, kernels/vector_rank.cc:422-441; RankOptions api_vector.h:195-240): 1-based uint64
    ranks, never null; nulls and NaNs are ranked where the sort puts them, all nulls tie, all NaNs tie."""
    return _rank(arr, order, null_placement, tiebreaker)


def rank_quantile(arr: Array, order: str = "ascending", null_placement: str = "at_end") -> Array:
    """compute "rank_quantile" (RankQuantileMetaFunction, kernels/vector_rank.cc:443-462): (rows below the row's run of
    ties + half the run) / length, float64."""
    return _rank(arr, order, null_placement, "quantile")


def rank_normal(arr: Array, order: str = "ascending", null_placement: str = "at_end") -> Array:
    """compute "rank_normal" (RankNormalMetaFunction, kernels/vector_rank.cc:424-441): the normal percent-point function
    (NormalPPF, util/math_internal.cc:26-137 — Wichura's AS 241) of the quantile rank, float64."""
    return _rank(arr, order, null_placement, "normal")


def partition_nth_indices(arr: Array, pivot: int, null_placement: str = "at_end") -> Array:
    """compute "partition_nth_indices" (PartitionNthToIndices, kernels/vector_array_sort.cc:56-95): uint64 indices such
    that the `pivot` first ones point at values no greater than the others; nulls and NaNs at the chosen end.  The
    reference runs std::nth_element (any valid partition is a right answer); a full sort is one such partition."""
    if pivot > arr.length:
        raise ArrowIndexError("NthToIndices index out of bound")
    return call_function("array_sort_indices", [arr], ArraySortOptions("ascending", null_placement))


# select_k by a THRESHOLD instead of a sort (round 6): rows below which row counts the fast path is not tried, the largest
# k / n it is tried for, and the largest share of the rows the candidates may be before the sort is the better plan
SELECT_K_MIN_ROWS = 1 << 22
SELECT_K_MAX_SHARE = 16
_SELECT_COUNTERS = {"threshold": 0, "sorted": 0}


def _select_k_by_threshold(arr: Array, k: int, order: str, null_placement: str):
    """The first k rows of the sort order WITHOUT sorting the column (uint64 / int64 keys, k much smaller than the
    column, every selected row a non-null): one pass for a 4096-bin histogram of the keys over their (sampled, widened)
    range — the pieces the sharded sort places its splitters with —, the bin in which the k-th smallest key falls, ONE
    comparison of the column against that bin's upper edge (`less_equal` / `greater_equal`: a bitmap), GetTakeIndices
    of the bitmap (the candidates' rows, ascending), and the sort of the candidates' keys alone.  The candidates are
    exactly the rows whose bin is at most that bin (the bin is monotone in the key, keys outside the sampled range
    included: they saturate into the end bins), they come in row order and the sort is stable, so the result is INDEX
    for index the head of the full stable sort.  ~3 passes over 8-byte keys instead of the sort's 51 B/row.
    None: not this case (the caller sorts)."""
    from .array import int64 as i64, uint64 as u64

    n = arr.length
    if arr.type not in (i64, u64) or n < SELECT_K_MIN_ROWS or n > 0xFFFFFFFF or k <= 0 or k * SELECT_K_MAX_SHARE > n:
        return None
    nulls = arr.null_count if (arr.buffers[0] is not None) else 0
    if nulls and (null_placement == "at_start" or k > n - nulls):
        return None
    dev = arr.device
    lib, stream = _lib_and_stream(dev)
    span = arr.span()
    is_signed = int(arr.type == i64)
    order_code = _lib.SORT_DESCENDING if order == "descending" else _lib.SORT_ASCENDING
    key_range = torch.zeros(2, dtype=torch.int64, device=dev)
    check(lib.arx_sort_key_range_sampled(C.byref(span), is_signed, order_code, 4, key_range.data_ptr(), stream))
    mask64 = (1 << 64) - 1
    inv_min, key_max = [int(x) & mask64 for x in key_range.tolist()]
    key_min = ~inv_min & mask64
    if key_max <= key_min:
        return None
    margin = ((key_max - key_min) >> 6) + 1
    key_min, key_max = max(0, key_min - margin), min(mask64, key_max + margin)
    shift = 64 - (key_max - key_min).bit_length()
    window = _lib.ArxSortKeyWindow(key_min, shift, 0)
    bits = 12
    hist = torch.zeros(1 << bits, dtype=torch.int64, device=dev)
    check(lib.arx_sort_key_histogram_window(C.byref(span), is_signed, order_code, bits, C.byref(window), hist.data_ptr(), stream))
    cum = torch.cumsum(hist.cpu(), 0)
    b = int(torch.searchsorted(cum, torch.tensor(k, dtype=cum.dtype)).item())
    if b >= (1 << bits) - 1 or int(cum[b]) * 4 > n:      # the last bin (open above), or a bin that holds a fifth of the column
        return None
    edge = key_min + ((((b + 1) << (64 - bits)) - 1) >> shift)      # the largest transformed key whose bin is at most b
    if edge >= mask64:
        return None
    # transformed key -> the column's value: descending sorts ~key, signed keys have their sign bit flipped
    raw = edge ^ mask64 if order == "descending" else edge
    if is_signed:
        raw ^= 1 << 63
        raw = raw - (1 << 64) if raw >= (1 << 63) else raw
    bound = Scalar(raw, arr.type, True)
    mask = call_function("greater_equal" if order == "descending" else "less_equal", [arr, bound])
    rows = get_take_indices(mask)               # nulls dropped; ascending row numbers
    if rows.length != int(cum[b]):
        raise ArrowInvalid(f"select_k_unstable: {rows.length} candidates, the histogram promised {int(cum[b])}")
    cand = take(arr, rows, boundscheck=False)
    perm = call_function("array_sort_indices", [cand], ArraySortOptions(order, "at_end"))
    head = Array(uint64, k, [None, perm.data[: k * 8]], 0, 0)
    picked = take(rows, head, boundscheck=False)
    _SELECT_COUNTERS["threshold"] += 1
    return picked if picked.type == uint64 else cast(picked, uint64)


def select_k_unstable(arr: Array, k: int, order: str = "ascending", null_placement: str = "at_end") -> Array:
    """compute "select_k_unstable" on an array (ArraySelector, kernels/vector_select_k.cc:156-232): the indices of the
    first k rows of the sorted order — non-nulls, NaNs, nulls taken in that sequence (or the reverse, at_start:
    CalculateOutputRangesByNullLikeness, :82-100).  "Unstable": the order of equal values is not promised; this one
    keeps them in row order."""
    if k < 0:
        raise ArrowInvalid("select_k_unstable requires a nonnegative `k`, got " + str(k))
    fast = _select_k_by_threshold(arr, k, order, null_placement)
    if fast is not None:
        return fast
    _SELECT_COUNTERS["sorted"] += 1
    perm = call_function("array_sort_indices", [arr], ArraySortOptions(order, null_placement))
    k = min(k, arr.length)
    return Array(uint64, k, [None, perm.data[: k * 8]], 0, 0)


def order_by(columns, sort_keys, null_placement="at_end"):
    """OrderByNode::DoFinish (acero/order_by_node.cc:100-108): concatenate the accumulated batches,
    SortIndices on the sort keys, Take on every column.  `columns` = list of columns, each a list of chunks;
    `sort_keys` = [(column index, "ascending" | "descending")]."""
    whole = [concat_arrays(chunks) if len(chunks) != 1 or chunks[0].offset != 0 else chunks[0] for chunks in columns]
    perm = sort_indices_by_keys([whole[i] for i, _ in sort_keys], [o for _, o in sort_keys], null_placement)
    return [take(col, perm, boundscheck=False) for col in whole]


# --------------------------------------------------------------------------- group-by
# --------------------------------------------------------------------------- scalar aggregates (int64)
class Int64Aggregator:
    """SumImpl / CountImpl / MinMaxImpl over int64 batches (aggregate_basic.inc.cc:49-110,776-860):
    consume() any number of device arrays, then sum() / count() / min_max() apply the options the
    way Finalize does.  (mean is not offered: the reference accumulates it in doubles, in row order.)"""

    def __init__(self, device=None, options: ScalarAggregateOptions | None = None):
        from .array import default_device

        self.device = torch.device(device) if device is not None else default_device()
        self.options = options or ScalarAggregateOptions()
        self.acc = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.rows = 0
        self.nulls_observed = False
        lib, stream = _lib_and_stream(self.device)
        check(lib.arx_reduce_i64_init(self.acc.data_ptr(), stream))

    def consume(self, arr: Array) -> None:
        if arr.type != int64:
            raise ArrowNotImplementedError("Int64Aggregator: int64 values only")
        lib, stream = _lib_and_stream(self.device)
        sp = arr.span()
        check(lib.arx_reduce_i64_consume(C.byref(sp), self.acc.data_ptr(), stream))
        self.rows += arr.length

    def _state(self):
        s, c, mn, mx = (int(x) for x in self.acc.cpu().tolist())
        return s, c, mn, mx

    def sum(self):
        s, c, _, _ = self._state()
        nulls = c < self.rows
        if (not self.options.skip_nulls and nulls) or c < self.options.min_count:
            return None
        return s

    def count(self, mode: str = "only_valid"):
        _, c, _, _ = self._state()
        return {"only_valid": c, "only_null": self.rows - c, "all": self.rows}[mode]

    def min_max(self):
        _, c, mn, mx = self._state()
        nulls = c < self.rows
        if (not self.options.skip_nulls and nulls) or c < max(1, self.options.min_count):
            return None
        return mn, mx


def sum(arr: Array, skip_nulls: bool = True, min_count: int = 1):  # noqa: A001
    """compute::Sum for int64 (wrap-around), None = null."""
    agg = Int64Aggregator(arr.device, ScalarAggregateOptions(skip_nulls, min_count))
    agg.consume(arr)
    return agg.sum()


def count(arr: Array, mode: str = "only_valid") -> int:
    agg = Int64Aggregator(arr.device)
    agg.consume(arr)
    return agg.count(mode)


def min_max(arr: Array, skip_nulls: bool = True, min_count: int = 1):
    agg = Int64Aggregator(arr.device, ScalarAggregateOptions(skip_nulls, min_count))
    agg.consume(arr)
    return agg.min_max()


def _next_pow2(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


class GroupBySum:
    """The fused device operator standing where Acero's GroupByNode drives
    Grouper::Consume + hash_sum {resize, consume, merge, finalize}
    (acero/groupby_aggregate_node.cc:210-337, compute/kernel.h:720-769).

    capacity: slots of the open-addressing table (power of two, > expected distinct keys).
    """

    def __init__(self, capacity: int, device=None, options: ScalarAggregateOptions | None = None):
        from .array import default_device

        self.device = torch.device(device) if device is not None else default_device()
        self.capacity = _next_pow2(max(2, int(capacity)))
        self.options = options or ScalarAggregateOptions()
        lib, stream = _lib_and_stream(self.device)
        self.state = alloc(lib.arx_groupby_state_bytes(self.capacity), self.device)
        check(lib.arx_groupby_init(self.state.data_ptr(), self.capacity, stream))

    # ---- key / value types beyond (int32, int64): what the reference registers (Grouper key types,
    # row/grouper.cc:559-611; hash_sum value types, hash_aggregate_numeric.cc:1188-1200) mapped onto the one device
    # table by width-changing casts that are bijections on the values present
    _KEY32_SIGNED = ("int8", "int16", "int32", "date32[day]", "time32[s]", "time32[ms]")
    _KEY32_UNSIGNED = ("uint8", "uint16", "uint32")

    def _normalise_key(self, keys: Array) -> Array:
        name = keys.type.name
        prev = getattr(self, "key_type", None)
        if prev is not None and prev != keys.type:
            raise ArrowInvalid(f"GroupBySum: key type changed from {prev.name} to {name}")
        self.key_type = keys.type
        if keys.type == int32:
            return keys
        if name in ("uint32", "date32[day]", "time32[s]", "time32[ms]"):
            return Array(int32, keys.length, keys.buffers, keys.null_count, keys.offset)      # same bits, same equality
        if name in ("int8", "int16", "uint8", "uint16"):
            return cast(keys, int32)                                                          # value-preserving widening
        if keys.type.bit_width == 64 and keys.type.name != "double":
            # 64-bit integer / temporal keys: the device table holds 32-bit keys, so they are accepted when every
            # valid key fits (a checked cast: the first one that does not names the error), declined otherwise
            try:
                if name == "uint64":
                    return cast(keys, int32)
                as_i64 = keys if keys.type == int64 else Array(int64, keys.length, keys.buffers, keys.null_count, keys.offset)
                return cast(as_i64, int32)
            except ArrowInvalid as e:
                raise ArrowNotImplementedError(f"GroupBySum: {name} keys beyond the int32 range are not implemented "
                                               f"(the device table holds 32-bit keys): {e}") from None
        raise ArrowNotImplementedError(f"GroupBySum: keys of type {name}")

    def _typed_keys(self, keys_i32: torch.Tensor) -> torch.Tensor:
        """The table's int32 keys in the CALLER's key type: the bit-reinterpreted 32-bit types get their own
        view back (uint32 >= 2^31 would read as negative), the widened narrow integers are narrowed again (every value
        fits: it came from that type), 64-bit keys that passed the checked cast are widened.  Temporal 32-bit types
        keep their physical int32 values (days / seconds / milliseconds), 64-bit temporal types int64."""
        kt = getattr(self, "key_type", None)
        if kt is None or kt == int32:
            return keys_i32
        name = kt.name
        if name == "uint32":
            return keys_i32.view(torch.uint32)
        if name in ("date32[day]", "time32[s]", "time32[ms]"):
            return keys_i32
        narrow = {"int8": torch.int8, "int16": torch.int16, "uint8": torch.uint8, "uint16": torch.uint16}
        if name in narrow:
            return keys_i32.to(narrow[name])
        if name == "uint64":
            return keys_i32.to(torch.int64).view(torch.uint64)      # (non-negative: it passed the checked cast)
        return keys_i32.to(torch.int64)

    def _normalise_value(self, values: Array) -> Array:
        name = values.type.name
        prev = getattr(self, "value_type", None)
        if prev is not None and prev != values.type:
            raise ArrowInvalid(f"GroupBySum: value type changed from {prev.name} to {name}")
        self.value_type = values.type
        if values.type == int64:
            return values
        if name == "uint64":      # the accumulator of unsigned inputs is UInt64 (FindAccumulatorType): same wrap-around bits
            return Array(int64, values.length, values.buffers, values.null_count, values.offset)
        if name in ("int8", "int16", "int32"):
            return cast(values, int64)
        if name in ("uint8", "uint16", "uint32"):
            w = cast(values, uint64)
            return Array(int64, w.length, w.buffers, w.null_count, w.offset)
        if name in ("float", "double"):
            raise ArrowNotImplementedError(
                f"GroupBySum: hash_sum({name}) accumulates doubles in row order in the reference "
                "(hash_aggregate_numeric.cc:70-83), which a parallel reduction cannot reproduce bit for bit")
        raise ArrowNotImplementedError(f"GroupBySum: values of type {name}")

    @property
    def sum_type(self) -> DataType:
        """Output type of hash_sum for the consumed value type (FindAccumulatorType, aggregate_internal.h:41-44)."""
        vt = getattr(self, "value_type", int64)
        return uint64 if vt.name.startswith("uint") else int64

    def consume(self, keys: Array, values: Array) -> None:
        keys, values = self._normalise_key(keys), self._normalise_value(values)
        lib, stream = _lib_and_stream(self.device)
        ks, vs = keys.span(), values.span()
        ws_bytes = lib.arx_groupby_consume_workspace_bytes(keys.length, self.capacity)
        ws_ptr, ws_len = None, 0
        if ws_bytes:
            ws = _workspace(self.device, ws_bytes + 256, "groupby")
            ws_ptr = (ws.data_ptr() + 255) & ~255
            ws_len = ws.numel() - (ws_ptr - ws.data_ptr())
        check(lib.arx_groupby_sum_i64_consume(self.state.data_ptr(), self.capacity, C.byref(ks),
                                              C.byref(vs), ws_ptr, ws_len, stream))

    # -- hash_min / hash_max on the same table (GroupedMinMaxImpl, kernels/hash_aggregate.cc:330-419)
    def consume_min_max(self, keys: Array, values: Array) -> None:
        """Folds the rows into per-group extrema; does not touch the sums, so the same rows may also
        go through consume()."""
        keys = self._normalise_key(keys)
        if values.type != int64:
            raise ArrowNotImplementedError("GroupBySum: hash_min / hash_max over int64 values only")
        lib, stream = _lib_and_stream(self.device)
        if getattr(self, "minmax", None) is None:
            self.minmax = alloc(lib.arx_groupby_minmax_bytes(self.capacity), self.device)
            check(lib.arx_groupby_minmax_init(self.minmax.data_ptr(), self.capacity, stream))
        ks, vs = keys.span(), values.span()
        check(lib.arx_groupby_minmax_i64_consume(self.state.data_ptr(), self.minmax.data_ptr(), self.capacity,
                                                 C.byref(ks), C.byref(vs), stream))

    def export_min_max(self):
        """Partial extrema: dict keys / key_is_valid / mins / maxs / no_nulls (device tensors)."""
        lib, stream = _lib_and_stream(self.device)
        g = self.num_groups()
        dev = self.device
        t = lambda dt: torch.empty(max(g, 1), dtype=dt, device=dev)  # noqa: E731
        cols = dict(keys=t(torch.int32), key_is_valid=t(torch.uint8), sums=t(torch.int64), counts=t(torch.int64),
                    no_nulls=t(torch.uint8), mins=t(torch.int64), maxs=t(torch.int64))
        check(lib.arx_groupby_export(self.state.data_ptr(), self.minmax.data_ptr(), cols["keys"].data_ptr(),
                                     cols["key_is_valid"].data_ptr(), cols["sums"].data_ptr(),
                                     cols["counts"].data_ptr(), cols["no_nulls"].data_ptr(),
                                     cols["mins"].data_ptr(), cols["maxs"].data_ptr(), stream))
        return {k: v[:g] for k, v in cols.items()}

    def merge_min_max(self, partial: dict) -> None:
        """Merge of GroupedMinMaxImpl (hash_aggregate.cc:371-399) from export_min_max() of another state."""
        lib, stream = _lib_and_stream(self.device)
        if getattr(self, "minmax", None) is None:
            self.minmax = alloc(lib.arx_groupby_minmax_bytes(self.capacity), self.device)
            check(lib.arx_groupby_minmax_init(self.minmax.data_ptr(), self.capacity, stream))
        g = int(partial["keys"].numel())
        if g == 0:
            return
        check(lib.arx_groupby_minmax_merge(self.state.data_ptr(), self.minmax.data_ptr(), self.capacity,
                                           partial["keys"].data_ptr(), partial["key_is_valid"].data_ptr(),
                                           partial["mins"].data_ptr(), partial["maxs"].data_ptr(),
                                           partial["no_nulls"].data_ptr(), g, stream))

    def finalize_min_max(self):
        """Returns (keys, key_is_valid, mins, maxs, valid) device tensors, `valid` by the options'
        skip_nulls (min_count is not consulted by the reference's min/max)."""
        lib, stream = _lib_and_stream(self.device)
        if getattr(self, "minmax", None) is None:
            raise ArrowInvalid("finalize_min_max without consume_min_max")
        g = self.num_groups()
        dev = self.device
        t = lambda dt: torch.empty(max(g, 1), dtype=dt, device=dev)  # noqa: E731
        keys, kv, sums, counts, nn = t(torch.int32), t(torch.uint8), t(torch.int64), t(torch.int64), t(torch.uint8)
        mins, maxs, valid = t(torch.int64), t(torch.int64), t(torch.uint8)
        check(lib.arx_groupby_export(self.state.data_ptr(), self.minmax.data_ptr(), keys.data_ptr(), kv.data_ptr(),
                                     sums.data_ptr(), counts.data_ptr(), nn.data_ptr(), mins.data_ptr(),
                                     maxs.data_ptr(), stream))
        check(lib.arx_groupby_minmax_finalize(mins.data_ptr(), maxs.data_ptr(), nn.data_ptr(), g,
                                              int(self.options.skip_nulls), valid.data_ptr(), stream))
        return self._typed_keys(keys[:g]), kv[:g], mins[:g], maxs[:g], valid[:g]

    def finalize_mean(self):
        """hash_mean(int64): (keys, key_is_valid, means f64, valid).  Needs the rows in BOTH consume() and
        consume_min_max() (the extrema bound the partial sums).  GroupedMeanImpl sums doubles in row order
        (hash_aggregate_numeric.cc:352-430); that equals (double)sum / count in any order exactly when every
        partial sum is an exact integer, i.e. count * max|value| < 2^53 for every group — otherwise the
        reference's own result depends on row order and this declines."""
        lib, stream = _lib_and_stream(self.device)
        if getattr(self, "minmax", None) is None:
            raise ArrowInvalid("finalize_mean without consume_min_max")
        p = self.export_min_max()
        g = int(p["keys"].numel())
        means = torch.empty(max(g, 1), dtype=torch.float64, device=self.device)
        valid = torch.empty(max(g, 1), dtype=torch.uint8, device=self.device)
        inexact = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(lib.arx_groupby_mean_i64_finalize(p["sums"].data_ptr(), p["counts"].data_ptr(), p["mins"].data_ptr(),
                                                p["maxs"].data_ptr(), p["no_nulls"].data_ptr(), g,
                                                int(self.options.skip_nulls), self.options.min_count,
                                                means.data_ptr(), valid.data_ptr(), inexact.data_ptr(), stream))
        if int(inexact.item()) != 0:
            raise ArrowNotImplementedError(
                "hash_mean(int64): a group's partial sums exceed 2^53, where the reference's row-order double "
                "accumulation is not associative (its result depends on row order); not reproducible bit for bit")
        return self._typed_keys(p["keys"]), p["key_is_valid"], means[:g], valid[:g]

    def num_groups(self) -> int:
        lib, stream = _lib_and_stream(self.device)
        n = C.c_int64(0)
        check(lib.arx_groupby_num_groups(self.state.data_ptr(), C.byref(n), stream))
        return n.value

    def export(self):
        """Partial aggregates: dict of device tensors keys(i32) key_is_valid(u8) sums(i64)
        counts(i64) no_nulls(u8), num_groups entries each, unspecified order."""
        lib, stream = _lib_and_stream(self.device)
        g = self.num_groups()
        dev = self.device
        cols = dict(keys=torch.empty(max(g, 1), dtype=torch.int32, device=dev),
                    key_is_valid=torch.empty(max(g, 1), dtype=torch.uint8, device=dev),
                    sums=torch.empty(max(g, 1), dtype=torch.int64, device=dev),
                    counts=torch.empty(max(g, 1), dtype=torch.int64, device=dev),
                    no_nulls=torch.empty(max(g, 1), dtype=torch.uint8, device=dev))
        check(lib.arx_groupby_sum_i64_export(self.state.data_ptr(), cols["keys"].data_ptr(),
                                             cols["key_is_valid"].data_ptr(), cols["sums"].data_ptr(),
                                             cols["counts"].data_ptr(), cols["no_nulls"].data_ptr(),
                                             stream))
        return {k: v[:g] for k, v in cols.items()}

    def merge(self, partial: dict) -> None:
        """Fold another state's partial aggregates in (Merge, hash_aggregate_numeric.cc:85-107)."""
        lib, stream = _lib_and_stream(self.device)
        g = int(partial["keys"].numel())
        if g == 0:
            return
        check(lib.arx_groupby_sum_i64_merge(self.state.data_ptr(), self.capacity,
                                            partial["keys"].data_ptr(), partial["key_is_valid"].data_ptr(),
                                            partial["sums"].data_ptr(), partial["counts"].data_ptr(),
                                            partial["no_nulls"].data_ptr(), g, stream))

    def finalize(self):
        """Returns (keys, key_is_valid, sums, valid) device tensors (valid: u8, 0 = null sum)."""
        lib, stream = _lib_and_stream(self.device)
        p = self.export()
        g = int(p["keys"].numel())
        valid = torch.empty(max(g, 1), dtype=torch.uint8, device=self.device)
        check(lib.arx_groupby_sum_i64_finalize(p["counts"].data_ptr(), p["no_nulls"].data_ptr(), g,
                                               int(self.options.skip_nulls), self.options.min_count,
                                               valid.data_ptr(), stream))
        return self._typed_keys(p["keys"]), p["key_is_valid"], p["sums"], valid[:g]


class RangeGroupBySum:
    """hash_sum(int64) BY int32 for keys from a narrow range, on the RANGE-PARTITIONED state of include/arrow_amd.h
    (arx_groupby_range_*; csrc/groupby_lines.h): no hash table — `partitions` dense blocks of `width` keys each,
    {uint64 sums[width] | uint64 counts[width]}.  The same operator as GroupBySum (ThreadLocalState -> Merge -> Finalize,
    acero/groupby_aggregate_node.cc:210-337; hash_aggregate_numeric.cc:44-187); rows with nulls, keys outside the
    planned range and hot keys are declined (consume returns False, nothing consumed) and go through GroupBySum."""

    SAMPLE_ROWS = 1 << 20
    MIN_ROWS = 1 << 22      # below this group_by_sum / sharded_group_by_sum do not try the state (the table operator's plans)

    @staticmethod
    def sampled_key_range(keys: Array, sample_rows: int | None = None) -> torch.Tensor:
        """Device int64[2] = {-min, max} of a sample of the key slots ({-INT32_MAX, INT32_MIN} for no rows): both fold
        over ranks with ONE all-reduce(MAX)."""
        lib, stream = _lib_and_stream(keys.device)
        pair = torch.tensor([2**31 - 1, -2**31], dtype=torch.int32, device=keys.device)
        if keys.length:
            span = keys.span()
            check(lib.arx_groupby_key_range_sampled_i32(C.byref(span), int(sample_rows or RangeGroupBySum.SAMPLE_ROWS),
                                                        pair.data_ptr(), stream))
        wide = pair.to(torch.int64)
        return torch.stack([-wide[0], wide[1]])

    @staticmethod
    def plan_for(max_rows: int, key_min: int, key_max: int, sampled: bool = True):
        """The plan for keys in [key_min, key_max] (widened by 1/64 of the range on both sides when the bounds come from a
        sample) or None when the range does not suit the state."""
        if key_min > key_max:
            return None
        pad = ((key_max - key_min + 1) // 64 + 1) if sampled else 0
        lo, hi = max(-2**31, key_min - pad), min(2**31 - 1, key_max + pad)
        plan = _lib.ArxRangePlan()
        rc = _lib.get_lib().arx_groupby_range_plan(int(max_rows), lo, hi, C.byref(plan))
        if rc == _lib.ARX_NOT_IMPLEMENTED:
            return None
        check(rc)
        return plan

    def __init__(self, plan, device=None, options: ScalarAggregateOptions | None = None):
        from .array import default_device

        self.plan = plan
        self.device = torch.device(device) if device is not None else default_device()
        self.options = options or ScalarAggregateOptions()
        self.state = torch.zeros(int(plan.state_bytes) // 8, dtype=torch.int64, device=self.device)

    def partition_bytes(self) -> int:
        return int(self.plan.width) * 16

    def consume(self, keys: Array, values: Array) -> bool:
        """Adds the rows' groups; False = declined (nothing consumed): nulls, a key outside the plan, a hot key."""
        if keys.type != int32 or values.type != int64:
            return False
        if (keys.null_count != 0 and keys.buffers[0] is not None) or (values.null_count != 0 and values.buffers[0] is not None):
            return False
        if keys.length == 0:
            return True
        lib, stream = _lib_and_stream(self.device)
        probe = _lib.ArxRangePlan()
        check(lib.arx_groupby_range_plan(keys.length, self.plan.key_min, self.plan.key_min + int(self.plan.slots) - 1, C.byref(probe)))
        ws = _workspace(self.device, int(probe.workspace_bytes) + 256, "groupby")
        ks, vs = keys.span(), values.span()
        rc = lib.arx_groupby_range_sum_i64_consume(self.state.data_ptr(), C.byref(self.plan), C.byref(ks), C.byref(vs),
                                                   ws.data_ptr(), ws.numel(), stream)
        if rc in (_lib.ARX_CAPACITY_ERROR, _lib.ARX_NOT_IMPLEMENTED):
            return False
        check(rc)
        return True

    def merge_blocks(self, first_partition: int, num_partitions: int, others: torch.Tensor, num_others: int) -> None:
        """partitions [first, first + num) += the same partitions of num_others states lying one behind the other in
        `others` (a uint8 / int64 tensor of num_others x num_partitions x width x 16 bytes)."""
        if num_partitions == 0 or num_others == 0:
            return
        lib, stream = _lib_and_stream(self.device)
        stride = num_partitions * self.partition_bytes()
        dst = self.state.data_ptr() + first_partition * self.partition_bytes()
        check(lib.arx_groupby_range_merge(dst, others.data_ptr(), self.plan.width, num_partitions, num_others, stride, stream))

    def finalize(self, first_partition: int = 0, num_partitions: int | None = None, blocks: torch.Tensor | None = None):
        """(keys, key_is_valid, sums, valid) of the partitions [first, first + num), ascending by key — the tuple
        GroupBySum.finalize returns.  `blocks`: finalize these partitions' blocks from another buffer instead of the state."""
        lib, stream = _lib_and_stream(self.device)
        if num_partitions is None:
            num_partitions = int(self.plan.partitions) - first_partition
        slots = num_partitions * int(self.plan.width)
        dev = self.device
        keys = torch.empty(max(slots, 1), dtype=torch.int32, device=dev)
        sums = torch.empty(max(slots, 1), dtype=torch.int64, device=dev)
        valid = torch.empty(max(slots, 1), dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        ws = alloc(lib.arx_groupby_range_finalize_workspace_bytes(slots), dev)
        src = (blocks.data_ptr() if blocks is not None else self.state.data_ptr() + first_partition * self.partition_bytes())
        check(lib.arx_groupby_range_finalize(src, self.plan.key_min + first_partition * int(self.plan.width), self.plan.width,
                                             num_partitions, int(self.options.min_count), ws.data_ptr(), ws.numel(),
                                             keys.data_ptr(), sums.data_ptr(), None, valid.data_ptr(), count.data_ptr(), stream))
        g = int(count.item())
        return keys[:g], torch.ones(g, dtype=torch.uint8, device=dev), sums[:g], valid[:g]


def indices_nonzero(arr: Array) -> Array:
    """compute::IndicesNonZero (kernels/vector_selection.cc:352, vector_selection.cc DoNonZero): the uint64 positions
    of the elements that are valid and non-zero (true for booleans), ascending.  = GetTakeIndices of the mask
    `arr != 0` (nulls dropped), widened to uint64."""
    if arr.type == bool_:
        mask = arr
    elif arr.type.name in _NUM_TYPE_ID:
        wide = arr
        if arr.type not in (int64, float64):
            wide = cast(arr, float64 if arr.type.name in ("float", "double") else
                        (uint64 if arr.type.name.startswith("uint") else int64))
            if wide.type == uint64:       # same zero-ness, same bits
                wide = Array(int64, wide.length, wide.buffers, wide.null_count, wide.offset)
        mask = call_function("not_equal", [wide, _wrap_scalar(0 if wide.type == int64 else 0.0, wide)])
    else:
        raise ArrowNotImplementedError(f"indices_nonzero: {arr.type.name} values")
    idx = get_take_indices(mask)
    return cast(idx, uint64)


def group_by_mean(keys: Array, values: Array, capacity: int | None = None,
                  options: ScalarAggregateOptions | None = None):
    """Table.group_by(k).aggregate([(v, 'mean')]) for one int32 key and one int64 value (see finalize_mean)."""
    cap = capacity or max(16, 2 * keys.length + 2)
    op = GroupBySum(cap, keys.device, options)
    op.consume(keys, values)
    op.consume_min_max(keys, values)
    return op.finalize_mean()


def _groups_by_first_row(arr: Array, capacity: int | None, with_counts: bool):
    """The distinct int32 values of `arr` ordered by first appearance, from the fused group-by table:
    the rows' own numbers go through the min reducer (first row of every group) and, for
    value_counts, through the sum consume (whose `counts` column is the number of rows per group);
    the G groups are then ordered by first row with array_sort_indices + take.  Everything
    row-sized runs in the HIP kernels; torch only numbers the rows.
    Returns (keys int32 tensor[G], key_is_valid uint8 tensor[G], counts Array | None)."""
    if arr.type != int32:
        raise ArrowNotImplementedError("unique / value_counts / dictionary_encode on the gfx950 path: int32 values only")
    dev = arr.device
    n = arr.length
    rows = Array(int64, n, [None, torch.arange(n, dtype=torch.int64, device=dev).view(torch.uint8)], 0, 0)
    op = GroupBySum(capacity or max(16, 2 * n + 2), dev)
    if with_counts:
        op.consume(arr, rows)
    op.consume_min_max(arr, rows)
    p = op.export_min_max()
    g = int(p["keys"].numel())
    as_arr = lambda t, col: Array(t, g, [None, col.contiguous().view(torch.uint8)], 0, 0)  # noqa: E731
    order = call_function("array_sort_indices", [as_arr(int64, p["mins"])], ArraySortOptions())
    keys = take(as_arr(int32, p["keys"]), order, boundscheck=False).data[: g * 4].view(torch.int32)
    kvalid = take(as_arr(uint8, p["key_is_valid"]), order, boundscheck=False).data[:g]
    counts = take(as_arr(int64, p["counts"]), order, boundscheck=False) if with_counts else None
    return keys, kvalid, counts


def _values_array(keys: torch.Tensor, kvalid: torch.Tensor) -> Array:
    """int32 Array over `keys` whose only possible null (all nulls are one group) is cleared in a fresh bitmap."""
    g = int(keys.numel())
    dev = keys.device
    validity, null_count = None, 0
    null_pos = torch.nonzero(kvalid == 0)
    if null_pos.numel():
        pos = int(null_pos[0])
        validity = torch.full((bitmap_nbytes(g),), 0xFF, dtype=torch.uint8, device=dev)
        validity[g // 8:] = 0
        if g % 8:
            validity[g // 8] = (1 << (g % 8)) - 1
        validity[pos // 8] = int(validity[pos // 8]) & ~(1 << (pos % 8))
        null_count = 1
    data = keys.contiguous().view(torch.uint8)
    if data.numel() < 64:      # keep the 64-byte padding every device buffer has
        padded = alloc(64, dev, zero=True)
        padded[: data.numel()] = data
        data = padded
    return Array(int32, g, [validity, data], null_count, 0)


def _first_occurrence_groups(arr: Array, capacity: int | None, with_counts: bool):
    dev = arr.device
    if arr.length == 0:
        empty = Array(int32, 0, [None, alloc(0, dev)], 0, 0)
        return empty, Array(int64, 0, [None, alloc(0, dev)], 0, 0)
    keys, kvalid, counts = _groups_by_first_row(arr, capacity, with_counts)
    return _values_array(keys, kvalid), counts


def dictionary_encode(arr: Array, null_encoding: str = "mask", capacity: int | None = None):
    """compute::DictionaryEncode (DictEncodeAction, kernels/vector_hash.cc:173-270) for int32:
    (indices int32 Array, dictionary int32 Array); the dictionary holds the distinct values in order
    of first appearance.  null_encoding "mask" (default): nulls stay null in the indices and are not
    in the dictionary; "encode": the null is a dictionary entry like any value.
    Groups -> first rows -> order (as unique), the positions merged back into a table as its "sums",
    then one read-only lookup per row (arx_groupby_lookup_i32)."""
    if null_encoding not in ("mask", "encode"):
        raise ArrowInvalid("null_encoding must be 'mask' or 'encode'")
    dev = arr.device
    n = arr.length
    if n == 0:
        return (Array(int32, 0, [None, alloc(0, dev)], 0, 0), Array(int32, 0, [None, alloc(0, dev)], 0, 0))
    keys, kvalid, _ = _groups_by_first_row(arr, capacity, False)
    if null_encoding == "mask":
        keep = kvalid != 0
        keys, kvalid = keys[keep].contiguous(), kvalid[keep].contiguous()
    g = int(keys.numel())
    lib, stream = _lib_and_stream(dev)
    table = GroupBySum(max(16, 2 * g + 2), dev)
    if g:
        ids = torch.arange(g, dtype=torch.int64, device=dev)
        zeros = torch.zeros(g, dtype=torch.int64, device=dev)
        check(lib.arx_groupby_sum_i64_merge(table.state.data_ptr(), table.capacity, keys.data_ptr(), kvalid.data_ptr(),
                                            ids.data_ptr(), zeros.data_ptr(), None, g, stream))
    out = alloc(n * 4, dev)
    sp = arr.span()
    check(lib.arx_groupby_lookup_i32(table.state.data_ptr(), table.capacity, C.byref(sp), out.data_ptr(), stream))
    if null_encoding == "mask":
        validity, nc = _propagate_validity([arr], n, dev)
    else:
        validity, nc = None, 0
    return Array(int32, n, [validity, out], nc, 0), _values_array(keys, kvalid)


def unique(arr: Array, capacity: int | None = None) -> Array:
    """compute::Unique (api_vector.cc; UniqueAction, kernels/vector_hash.cc:65-120) for int32:
    distinct values in order of first appearance, the nulls as one entry.  `capacity`: slots of
    the device hash table (default 2 * length + 2; pass ~2x the expected distinct count to save HBM)."""
    return _first_occurrence_groups(arr, capacity, False)[0]


def value_counts(arr: Array, capacity: int | None = None):
    """compute::ValueCounts (ValueCountsAction, kernels/vector_hash.cc:125-190) for int32:
    (values, counts int64) in order of first appearance; nulls are counted as one value."""
    return _first_occurrence_groups(arr, capacity, True)


class _GrouperLevel:
    """One device table of csrc/grouper.hip: key rows of up to 8 fixed-width columns and 16 bytes (`Grouper` below
    chains several of these for wider rows)."""

    def __init__(self, key_types, max_groups: int, device=None):
        from .array import default_device

        self.key_types = list(key_types)
        self.device = torch.device(device) if device is not None else default_device()
        self.max_groups = max(1, int(max_groups))
        self._widths = (C.c_int32 * len(self.key_types))(*[t.byte_width for t in self.key_types])
        lib, stream = _lib_and_stream(self.device)
        self.state = alloc(lib.arx_grouper_state_bytes(self.max_groups) + 256, self.device)
        self._state_ptr = (self.state.data_ptr() + 255) & ~255
        check(lib.arx_grouper_init(self._state_ptr, self.max_groups, stream))

    def reset(self) -> None:
        lib, stream = _lib_and_stream(self.device)
        check(lib.arx_grouper_init(self._state_ptr, self.max_groups, stream))

    def _spans(self, batch):
        cols = list(batch.values) if isinstance(batch, ExecBatch) else list(batch)
        if len(cols) != len(self.key_types):
            raise ArrowInvalid(f"Grouper: expected {len(self.key_types)} key columns, got {len(cols)}")
        n = cols[0].length
        for c, t in zip(cols, self.key_types):
            if c.type != t:
                raise ArrowInvalid(f"Grouper: key column of type {c.type.name}, expected {t.name}")
            if c.length != n:
                raise ArrowInvalid("Array arguments must all be the same length")
        spans = (_lib.ArxSpan * len(cols))(*[c.span() for c in cols])
        return cols, spans, n

    def _run(self, batch, lookup: bool):
        lib, stream = _lib_and_stream(self.device)
        cols, spans, n = self._spans(batch)
        ids = alloc(max(n, 1) * 4, self.device)
        ws_bytes = lib.arx_grouper_consume_workspace_bytes(n)
        ws = _workspace(self.device, ws_bytes + 256, "grouper")
        ws_ptr = (ws.data_ptr() + 255) & ~255
        ws_len = ws.numel() - (ws_ptr - ws.data_ptr())
        if lookup:
            valid = alloc(bitmap_nbytes(n), self.device, zero=True)
            check(lib.arx_grouper_lookup(self._state_ptr, self.max_groups, spans, self._widths, len(cols), ws_ptr,
                                         ws_len, ids.data_ptr(), valid.data_ptr(), stream))
            return Array(uint32, n, [valid, ids], kUnknownNullCount, 0)
        check(lib.arx_grouper_consume(self._state_ptr, self.max_groups, spans, self._widths, len(cols), ws_ptr, ws_len,
                                      ids.data_ptr(), stream))
        return Array(uint32, n, [None, ids], 0, 0)

    def consume(self, batch) -> Array:
        return self._run(batch, lookup=False)

    def lookup(self, batch) -> Array:
        return self._run(batch, lookup=True)

    def populate(self, batch) -> None:
        self._run(batch, lookup=False)

    @property
    def num_groups(self) -> int:
        lib, stream = _lib_and_stream(self.device)
        n = C.c_int64(0)
        check(lib.arx_grouper_num_groups(self._state_ptr, C.byref(n), stream))
        return n.value

    def get_uniques(self):
        """The unique key rows as one Array per key column, in group-id order."""
        lib, stream = _lib_and_stream(self.device)
        g = self.num_groups
        out = []
        for j, t in enumerate(self.key_types):
            data = alloc(max(g, 1) * t.byte_width, self.device)
            valid = alloc(bitmap_nbytes(g), self.device, zero=True)
            nulls = C.c_int64(0)
            check(lib.arx_grouper_get_uniques(self._state_ptr, self.max_groups, self._widths, len(self.key_types), j,
                                              data.data_ptr(), valid.data_ptr(), C.byref(nulls), stream))
            out.append(Array(t, g, [valid if nulls.value else None, data], nulls.value, 0))
        return ExecBatch(out, g)


kGrouperLevelBytes = 16   # csrc/grouper.hip: one table holds key rows of up to 16 bytes ...
kGrouperLevelKeys = 8     # ... and 8 columns


def _grouper_levels(widths):
    """Key columns -> the levels of the chain: level 0 takes columns while they fit 16 bytes / 8 columns, every later
    level takes the previous level's uint32 group id (4 bytes, never null) plus the columns that fit beside it."""
    levels, cur, used = [], [], 0
    for j, w in enumerate(widths):
        if cur and (used + w > kGrouperLevelBytes or len(cur) + (1 if levels else 0) >= kGrouperLevelKeys):
            levels.append(cur)
            cur, used = [], 4
        cur.append(j)
        used += w
    levels.append(cur)
    return levels


class Grouper:
    """arrow::compute::Grouper (compute/row/grouper.h:104-137) over key columns that live in HBM: `consume(batch)`
    -> uint32 group ids (:121), `lookup` (:126; unseen keys -> null), `populate` (:130), `get_uniques` (:134),
    `num_groups` (:137), `reset` (:115).  Key rows = one or several fixed-width columns (byte widths 1, 2, 4, 8),
    compared by their bits with null as a key value of its own, as the reference's row encoder does (GrouperFastImpl,
    row/grouper.cc:555-973; any number of fixed-width columns, :559-611).  The k-th distinct key row in row order gets
    id k.  `max_groups` bounds the distinct rows over the Grouper's life.

    One device table holds rows of up to 16 bytes (32-byte slots, csrc/grouper.hip).  Wider rows go through a CHAIN of
    tables instead of wider slots: level 0 maps the first columns to ids, level s maps (id of level s-1, next columns) —
    a 4-byte id stands for everything to its left, so every slot stays 32 bytes whatever the row width, and the ids of
    the last level are the ids of the whole row, in order of first appearance (a row's tuple (prefix id, columns)
    appears first exactly where the row does).  GetUniques walks back: level s keeps its groups' level s-1 ids, so the
    columns of level s are gathered through the composed id maps (`take`)."""

    def __init__(self, key_types, max_groups: int, device=None):
        from .array import default_device

        self.key_types = list(key_types)
        if not 1 <= len(self.key_types) <= 32:
            raise ArrowNotImplementedError(f"Grouper: 1 to 32 key columns (got {len(self.key_types)})")
        for t in self.key_types:
            if t.bit_width not in (8, 16, 32, 64):
                raise ArrowNotImplementedError(f"Grouper: keys of type {t.name}")
        self.device = torch.device(device) if device is not None else default_device()
        self.max_groups = max(1, int(max_groups))
        self._level_cols = _grouper_levels([t.byte_width for t in self.key_types])
        self._levels = []
        for s, cols in enumerate(self._level_cols):
            types = ([uint32] if s else []) + [self.key_types[j] for j in cols]
            self._levels.append(_GrouperLevel(types, self.max_groups, self.device))

    @classmethod
    def make(cls, key_types, max_groups: int, device=None) -> "Grouper":
        """Grouper::Make (:110)."""
        return cls(key_types, max_groups, device)

    @property
    def num_levels(self) -> int:
        return len(self._levels)

    def reset(self) -> None:
        for lv in self._levels:
            lv.reset()

    def _check(self, batch):
        cols = list(batch.values) if isinstance(batch, ExecBatch) else list(batch)
        if len(cols) != len(self.key_types):
            raise ArrowInvalid(f"Grouper: expected {len(self.key_types)} key columns, got {len(cols)}")
        n = cols[0].length
        for c, t in zip(cols, self.key_types):
            if c.type != t:
                raise ArrowInvalid(f"Grouper: key column of type {c.type.name}, expected {t.name}")
            if c.length != n:
                raise ArrowInvalid("Array arguments must all be the same length")
        return cols

    def _run(self, batch, lookup: bool):
        cols = self._check(batch)
        ids = None
        for lv, idx in zip(self._levels, self._level_cols):
            # a Lookup's unseen prefix is a null id: no consumed row has one, so the next level does not find it either
            part = ([ids] if ids is not None else []) + [cols[j] for j in idx]
            ids = lv._run(part, lookup)
        return ids

    def consume(self, batch) -> Array:
        return self._run(batch, lookup=False)

    def lookup(self, batch) -> Array:
        return self._run(batch, lookup=True)

    def populate(self, batch) -> None:
        self._run(batch, lookup=False)

    @property
    def num_groups(self) -> int:
        return self._levels[-1].num_groups

    def get_uniques(self):
        """The unique key rows as one Array per key column, in group-id order."""
        out = [None] * len(self.key_types)
        to_level = None   # final group id -> group id of the level at hand (None: the identity, at the last level)
        for s in range(len(self._levels) - 1, -1, -1):
            u = self._levels[s].get_uniques().values
            own = u[1:] if s else u
            for j, a in zip(self._level_cols[s], own):
                out[j] = a if to_level is None else take(a, to_level, boundscheck=False)
            if s:
                to_level = u[0] if to_level is None else take(u[0], to_level, boundscheck=False)
        return ExecBatch(out, self.num_groups)



def binary_key_columns(arr: Array):
    """A utf8 / binary KEY column as the fixed-width virtual key columns the chain of Grouper tables takes
    (arx_binary_key_lengths / arx_binary_key_chunk; the var-length part of the reference's key rows,
    row/grouper.cc:559-611): (lengths uint32 Array — 0xFFFFFFFF for a null, [(lo uint64 Array, hi uint32 Array) per
    12-byte chunk, zero-padded past the string's end])."""
    lib, stream = _lib_and_stream(arr.device)
    n = arr.length
    bspan = arr.binary_span()
    lens = alloc(max(n, 1) * 4, arr.device)
    ws = _workspace(arr.device, 256, "binary_key")
    max_len = C.c_int64(0)
    check(lib.arx_binary_key_lengths(C.byref(bspan), lens.data_ptr(), C.byref(max_len), ws.data_ptr(), stream))
    chunks = []
    for c in range((max_len.value + 11) // 12):
        lo, hi = alloc(max(n, 1) * 8, arr.device), alloc(max(n, 1) * 4, arr.device)
        check(lib.arx_binary_key_chunk(C.byref(bspan), c, lo.data_ptr(), hi.data_ptr(), stream))
        chunks.append((Array(uint64, n, [None, lo], 0, 0), Array(uint32, n, [None, hi], 0, 0)))
    return Array(uint32, n, [None, lens], 0, 0), chunks


def group_first_rows(group_ids: Array, num_groups: int) -> Array:
    """first_rows[g] = the smallest row whose group id is g (arx_group_first_rows): `take(keys, first_rows)` are the
    unique key rows in group-id order — how var-width keys come back out of the chain of tables."""
    lib, stream = _lib_and_stream(group_ids.device)
    out = alloc(max(num_groups, 1) * 4, group_ids.device)
    check(lib.arx_group_first_rows(group_ids.buffers[1].data_ptr() + 4 * group_ids.offset, group_ids.length, num_groups,
                                   out.data_ptr(), stream))
    return Array(uint32, num_groups, [None, out], 0, 0)


_GROUP_BY_AGGREGATES = ("hash_sum", "hash_count", "hash_mean")


def group_by(keys, aggregates, max_groups: int | None = None, options: ScalarAggregateOptions | None = None):
    """What GroupByNode does with one batch (acero/groupby_aggregate_node.cc:210-337): Grouper::Consume over the key
    columns, then every aggregate's {resize, consume} on (values, group ids), then finalize + GetUniques.
    keys: list of Arrays (any fixed-width types up to 16 bytes per row — int64 keys, several key columns);
    aggregates: list of (values Array, "hash_sum" | "hash_count" | "hash_mean") over int64 values.
    Returns (unique key columns, [one result Array per aggregate]), rows in group-id order (first appearance)."""
    keys = list(keys)
    n = keys[0].length
    g = Grouper([k.type for k in keys], max_groups or max(16, n), keys[0].device)
    ids = g.consume(keys)
    num_groups = g.num_groups
    results = []
    states = {}
    for values, fn in aggregates:
        if fn not in _GROUP_BY_AGGREGATES:
            raise ArrowNotImplementedError(f"group_by: aggregate {fn}")
        if id(values) not in states:   # sum / count / mean of one column share its state
            st = _hash_sum_init(options, keys[0].device)
            _hash_sum_resize(st, num_groups)
            _hash_sum_consume(st, [GroupBySum._normalise_value(GroupBySum.__new__(GroupBySum), values), ids])
            states[id(values)] = st
        st = states[id(values)]
        if fn == "hash_sum":
            out = _hash_sum_finalize(st)
            if values.type.name.startswith("uint"):
                out = Array(uint64, out.length, out.buffers, out.null_count, out.offset)
        elif fn == "hash_count":
            out = Array(int64, num_groups, [None, st.counts[:num_groups].contiguous().view(torch.uint8)], 0, 0)
        else:
            out = _hash_mean_from_dense(st, values)
        results.append(out)
    return g.get_uniques(), results


def _hash_mean_from_dense(st: "GroupedSumInt64State", values: Array) -> Array:
    """hash_mean(int64) from the dense sums / counts: GroupedMeanImpl::Finalize (hash_aggregate_numeric.cc:352-430)
    divides a sum that was accumulated as DOUBLES in row order; that equals double(exact sum) / count exactly when
    every partial sum is an integer below 2^53 — guaranteed here when count * max|value| < 2^53 for every group,
    which is checked with the column's extrema (a bound, not per group); otherwise declined."""
    if values.type != int64:
        raise ArrowNotImplementedError(f"group_by: hash_mean of {values.type.name}")
    g = st.num_groups
    mm = min_max(values)
    lo, hi = mm if mm else (0, 0)
    bound = builtins.max(builtins.abs(int(lo)), builtins.abs(int(hi)))
    lib, stream = _lib_and_stream(st.device)
    bits = alloc(bitmap_nbytes(g), st.device, zero=True)
    counter = torch.zeros(8, dtype=torch.uint8, device=st.device)
    check(lib.arx_hash_sum_i64_finalize(st.counts.data_ptr(), st.null_seen.data_ptr(), g, int(st.options.skip_nulls),
                                        st.options.min_count, bits.data_ptr(), counter.data_ptr(), stream))
    means = alloc(max(g, 1) * 8, st.device)
    inexact = torch.zeros(1, dtype=torch.int32, device=st.device)
    check(lib.arx_hash_mean_i64_finalize(st.sums.data_ptr(), st.counts.data_ptr(), g, bound, means.data_ptr(),
                                         inexact.data_ptr(), stream))
    if int(inexact.item()) != 0:
        raise ArrowNotImplementedError(
            "hash_mean(int64): a group's partial sums may exceed 2^53, where the reference's row-order double "
            "accumulation is not associative (its result depends on row order); not reproducible bit for bit")
    nulls = g - int(counter.cpu().view(torch.int64)[0])
    return Array(float64, g, [bits if nulls else None, means], nulls, 0)


def group_by_sum(keys: Array, values: Array, capacity: int | None = None,
                 options: ScalarAggregateOptions | None = None):
    """Table.group_by(k).aggregate([(v, 'sum')]) for one int32 key and one int64 value.  Large null-free inputs whose keys
    come from a narrow range go through the range-partitioned state (RangeGroupBySum: no hash table, groups in key order);
    everything else — and whatever that state declines — through the table operator."""
    if (keys.type == int32 and values.type == int64 and keys.length >= RangeGroupBySum.MIN_ROWS and
            not (keys.null_count != 0 and keys.buffers[0] is not None) and not (values.null_count != 0 and values.buffers[0] is not None)):
        neg_lo, hi = [int(x) for x in RangeGroupBySum.sampled_key_range(keys).cpu().tolist()]
        plan = RangeGroupBySum.plan_for(keys.length, -neg_lo, hi) if -neg_lo <= hi else None
        if plan is not None:
            st = RangeGroupBySum(plan, keys.device, options)
            if st.consume(keys, values):
                return st.finalize()
    cap = capacity or max(16, 2 * keys.length + 2)
    op = GroupBySum(cap, keys.device, options)
    op.consume(keys, values)
    return op.finalize()


# --------------------------------------------------------------------------- set lookup
# is_in / index_in (compute/kernels/scalar_set_lookup.cc): the value set becomes a device hash table once per call
# (arx_set_lookup_build*), every row is looked up once (arx_set_lookup_is_in / _index_in*).  Bits of the string hash the
# binary tables keep: 64 in production; tests lower it to force collisions, which the byte comparison resolves.
SET_LOOKUP_HASH_BITS = 64


def _pa_type(t: DataType):
    """The pyarrow type of a device array's type (without touching its buffers)."""
    import pyarrow as pa

    from .array import _PA_ALIAS, _pa_temporal, is_temporal

    if is_base_binary(t):
        return pa.binary() if t.name == "binary" else pa.string()
    if is_temporal(t):
        return _pa_temporal(t.name)
    return pa.type_for_alias(_PA_ALIAS[t.name])


def _value_set_pyarrow(value_set):
    import pyarrow as pa

    if isinstance(value_set, Array):
        return value_set.to_pyarrow()
    if isinstance(value_set, pa.ChunkedArray):      # indexed across its chunks
        return value_set.combine_chunks() if value_set.num_chunks else pa.array([], value_set.type)
    if isinstance(value_set, pa.Array):
        return value_set
    return pa.array(list(value_set))


def _resolve_set_lookup(values: Array, value_set, skip_nulls: bool):
    """SetLookupState's type resolution: the value set is cast to the input's type when that cast is safe, otherwise
    the input is compared in the value set's type (a device cast).  Pairs the reference refuses raise its own error: a
    zero-length call of the reference settles them."""
    import pyarrow as pa
    import pyarrow.compute as pc

    from .array import type_from_name

    vt = _pa_type(values.type)
    vs = _value_set_pyarrow(value_set)
    pc.is_in(pa.array([], vt), value_set=vs, skip_nulls=skip_nulls)
    if vs.type == vt:
        return values, vs
    try:
        return values, vs.cast(vt, safe=True)
    except (pa.ArrowInvalid, pa.ArrowNotImplementedError, pa.ArrowTypeError):
        try:
            set_type = type_from_name(str(vs.type))
        except Exception:
            raise ArrowNotImplementedError(f"is_in / index_in of {values.type.name} values against a {vs.type} value set on the "
                                           "device: no device cast between them") from None
        return cast(values, set_type), vs


def _set_lookup(values: Array, value_set, skip_nulls: bool, index: bool):
    if not isinstance(values, Array):
        raise TypeError("is_in / index_in: values must be an arrow_amd.Array")
    probe, vs = _resolve_set_lookup(values, value_set, bool(skip_nulls))
    dev = values.device
    lib, stream = _lib_and_stream(dev)
    t = probe.type
    try:
        dset = Array.from_pyarrow(vs, device=dev)
    except KeyError:
        raise ArrowNotImplementedError(f"is_in / index_in of {t.name} values on the device") from None
    m = len(vs)
    binary = is_base_binary(t)
    if not binary and t != bool_ and t.byte_width not in (1, 2, 4, 8, 16):
        raise ArrowNotImplementedError(f"is_in / index_in of {t.name} values on the device")
    kw = -1 if binary else (0 if t == bool_ else t.byte_width)
    state = alloc(int(lib.arx_set_lookup_state_bytes(m, kw)), dev)
    n = probe.length
    words = alloc(max(1, (n + 63) // 64) * 8, dev)
    out_index = alloc(max(1, n) * 4, dev) if index else None
    idx_ptr = out_index.data_ptr() if index else None
    skip = int(bool(skip_nulls))
    if binary:
        bits = SET_LOOKUP_HASH_BITS
        sspan, vspan = dset.binary_span(), probe.binary_span()
        check(lib.arx_set_lookup_build_binary(state.data_ptr(), C.byref(sspan), 4, bits, stream))
        if index:
            check(lib.arx_set_lookup_index_in_binary(state.data_ptr(), C.byref(sspan), 4, bits, C.byref(vspan), 4, skip, idx_ptr,
                                                     words.data_ptr(), stream))
        else:
            check(lib.arx_set_lookup_is_in_binary(state.data_ptr(), C.byref(sspan), 4, bits, C.byref(vspan), 4, skip,
                                                  words.data_ptr(), stream))
    else:
        sspan, vspan = dset.span(), probe.span()
        check(lib.arx_set_lookup_build(state.data_ptr(), C.byref(sspan), kw, stream))
        if index:
            check(lib.arx_set_lookup_index_in(state.data_ptr(), m, kw, C.byref(vspan), skip, idx_ptr, words.data_ptr(), stream))
        else:
            check(lib.arx_set_lookup_is_in(state.data_ptr(), m, kw, C.byref(vspan), skip, words.data_ptr(), stream))
    if not index:
        return Array(bool_, n, [None, words], 0, 0)
    out = Array(int32, n, [words, out_index], kUnknownNullCount, 0)
    out.set_lazy_null_count(_lazy_null_count(words, n))
    return out


def is_in(values: Array, value_set, *, skip_nulls: bool = False) -> Array:
    """compute::IsIn (scalar_set_lookup.cc): a boolean array, true where the row's value is in `value_set` (a pyarrow
    array or chunked array, a Python list or an arrow_amd.Array), never null.  Values compare by their bits; a null row
    matches a null in the set unless skip_nulls.  The result stays on the device."""
    return _set_lookup(values, value_set, skip_nulls, False)


def index_in(values: Array, value_set, *, skip_nulls: bool = False) -> Array:
    """compute::IndexIn (scalar_set_lookup.cc): int32, the index of the row's value's first occurrence in `value_set`
    (chunks counted one after the other), null where the value is absent.  The result stays on the device."""
    return _set_lookup(values, value_set, skip_nulls, True)


# --------------------------------------------------------------------------- what the scalar kernels below share
def _lazy_null_count(bitmap, n: int):
    """For set_lazy_null_count: the zeros among the first n bits of the device bitmap, read back on first use."""
    nbytes = (n + 7) // 8
    return lambda: n - int(np.unpackbits(bitmap[:nbytes].cpu().numpy(), bitorder="little")[:n].sum()) if n else 0


def _require_array(name: str, x) -> None:
    if not isinstance(x, Array):
        raise ArrowNotImplementedError(f"arrow_amd: {name} of a scalar on the device path")


def _input_has_nulls(values: Array) -> bool:
    """Whether a one-operand kernel has to look at its input's bitmap: there is one, and the null count is not known to
    be 0 (a pending device-side count stays pending: no read-back here)."""
    known = values._null_count
    return values.validity is not None and (callable(known) or known != 0)


def _unary_span(values: Array):
    """The ArxSpan of a one-operand fixed-width kernel's input: no bitmap unless _input_has_nulls."""
    known = values._null_count
    return _lib.ArxSpan(values.validity.data_ptr() if _input_has_nulls(values) else None, values.data.data_ptr(), values.offset,
                        values.length, kUnknownNullCount if callable(known) else int(known))


def _carry_null_count(res: Array, values: Array) -> Array:
    """`res`, whose validity is that of `values` at offset 0: the input's null count where it is known, a count on first
    use otherwise."""
    known = values._null_count
    if callable(known) or known == kUnknownNullCount:
        res.set_lazy_null_count(_lazy_null_count(res.validity, res.length))
    else:
        res._null_count = int(known)
    return res


def _under_input_validity(values: Array, out_type: DataType, *out) -> Array:
    """The result of a one-operand kernel: the buffers `out` under the input's validity at offset 0.  No bitmap unless
    _input_has_nulls; the input's own bitmap, shared like the two-operand kernels do, when it is at offset 0 already, a
    re-based copy otherwise."""
    n = values.length
    if not _input_has_nulls(values):
        return Array(out_type, n, [None, *out], 0, 0)
    valid = values.validity
    if values.offset != 0:
        lib, stream = _lib_and_stream(values.device)
        valid = alloc(bitmap_nbytes(n), values.device)
        check(lib.arx_bitmap_copy(values.validity.data_ptr(), values.offset, n, valid.data_ptr(), stream))
    return _carry_null_count(Array(out_type, n, [valid, *out], kUnknownNullCount, 0), values)


def _literal_operand(name: str, what: str, x) -> bytes:
    """A literal operand as bytes (str: UTF-8 encoded); `what` opens the TypeError, as in "pattern must be"."""
    if isinstance(x, str):
        return x.encode("utf-8")
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    raise TypeError(f"{name}: {what} str or bytes, not {type(x).__name__}")


def _device_literal(dev, *parts: bytes):
    """The literal operands of a call back to back in one device tensor of at least one byte.  The caller drops it on
    return while its kernels may still be queued: torch's caching allocator hands a freed block out again only to work
    queued behind this call on the same stream."""
    raw = b"".join(parts)
    out = alloc(max(len(raw), 1), dev)
    if raw:
        out[:len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
    return out


def _values_wrapper(name: str, doc: str, what: str):
    """The public function `name(values)` of a kernel that takes no options; its docstring is doc.format(what)."""
    def f(values: Array) -> Array:
        return call_function(name, [values])
    f.__name__ = f.__qualname__ = name
    f.__doc__ = doc.format(what)
    return f


# --------------------------------------------------------------------------- substring predicates
# match_substring / starts_with / ends_with with a literal pattern (compute/kernels/scalar_string_ascii.cc, MatchSubstring
# under MatchSubstringOptions{pattern, ignore_case}): csrc/match_substring.hip.  The `path` handed to
# arx_match_substring: 0 = the library chooses (rows, or bytes from a mean row size on), 1 = one lane per row, 2 = the
# lanes walk the bytes (match_substring only).  Tests set it to reach either kernel.
MATCH_SUBSTRING_PATH = 0
_MATCH_OPS = {"match_substring": 0, "starts_with": 1, "ends_with": 2}


def _exec_match_substring(name: str):
    def run(args, options):
        return _match_substring(name, args[0], options.pattern, options.ignore_case)
    return run


def _call_match_substring(name: str, values, pattern, ignore_case: bool) -> Array:
    return _call_string_function(name, values, MatchSubstringOptions(pattern, ignore_case), "")


def _match_substring(name: str, values: Array, pattern, ignore_case: bool) -> Array:
    pattern = _literal_operand(name, "pattern must be", pattern)
    if ignore_case:
        raise ArrowNotImplementedError(f"arrow_amd: {name} with ignore_case=True on device-resident arrays")
    dev = values.device
    lib, stream = _lib_and_stream(dev)
    n = values.length
    words = alloc(max(1, (n + 63) // 64) * 8, dev)
    dpat = _device_literal(dev, pattern)
    vspan = values.binary_span()
    check(lib.arx_match_substring(C.byref(vspan), 4, _MATCH_OPS[name], dpat.data_ptr(), len(pattern), _data_bytes_hint(values),
                                  int(MATCH_SUBSTRING_PATH), words.data_ptr(), stream))
    return _under_input_validity(values, bool_, words)


def match_substring(values: Array, pattern, *, ignore_case: bool = False) -> Array:
    """compute::MatchSubstring (scalar_string_ascii.cc): a boolean array, true where the row contains `pattern` (str,
    UTF-8 encoded, or bytes) as a run of bytes; null where the row is null.  The empty pattern matches every valid row.
    utf8 / binary values; ignore_case=True raises ArrowNotImplementedError (there is no CPU fallback).  The result stays
    on the device."""
    return _call_match_substring("match_substring", values, pattern, ignore_case)


def starts_with(values: Array, pattern, *, ignore_case: bool = False) -> Array:
    """compute::StartsWith: true where the row's first bytes are `pattern`.  See match_substring."""
    return _call_match_substring("starts_with", values, pattern, ignore_case)


def ends_with(values: Array, pattern, *, ignore_case: bool = False) -> Array:
    """compute::EndsWith: true where the row's last bytes are `pattern`.  See match_substring."""
    return _call_match_substring("ends_with", values, pattern, ignore_case)


# --------------------------------------------------------------------------- string comparisons
# equal .. less_equal of utf8 / binary operands (CompareKernel on BaseBinaryType, scalar_compare.cc): csrc/string_compare.hip.
# The `path` handed to arx_compare_binary: 0 = the library chooses (rows, or waves from a mean pair size on), 1 = one
# lane per row pair, 2 = one wave per row pair.  Tests set it to reach either form.
STRING_COMPARE_PATH = 0


def _exec_compare_binary(op_name):
    code = _CMP_CODE[op_name]

    def run(args, options):
        """CompareKernel<BinaryType / StringType, Op>::Exec (scalar_compare.cc): array x array, array x scalar, scalar x
        array; one arx_compare_binary call, the validity is the intersection of the operands'."""
        left, right = args
        arrays = [a for a in args if isinstance(a, Array)]
        if not arrays:
            raise ArrowNotImplementedError(f"arrow_amd: {op_name} of two scalars on the device path")
        if len(arrays) == 2 and left.length != right.length:
            raise ArrowInvalid("Array arguments must all be the same length")
        n, dev = arrays[0].length, arrays[0].device
        lib, stream = _lib_and_stream(dev)
        words = alloc(max(1, (n + 63) // 64) * 8, dev, zero=_has_null_scalar(left, right))
        if not _has_null_scalar(left, right):
            dlit, m = None, 0
            for a in args:
                if isinstance(a, Scalar):
                    literal = _literal_operand(op_name, f"a {a.type.name} scalar must hold", a.value)
                    dlit, m = _device_literal(dev, literal), len(literal)
            spans = [a.binary_span() if isinstance(a, Array) else None for a in args]
            hint = builtins.sum(_data_bytes_hint(a) for a in arrays)
            with tracing.span("arx_compare_binary"):
                check(lib.arx_compare_binary(code, *[None if s is None else C.byref(s) for s in spans], 4,
                                             None if dlit is None else dlit.data_ptr(), m, builtins.max(hint, -1),
                                             int(STRING_COMPARE_PATH), words.data_ptr(), stream))
        validity, nc = _propagate_validity([left, right], n, dev)
        out = Array(bool_, n, [validity, words], nc, 0)
        if nc == kUnknownNullCount:
            out.set_lazy_null_count(_lazy_null_count(validity, n))
        return out
    return run


# --------------------------------------------------------------------------- string lengths and slices
# binary_length / utf8_length / binary_slice / utf8_slice_codeunits (compute/kernels/scalar_string_ascii.cc,
# scalar_string_utf8.cc): csrc/string_slice.hip.  The `path` handed to arx_string_length / arx_string_slice_offsets for
# the codepoint walk: 0 = the library chooses (rows, or waves from a mean row size on), 1 = one lane per row, 2 = one
# wave per row.  Tests set it to reach either form.
STRING_SLICE_PATH = 0
# the same for arx_replace_substring_offsets / _data (csrc/string_replace.hip): 0 = the library chooses, 1 = rows, 2 = waves
STRING_REPLACE_PATH = 0
_STRING_UNIT = {"binary_length": 0, "utf8_length": 1, "binary_slice": 0, "utf8_slice_codeunits": 1}
_NO_STOP = 2**63 - 1            # stop = INT64_MAX: to the row's end
_BINARY_ONLY = lambda t: t.name == "binary"  # noqa: E731
_UTF8_ONLY = lambda t: t.name == "string"  # noqa: E731


def _data_bytes_hint(values: Array) -> int:
    return int(values.buffers[2].numel()) if values.buffers[2] is not None else -1


def _exec_string_length(name: str):
    def run(args, options):
        (values,) = args
        _require_array(name, values)
        lib, stream = _lib_and_stream(values.device)
        out = alloc(max(values.length, 1) * 4, values.device)
        vspan = values.binary_span()
        with tracing.span("arx_string_length"):
            check(lib.arx_string_length(C.byref(vspan), 4, _STRING_UNIT[name], _data_bytes_hint(values), int(STRING_SLICE_PATH),
                                        out.data_ptr(), stream))
        return _under_input_validity(values, int32, out)
    return run


def _exec_string_slice(name: str):
    def run(args, options):
        (values,) = args
        _require_array(name, values)
        options = options or SliceOptions(0)
        if options.step == 0:
            raise ArrowInvalid("Slice step cannot be zero")
        if options.step != 1:
            raise ArrowNotImplementedError(f"arrow_amd: {name} with step={options.step} on device-resident arrays: only step=1 has "
                                           "a device kernel")
        clamp = lambda x: max(-2**63, min(int(x), 2**63 - 2))  # noqa: E731  (INT64_MAX itself means "no stop")
        stop = _NO_STOP if options.stop is None else clamp(options.stop)
        return _sub_range_result(values, "arx_string_slice_offsets", lambda lib, vspan, *rest: lib.arx_string_slice_offsets(
            vspan, 4, _STRING_UNIT[name], clamp(options.start), stop, _data_bytes_hint(values), int(STRING_SLICE_PATH), *rest))
    return run


def _slice_data_call(lib, vspan, *rest):
    return lib.arx_string_slice_data(vspan, 4, *rest)


def _sub_range_result(values: Array, span_name: str, offsets_call, data_name: str = "arx_string_slice_data",
                      data_call=_slice_data_call, workspace_bytes: str = "arx_string_slice_workspace_bytes") -> Array:
    """The result of a function whose rows are made from the input's rows, one for one (slices, trims, replace_substring).
    `offsets_call(lib, vspan, ws, ws_bytes, out_offsets, total, stream)` writes the n + 1 offsets and leaves in the
    workspace what `data_call(lib, vspan, ws, ws_bytes, out_offsets, total_bytes, out_data, stream)` needs to write the
    bytes: for a row that is a sub-range of the input's row its source position, and arx_string_slice_data copies.  The
    validity is the input's."""
    dev = values.device
    lib, stream = _lib_and_stream(dev)
    n = values.length
    out_offsets = alloc((n + 1) * 4, dev)
    ws = _workspace(dev, getattr(lib, workspace_bytes)(n, 4), "string_slice")
    total = C.c_int64(0)
    vspan = values.binary_span()
    with tracing.span(span_name):
        check(offsets_call(lib, C.byref(vspan), ws.data_ptr(), ws.numel(), out_offsets.data_ptr(), C.byref(total), stream))
    out_data = alloc(total.value, dev)
    with tracing.span(data_name):
        check(data_call(lib, C.byref(vspan), ws.data_ptr(), ws.numel(), out_offsets.data_ptr(), total.value, out_data.data_ptr(), stream))
    return _under_input_validity(values, values.type, out_offsets, out_data)


def _call_string_function(name: str, values, options, *reference_args) -> Array:
    import pyarrow as pa
    import pyarrow.compute as pc

    if not isinstance(values, Array):
        raise TypeError(f"{name}: values must be an arrow_amd.Array")
    if not _STRING_INPUT[name](values.type):
        # the reference's own "has no kernel matching input types" error, from a zero-length call
        getattr(pc, name)(pa.array([], _pa_type(values.type)), *reference_args)
    return call_function(name, [values], options)


_STRING_INPUT = {"binary_length": is_base_binary, "utf8_length": _UTF8_ONLY, "binary_slice": _BINARY_ONLY,
                 "utf8_slice_codeunits": _UTF8_ONLY, "match_substring": is_base_binary, "starts_with": is_base_binary,
                 "ends_with": is_base_binary, "replace_substring": is_base_binary}


def binary_length(values: Array) -> Array:
    """compute::BinaryLength: int32, the bytes of each row of a utf8 / binary array; null where the row is null.  The
    result stays on the device."""
    return _call_string_function("binary_length", values, None)


def utf8_length(values: Array) -> Array:
    """compute::UTF8Length: int32, the codepoints of each row of a utf8 array (every byte that is not a continuation byte
    counts one, valid UTF-8 or not); null where the row is null.  The result stays on the device."""
    return _call_string_function("utf8_length", values, None)


def binary_slice(values: Array, start: int, stop=None, step: int = 1) -> Array:
    """compute::BinarySlice under SliceOptions: Python's b[start:stop] of each row of a binary array; a null row stays
    null and holds no bytes.  step=0 raises the reference's ArrowInvalid, any other step but 1 ArrowNotImplementedError
    (there is no CPU fallback).  The result stays on the device."""
    return _call_string_function("binary_slice", values, SliceOptions(start, stop, step), 0)


def utf8_slice_codeunits(values: Array, start: int, stop=None, step: int = 1) -> Array:
    """compute::UTF8SliceCodeunits under SliceOptions: Python's s[start:stop] of each row of a utf8 array, counted in
    codepoints.  See binary_slice."""
    return _call_string_function("utf8_slice_codeunits", values, SliceOptions(start, stop, step), 0)


# --------------------------------------------------------------------------- replace_substring
# compute::ReplaceSubstring with a literal pattern (PlainSubstringReplacer, scalar_string_ascii.cc):
# csrc/string_replace.hip.  The rows are assembled, not sub-ranges: arx_replace_substring_offsets counts every row's
# matches, arx_replace_substring_data writes "gap, replacement, gap, ...".
def _exec_replace_substring(args, options):
    name = "replace_substring"
    (values,) = args
    _require_array(name, values)
    if options is None:
        raise ArrowInvalid(f"Function '{name}' cannot be called without options")
    pattern = _literal_operand(name, "pattern must be", options.pattern)
    replacement = _literal_operand(name, "replacement must be", options.replacement)
    if not pattern:
        raise ArrowNotImplementedError(f"arrow_amd: {name} with an empty pattern on device-resident arrays: there is no device "
                                       "kernel (the reference does not terminate on it with unlimited replacements)")
    cap = -1 if options.max_replacements is None or options.max_replacements < 0 else min(int(options.max_replacements), 2**63 - 1)
    m, r = len(pattern), len(replacement)
    literals = _device_literal(values.device, pattern, replacement)   # copied to the device once per call
    dpat, drep = literals.data_ptr(), literals.data_ptr() + m
    path = int(STRING_REPLACE_PATH)
    return _sub_range_result(
        values, "arx_replace_substring_offsets",
        lambda lib, vspan, *rest: lib.arx_replace_substring_offsets(vspan, 4, dpat, m, r, cap, _data_bytes_hint(values), path, *rest),
        "arx_replace_substring_data",
        lambda lib, vspan, *rest: lib.arx_replace_substring_data(vspan, 4, dpat, m, drep, r, cap, path, *rest),
        "arx_replace_substring_workspace_bytes")


def replace_substring(values: Array, pattern, replacement, *, max_replacements=None) -> Array:
    """compute::ReplaceSubstring under ReplaceSubstringOptions: each row of a utf8 / binary array with the non-overlapping
    matches of the literal `pattern` (str, UTF-8 encoded, or bytes), found left to right, replaced by `replacement`;
    max_replacements None or negative replaces all of them, 0 none, k > 0 the first k of each row.  Bytes are bytes; a null
    row stays null and holds no bytes.  The empty pattern raises ArrowNotImplementedError (there is no CPU fallback); a
    result past int32 offsets raises ArrowInvalid ("offset overflow").  The result stays on the device."""
    return _call_string_function("replace_substring", values, ReplaceSubstringOptions(pattern, replacement, max_replacements), "x", "y")


# --------------------------------------------------------------------------- binary_join_element_wise
# compute::BinaryJoinElementWise under JoinOptions (scalar_string_ascii.cc): csrc/string_join.hip.  Every operand, the
# separator (the last) included, is an Array, a valid Scalar (a literal) or a null Scalar.  arx_binary_join_offsets makes
# the offsets, the validity and the null count from the operands' offsets and validity bits, arx_binary_join_data gathers
# the bytes.
def _exec_binary_join_element_wise(args, options):
    name = "binary_join_element_wise"
    options = options if options is not None else JoinOptions()
    arrays = [a for a in args if isinstance(a, Array)]
    if not arrays:
        raise ArrowNotImplementedError(f"arrow_amd: {name} of scalars only on the device path")
    n, dev, out_type = arrays[0].length, arrays[0].device, arrays[0].type
    if any(a.length != n for a in arrays):
        raise ArrowInvalid("Array arguments must all be the same length")
    replacement = _literal_operand(name, "null_replacement must be", options.null_replacement)
    parts = [replacement] + [_literal_operand(name, f"a {a.type.name} scalar must hold", a.value) if isinstance(a, Scalar) and a.is_valid
                             else b"" for a in args]
    literals = _device_literal(dev, *parts)                         # copied to the device once per call
    at = literals.data_ptr() + len(replacement)
    operands = (_lib.ArxJoinOperand * len(args))()
    for op, a, part in zip(operands, args, parts[1:]):
        if isinstance(a, Array):
            op.kind, op.column = _lib.JOIN_COLUMN, a.binary_span()
        elif a.is_valid:
            op.kind, op.literal, op.literal_length = _lib.JOIN_LITERAL, at if part else None, len(part)
        else:
            op.kind = _lib.JOIN_NULL
        at += len(part)
    mode = _lib.JOIN_NULL_HANDLING[options.null_handling]
    lib, stream = _lib_and_stream(dev)
    out_offsets = alloc((n + 1) * 4, dev)
    out_valid = alloc(max(1, (n + 63) // 64) * 8, dev)
    ws = _workspace(dev, lib.arx_binary_join_workspace_bytes(n, 4), "string_slice")
    total, nulls = C.c_int64(0), C.c_int64(0)
    with tracing.span("arx_binary_join_offsets"):
        check(lib.arx_binary_join_offsets(operands, len(args), n, 4, mode, len(replacement), ws.data_ptr(), ws.numel(),
                                          out_offsets.data_ptr(), out_valid.data_ptr(), C.byref(nulls), C.byref(total), stream))
    out_data = alloc(total.value, dev)
    with tracing.span("arx_binary_join_data"):
        check(lib.arx_binary_join_data(operands, len(args), n, 4, mode, literals.data_ptr() if replacement else None, len(replacement),
                                       out_offsets.data_ptr(), total.value, out_data.data_ptr(), stream))
    return Array(out_type, n, [out_valid if nulls.value else None, out_offsets, out_data], nulls.value, 0)


def binary_join_element_wise(*operands, null_handling: str = "emit_null", null_replacement="") -> Array:
    """compute::BinaryJoinElementWise under JoinOptions: row i of the result is operands[0][i], sep[i], operands[1][i], ...
    with the LAST operand as the separator.  An operand is an Array (utf8 or binary, all of one type and length), a str
    (a utf8 literal), bytes (a binary literal), a Scalar or None (a null literal of the arrays' type); at least one is an
    Array.  A null separator makes the row null; null_handling says what a null value does: "emit_null" (the row is null),
    "skip" (it is left out with one separator) or "replace" (it contributes `null_replacement`).  Bytes are bytes.  Not the
    reference's: under "skip" a row whose values are all null is the empty string, where Arrow 25.0.0 drops the row.  More
    than 32 operands raise ArrowNotImplementedError (there is no CPU fallback); a result past int32 offsets raises
    ArrowInvalid ("offset overflow").  The result stays on the device and has no bitmap when no row is null."""
    from .array import type_from_name

    name = "binary_join_element_wise"
    arrays = [a for a in operands if isinstance(a, Array)]
    if not arrays:
        raise TypeError(f"{name}: at least one operand must be an arrow_amd.Array")
    args = []
    for a in operands:
        if isinstance(a, str):
            a = Scalar(a, type_from_name("string"), True)
        elif isinstance(a, (bytes, bytearray, memoryview)):
            a = Scalar(bytes(a), type_from_name("binary"), True)
        elif a is None:
            a = Scalar(None, arrays[0].type, False)
        elif not isinstance(a, (Array, Scalar)):
            raise TypeError(f"{name}: an operand must be an Array, str, bytes, Scalar or None, not {type(a).__name__}")
        args.append(a)
    return call_function(name, args, JoinOptions(null_handling, null_replacement))


# --------------------------------------------------------------------------- string trimming
# {ascii,utf8}_{,l,r}trim and their _whitespace forms (compute/kernels/scalar_string_ascii.cc, scalar_string_utf8.cc):
# csrc/string_trim.hip writes the offsets, the copy is the slices' arx_string_slice_data.  name -> (sides, set kind) of
# arx_string_trim_offsets; the set kinds 2 (bytes) and 3 (codepoints) take TrimOptions.
_TRIM_SIDES = {"trim": 3, "ltrim": 1, "rtrim": 2}
_TRIMS = {f"{enc}_{side}{ws}": (_TRIM_SIDES[side], {("ascii", "_whitespace"): 0, ("utf8", "_whitespace"): 1, ("ascii", ""): 2,
                                                    ("utf8", ""): 3}[enc, ws])
          for enc in ("ascii", "utf8") for side in _TRIM_SIDES for ws in ("_whitespace", "")}
TRIM_MAX_CODEPOINTS = 64        # ARX_TRIM_MAX_CODEPOINTS: distinct codepoints the device kernel takes as arguments


def _utf8_codepoints(raw: bytes):
    """The codepoints of `raw` as the reference's UTF8Decode reads them (lead and continuation bits only), or its
    ArrowInvalid."""
    out, i = [], 0
    while i < len(raw):
        lead = raw[i]
        extra = 0 if lead < 0x80 else 1 if 0xC0 <= lead < 0xE0 else 2 if 0xE0 <= lead < 0xF0 else 3 if 0xF0 <= lead < 0xF8 else None
        tail = raw[i + 1: i + 1 + (extra or 0)]
        if extra is None or len(tail) != extra or any((x & 0xC0) != 0x80 for x in tail):
            raise ArrowInvalid("Invalid UTF8 sequence in input")
        v = lead if extra == 0 else lead & (0xFF >> (extra + 2))
        for x in tail:
            v = (v << 6) | (x & 0x3F)
        out.append(v)
        i += 1 + extra
    return out


def _exec_string_trim(name: str):
    sides, kind = _TRIMS[name]

    def run(args, options):
        (values,) = args
        _require_array(name, values)
        members, count = None, 0
        if kind >= 2:
            if options is None:
                raise ArrowInvalid(f"Function '{name}' cannot be called without options")
            raw = options.characters.encode() if isinstance(options.characters, str) else bytes(options.characters)
            if kind == 2:
                members, count = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0"), len(raw)
            else:
                codepoints = _utf8_codepoints(raw)
                if len(set(codepoints)) > TRIM_MAX_CODEPOINTS:
                    raise ArrowNotImplementedError(f"arrow_amd: {name} with {len(set(codepoints))} distinct characters on device-resident "
                                                   f"arrays: the device kernel takes up to {TRIM_MAX_CODEPOINTS}")
                members, count = (C.c_uint32 * max(len(codepoints), 1))(*codepoints), len(codepoints)
        return _sub_range_result(values, "arx_string_trim_offsets", lambda lib, vspan, *rest: lib.arx_string_trim_offsets(
            vspan, 4, sides, kind, C.cast(members, C.c_void_p) if members is not None else None, count, *rest))
    return run


def _make_trim(name: str):
    if _TRIMS[name][1] < 2:
        def trim(values: Array) -> Array:
            return _call_string_function(name, values, None)
    else:
        def trim(values: Array, characters) -> Array:
            return _call_string_function(name, values, TrimOptions(characters), characters)
    trim.__name__ = trim.__qualname__ = name
    what = {1: "front", 2: "back", 3: "front and back"}[_TRIMS[name][0]]
    of = ("ASCII whitespace bytes (9 .. 13, 32)", "Unicode whitespace codepoints", "bytes of `characters`",
          "codepoints of `characters`")[_TRIMS[name][1]]
    trim.__doc__ = (f"compute::{name}: each row of a utf8 array without the {of} at its {what}; a null row stays null and holds no "
                    "bytes.  The result stays on the device.")
    return trim


for _name in _TRIMS:
    globals()[_name] = _make_trim(_name)
    _STRING_INPUT[_name] = _UTF8_ONLY
del _name


# --------------------------------------------------------------------------- if_else
# if_else(cond, left, right) (compute/kernels/scalar_if_else.cc, IfElseFunctor): csrc/if_else.hip.  The reference's
# DispatchBest casts the operands to a common type; the mirror has no implicit casts: both sides are of one type.
_IF_ELSE_VALUE = lambda t: t == bool_ or (t.np_dtype is not None and t.byte_width in (1, 2, 4, 8))  # noqa: E731


def _exec_if_else(args, options):
    cond, left, right = args
    if not isinstance(cond, Array):
        raise ArrowNotImplementedError("arrow_amd: if_else with a scalar cond on device-resident arrays")
    t = left.type
    if right.type != t:
        raise ArrowNotImplementedError(f"if_else: left is {t.name}, right is {right.type.name}; the device kernel takes both sides "
                                       "of one type (no implicit casts)")
    n = cond.length
    if any(isinstance(a, Array) and a.length != n for a in (left, right)):
        raise ArrowInvalid("Array arguments must all be the same length")
    dev = cond.device
    lib, stream = _lib_and_stream(dev)
    width = 0 if t == bool_ else t.byte_width
    keep = []

    def operand(x):
        """(span pointer | None, host scalar pointer | None) as arx_if_else takes an operand."""
        if isinstance(x, Array):
            keep.append(x.span())
            return C.byref(keep[-1]), None
        if not x.is_valid:
            return None, None
        holder = np.zeros(1, dtype=np.uint8 if width == 0 else t.np_dtype)
        holder[0] = bool(x.value) if width == 0 else t.np_dtype.type(x.value)
        keep.append(holder)
        return None, holder.ctypes.data

    null_scalars = [isinstance(a, Scalar) and not a.is_valid for a in (left, right)]
    nulls = any(null_scalars) or any(isinstance(a, Array) and a.may_have_nulls() for a in args)
    out = alloc(bitmap_nbytes(n) if width == 0 else n * width, dev)
    valid = alloc(bitmap_nbytes(n), dev) if nulls else None
    cspan = cond.span()
    (lspan, lsc), (rspan, rsc) = operand(left), operand(right)
    with tracing.span("arx_if_else"):
        check(lib.arx_if_else(width, C.byref(cspan), lspan, lsc, rspan, rsc, n, out.data_ptr(), _ptr_or_none(valid), stream))
    if not nulls:
        return Array(t, n, [None, out], 0, 0)
    res = Array(t, n, [valid, out], kUnknownNullCount, 0)
    if all(null_scalars):
        res._null_count = n
    else:
        res.set_lazy_null_count(_lazy_null_count(valid, n))
    return res


def if_else(cond: Array, left, right) -> Array:
    """compute::IfElse (scalar_if_else.cc): out[i] = left[i] where cond[i] is true, right[i] where it is false, null where
    cond is null; a slot takes the validity of the side it comes from.  cond: a boolean Array.  left / right: an Array, an
    arrow_amd.Scalar, a Python number or bool (it takes the other side's type) or None (a null scalar); both of one type —
    boolean or 1 / 2 / 4 / 8 bytes wide, temporal types included — since the mirror casts nothing implicitly.  The result
    stays on the device and has no validity buffer when no operand can be null."""
    if not isinstance(cond, Array) or cond.type != bool_:
        got = cond.type.name if isinstance(cond, (Array, Scalar)) else type(cond).__name__
        raise ArrowNotImplementedError(f"if_else: cond must be a boolean arrow_amd.Array, not {got}")
    typed = [x.type for x in (left, right) if isinstance(x, (Array, Scalar))]
    if not typed:
        raise ArrowNotImplementedError(f"if_else: neither left ({left!r}) nor right ({right!r}) carries a type; pass an Array or an "
                                       "arrow_amd.Scalar on one side")
    wrap = lambda x: x if isinstance(x, (Array, Scalar)) else Scalar(x, typed[0], x is not None)  # noqa: E731
    return call_function("if_else", [cond, wrap(left), wrap(right)])


# --------------------------------------------------------------------------- case_when
# case_when(conds, v_0 .. v_{k-1} [, else]) (compute/kernels/scalar_if_else.cc, CaseWhenFunctor): csrc/case_when.hip.
# As for if_else there are no implicit casts: every value is of one type.
def _operand_holder(x: Scalar, t: DataType):
    """The host bytes of a valid scalar as the C ABI takes them (booleans: one byte 0 / 1)."""
    holder = np.zeros(1, dtype=np.uint8 if t == bool_ else t.np_dtype)
    holder[0] = bool(x.value) if t == bool_ else t.np_dtype.type(x.value)
    return holder


def _operand_table(operands, t: DataType, keep: list):
    """ArxOperand[len(operands)] of Arrays and Scalars of type t; `keep` holds what the pointers refer to."""
    table = (_lib.ArxOperand * len(operands))()
    for j, x in enumerate(operands):
        if isinstance(x, Array):
            keep.append(x.span())
            table[j].span = C.pointer(keep[-1])
        elif x.is_valid:
            keep.append(_operand_holder(x, t))
            table[j].scalar = keep[-1].ctypes.data
    return table


def _typed_operands(name: str, values, what: str):
    """values with every Python number, bool or None made a Scalar of the type the typed operands carry."""
    typed = [x.type for x in values if isinstance(x, (Array, Scalar))]
    if not typed:
        raise ArrowNotImplementedError(f"{name}: none of the {what} ({', '.join(repr(x) for x in values)}) carries a type; pass an Array "
                                       "or an arrow_amd.Scalar as one of them")
    return [x if isinstance(x, (Array, Scalar)) else Scalar(x, typed[0], x is not None) for x in values]


def _one_type(name: str, values, what: str) -> DataType:
    t = values[0].type
    for j, x in enumerate(values):
        if x.type != t:
            raise ArrowNotImplementedError(f"{name}: {what} 0 is {t.name}, {what} {j} is {x.type.name}; the device kernel takes every "
                                           f"{what} of one type (no implicit casts)")
    return t


_CASE_WHEN_TOP_LEVEL_NULLS = "cond struct must not be a null scalar or have top-level nulls"


def case_when(conds, *values) -> Array:
    """compute::CaseWhen (scalar_if_else.cc): row i takes values[j][i] of the first j whose conds[j][i] is true and valid (a
    null cond is false); a row no cond takes comes from the else — the value after the last cond's, if given — or is null.
    conds: a list or tuple of 1 .. 16 boolean Arrays (or a StructArray whose children they are).  values: as many as conds,
    or one more; each an Array, an arrow_amd.Scalar, a Python number or bool (it takes the other values' type) or None (a
    null scalar); all of one type — boolean or 1 / 2 / 4 / 8 bytes wide, temporal types included — since the mirror casts
    nothing implicitly.  The result stays on the device and has no validity buffer when it cannot hold a null."""
    from .array import StructArray

    if conds is None or isinstance(conds, Scalar):
        raise ArrowInvalid(_CASE_WHEN_TOP_LEVEL_NULLS)
    if isinstance(conds, StructArray):
        if conds.buffers[0] is not None and conds.null_count != 0:
            raise ArrowInvalid(_CASE_WHEN_TOP_LEVEL_NULLS)
        conds = conds.children
    if not isinstance(conds, (list, tuple)):
        raise ArrowNotImplementedError(f"case_when: conds must be a list of boolean arrow_amd.Arrays, not {type(conds).__name__}")
    conds = list(conds)
    for c in conds:
        if not isinstance(c, Array) or c.type != bool_:
            got = c.type.name if isinstance(c, (Array, Scalar)) else type(c).__name__
            raise ArrowNotImplementedError(f"case_when: every cond must be a boolean arrow_amd.Array, not {got}")
    if not values:
        raise ArrowInvalid("VarArgs function 'case_when' needs at least 2 arguments but only 1 passed")
    if len(values) not in (len(conds), len(conds) + 1) or not conds:
        raise ArrowInvalid("case_when: number of struct fields must be equal to or one less than count of remaining arguments "
                           f"({len(values)}), got: {len(conds)}")
    values = _typed_operands("case_when", values, "values")
    t = _one_type("case_when", values, "value")
    if not _IF_ELSE_VALUE(t):
        names = ", ".join([f"struct<{', '.join(['bool'] * len(conds))}>"] + [x.type.name for x in values])
        raise ArrowNotImplementedError(f"Function 'case_when' has no kernel matching input types ({names})")
    if len(conds) > _lib.CASE_WHEN_MAX_CONDS:
        raise ArrowNotImplementedError(f"arrow_amd: case_when with {len(conds)} conds on device-resident arrays: the device kernel "
                                       f"takes up to {_lib.CASE_WHEN_MAX_CONDS}")
    n = conds[0].length
    if any(isinstance(a, Array) and a.length != n for a in conds + values):
        raise ArrowInvalid("Array arguments must all be the same length")
    dev = conds[0].device
    lib, stream = _lib_and_stream(dev)
    width = 0 if t == bool_ else t.byte_width
    keep = []
    cspans = [c.span() for c in conds]
    ctable = (C.POINTER(_lib.ArxSpan) * len(conds))(*[C.pointer(sp) for sp in cspans])
    vtable = _operand_table(values, t, keep)
    null_scalars = [isinstance(a, Scalar) and not a.is_valid for a in values]
    nulls = len(values) == len(conds) or any(null_scalars) or any(isinstance(a, Array) and a.may_have_nulls() for a in values)
    out = alloc(bitmap_nbytes(n) if width == 0 else n * width, dev)
    valid = alloc(bitmap_nbytes(n), dev) if nulls else None
    with tracing.span("arx_case_when"):
        check(lib.arx_case_when(width, ctable, len(conds), vtable, len(values), n, out.data_ptr(), _ptr_or_none(valid), stream))
    if not nulls:
        return Array(t, n, [None, out], 0, 0)
    res = Array(t, n, [valid, out], kUnknownNullCount, 0)
    if all(null_scalars):
        res._null_count = n
    else:
        res.set_lazy_null_count(_lazy_null_count(valid, n))
    return res


# --------------------------------------------------------------------------- min_element_wise / max_element_wise
# MinMaxFunctor / ScalarMinMax (compute/kernels/scalar_compare.cc): csrc/element_wise.hip.  One type for every operand (the
# reference's DispatchBest casts; the mirror casts nothing).
_ELEMENT_WISE_OPS = {"min_element_wise": _lib.ELEMENT_WISE_MIN, "max_element_wise": _lib.ELEMENT_WISE_MAX}


def _ELEMENT_WISE_VALUE(t: DataType) -> bool:
    from .array import is_temporal

    return t.name in _NUM_TYPE_ID or is_temporal(t)


def _exec_min_max_element_wise(name: str):
    def run(args, options):
        t = _one_type(name, args, "operand")
        if len(args) > _lib.ELEMENT_WISE_MAX_OPERANDS:
            raise ArrowNotImplementedError(f"arrow_amd: {name} with {len(args)} operands on device-resident arrays: the device kernel "
                                           f"takes up to {_lib.ELEMENT_WISE_MAX_OPERANDS}")
        arrays = [a for a in args if isinstance(a, Array)]
        if not arrays:
            raise ArrowNotImplementedError(f"arrow_amd: {name} of scalars only; pass an arrow_amd.Array as one of the operands")
        n = arrays[0].length
        if any(a.length != n for a in arrays):
            raise ArrowInvalid("Array arguments must all be the same length")
        skip_nulls = bool(options.skip_nulls)
        dev = arrays[0].device
        lib, stream = _lib_and_stream(dev)
        keep = []
        table = _operand_table(args, t, keep)
        nullable = [a.may_have_nulls() if isinstance(a, Array) else not a.is_valid for a in args]
        nulls = all(nullable) if skip_nulls else any(nullable)
        out = alloc(n * t.byte_width, dev)
        valid = alloc(bitmap_nbytes(n), dev) if nulls else None
        with tracing.span("arx_min_max_element_wise"):
            check(lib.arx_min_max_element_wise(_num_type_id(t), _ELEMENT_WISE_OPS[name], 1 if skip_nulls else 0, table, len(args), n,
                                               out.data_ptr(), _ptr_or_none(valid), stream))
        if not nulls:
            return Array(t, n, [None, out], 0, 0)
        res = Array(t, n, [valid, out], kUnknownNullCount, 0)
        null_scalar = any(isinstance(a, Scalar) and not a.is_valid for a in args)
        if null_scalar and not skip_nulls:
            res._null_count = n
        else:
            res.set_lazy_null_count(_lazy_null_count(valid, n))
        return res
    return run


def _make_element_wise(name: str):
    def fn(*args, skip_nulls: bool = True) -> Array:
        if not args:
            return call_function(name, [], ElementWiseAggregateOptions(skip_nulls))
        return call_function(name, _typed_operands(name, args, "operands"), ElementWiseAggregateOptions(skip_nulls))
    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = (f"compute::{'Min' if name.startswith('min') else 'Max'}ElementWise (scalar_compare.cc): the row-wise "
                  f"{'smallest' if name.startswith('min') else 'largest'} of 1 .. 32 operands of one numeric type (or a temporal one that "
                  "is physically int32 / int64).  Each operand: an Array, an arrow_amd.Scalar, a Python number (it takes the other "
                  "operands' type) or None (a null scalar).  skip_nulls: null only where every operand is null; otherwise where any is.  "
                  "The fold is the reference's (scalars first, then the arrays left to right; a NaN loses to every number).  The "
                  "result stays on the device and has no validity buffer when it cannot hold a null.")
    return fn


for _name in _ELEMENT_WISE_OPS:
    globals()[_name] = _make_element_wise(_name)
del _name


# --------------------------------------------------------------------------- date / time fields
# Year .. ISOWeek, Hour .. Nanosecond (compute/kernels/scalar_temporal_unary.cc): csrc/temporal.hip.  name -> ARX_TEMPORAL_*
_TEMPORAL_COMPONENTS = {"year": 0, "quarter": 1, "month": 2, "day": 3, "day_of_week": 4, "day_of_year": 5, "iso_year": 6,
                        "iso_week": 7, "hour": 8, "minute": 9, "second": 10, "millisecond": 11, "microsecond": 12,
                        "nanosecond": 13}
# type name (a timestamp's without its zone) -> ARX_TIME_*
_TEMPORAL_INPUTS = {"date32[day]": 0, "date64[ms]": 1, "timestamp[s]": 2, "timestamp[ms]": 3, "timestamp[us]": 4,
                    "timestamp[ns]": 5, "time32[s]": 6, "time32[ms]": 7, "time64[us]": 8, "time64[ns]": 9}


def _without_zone(name: str) -> str:
    """A type's name without a timestamp's zone: timestamp[us, tz=UTC] -> timestamp[us]."""
    unit, sep, _ = name.partition(", tz=")
    return unit + "]" if sep else name


def _temporal_input_code(t: DataType):
    return _TEMPORAL_INPUTS.get(_without_zone(t.name))


def _temporal_input(name: str):
    """The reference's kernel lists: calendar fields take dates and timestamps, time-of-day fields timestamps and times
    (a timestamp matches by unit whatever its zone; the exec refuses a zone)."""
    calendar = _TEMPORAL_COMPONENTS[name] <= 7

    def matches(t: DataType) -> bool:
        code = _temporal_input_code(t)
        return code is not None and (code <= 5 if calendar else code >= 2)
    return matches


def _exec_temporal(name: str):
    component = _TEMPORAL_COMPONENTS[name]

    def run(args, options):
        (values,) = args
        _require_array(name, values)
        if _without_zone(values.type.name) != values.type.name:
            raise ArrowNotImplementedError(f"arrow_amd: {name} of {values.type.name} on device-resident arrays: time zones need "
                                           "the tz database, which has no device kernel")
        options = options or DayOfWeekOptions()
        week_start, count_from_zero = (options.week_start, options.count_from_zero) if name == "day_of_week" else (1, True)
        if not 1 <= week_start <= 7:
            raise ArrowInvalid(f"week_start must follow ISO convention (Monday=1, Sunday=7). Got week_start={week_start}")
        n = values.length
        dev = values.device
        lib, stream = _lib_and_stream(dev)
        nulls = _input_has_nulls(values)
        vspan = _unary_span(values)
        out = alloc(n * 8, dev)
        valid = alloc(bitmap_nbytes(n), dev) if nulls else None   # (the kernel writes the validity at offset 0 itself)
        with tracing.span("arx_temporal_component"):
            check(lib.arx_temporal_component(component, _temporal_input_code(values.type), C.byref(vspan), n, week_start,
                                             1 if count_from_zero else 0, out.data_ptr(), _ptr_or_none(valid), stream))
        if not nulls:
            return Array(int64, n, [None, out], 0, 0)
        return _carry_null_count(Array(int64, n, [valid, out], kUnknownNullCount, 0), values)
    return run


_TEMPORAL_DOC = ("compute::{} (scalar_temporal_unary.cc): an int64 Array on the device, null where `values` is null (no validity "
                 "buffer when `values` has none; the null count is the input's).  Proleptic Gregorian calendar, floor division "
                 "before the epoch, no time zones (a zoned timestamp raises ArrowNotImplementedError).")
year = _values_wrapper("year", _TEMPORAL_DOC, "Year")
quarter = _values_wrapper("quarter", _TEMPORAL_DOC, "Quarter")
month = _values_wrapper("month", _TEMPORAL_DOC, "Month")
day = _values_wrapper("day", _TEMPORAL_DOC, "Day")
day_of_year = _values_wrapper("day_of_year", _TEMPORAL_DOC, "DayOfYear")
iso_year = _values_wrapper("iso_year", _TEMPORAL_DOC, "ISOYear")
iso_week = _values_wrapper("iso_week", _TEMPORAL_DOC, "ISOWeek")
hour = _values_wrapper("hour", _TEMPORAL_DOC, "Hour")
minute = _values_wrapper("minute", _TEMPORAL_DOC, "Minute")
second = _values_wrapper("second", _TEMPORAL_DOC, "Second")
millisecond = _values_wrapper("millisecond", _TEMPORAL_DOC, "Millisecond")
microsecond = _values_wrapper("microsecond", _TEMPORAL_DOC, "Microsecond")
nanosecond = _values_wrapper("nanosecond", _TEMPORAL_DOC, "Nanosecond")


def day_of_week(values: Array, *, count_from_zero: bool = True, week_start: int = 1) -> Array:
    """compute::DayOfWeek: (ISO weekday - week_start + 7) % 7, plus 1 unless count_from_zero; Monday = 0 at the defaults.
    week_start outside 1 .. 7 raises ArrowInvalid with the reference's text.  See year."""
    return call_function("day_of_week", [values], DayOfWeekOptions(count_from_zero, week_start))


# --------------------------------------------------------------------------- one-operand arithmetic and rounding
# Negate .. Sign (base_arithmetic_internal.h), Floor / Ceil / Trunc / Round / RoundToMultiple (scalar_round.cc):
# csrc/unary_arith.hip.  name -> (ARX_UNARY_*, checked)
_UNARY_OPS = {"negate": (0, False), "negate_checked": (0, True), "abs": (1, False), "abs_checked": (1, True), "sign": (2, False),
              "floor": (3, False), "ceil": (4, False), "trunc": (5, False)}
_ROUND_KINDS = {"round": 0, "round_to_multiple": 1}
_NUM_NP_DTYPE = {"int8": np.int8, "uint8": np.uint8, "int16": np.int16, "uint16": np.uint16, "int32": np.int32, "uint32": np.uint32,
                 "int64": np.int64, "uint64": np.uint64, "float": np.float32, "double": np.float64}
_FLOATING = lambda t: t.name in ("float", "double")  # noqa: E731
_SIGNED_OR_FLOATING = lambda t: t.name in _NUM_TYPE_ID and not t.name.startswith("u")  # noqa: E731


def _unary_input(name: str):
    """The reference's kernel lists: negate_checked has no unsigned kernels, floor / ceil / trunc only the two float ones
    (its DispatchBest casts an integer column to double first; the mirror casts nothing implicitly)."""
    return _SIGNED_OR_FLOATING if name == "negate_checked" else _FLOATING if name in ("floor", "ceil", "trunc") else _NUMERIC


def _exec_unary_arith(name: str):
    op, checked = _UNARY_OPS[name]

    def run(args, options):
        (values,) = args
        _require_array(name, values)
        t = values.type
        integral = not _FLOATING(t)
        out_type = int8 if name == "sign" and integral else t
        can_fail = checked and integral and not t.name.startswith("u")
        n = values.length
        dev = values.device
        lib, stream = _lib_and_stream(dev)
        out = alloc(max(n * out_type.byte_width, 8), dev)
        errors = torch.zeros(1, dtype=torch.int64, device=dev) if can_fail else None
        vspan = _unary_span(values)
        with tracing.span("arx_unary_numeric"):
            check(lib.arx_unary_numeric(op, 1 if checked else 0, _NUM_TYPE_ID[t.name], C.byref(vspan), out.data_ptr(),
                                        None if errors is None else errors.data_ptr(), stream))
        if errors is not None and int(errors.cpu()[0]) != 0:
            raise ArrowInvalid("overflow")   # NegateChecked / AbsoluteValueChecked::Call
        return _under_input_validity(values, out_type, out)
    return run


def _round_multiple_as(multiple, t: DataType):
    """RoundToMultipleOptions::multiple cast to the column's type, with the reference's cast errors (a Python int is an
    int64 scalar there, a Python float a double)."""
    if isinstance(multiple, Scalar):
        multiple = multiple.value if multiple.is_valid else None
    if multiple is None:
        raise ArrowInvalid("Rounding multiple must be non-null and valid")
    if not multiple > 0:      # (the reference looks at the sign before it casts: -2 for a uint32 column is this error)
        raise ArrowInvalid("Rounding multiple must be positive")
    dtype = _NUM_NP_DTYPE[t.name]
    if _FLOATING(t):
        with np.errstate(over="ignore"):
            return np.array([multiple], dtype=np.float64).astype(dtype)
    info = np.iinfo(dtype)
    if isinstance(multiple, (float, np.floating)):
        if multiple != multiple or multiple in (float("inf"), float("-inf")) or int(multiple) != multiple or not info.min <= int(multiple) <= info.max:
            raise ArrowInvalid(f"Float value {float(multiple):f} was truncated converting to {t.name}")
    elif not info.min <= int(multiple) <= info.max:
        raise ArrowInvalid(f"Integer value {int(multiple)} not in range: {info.min} to {info.max}")
    return np.array([int(multiple)], dtype=dtype)


def _exec_round(name: str):
    kind = _ROUND_KINDS[name]

    def run(args, options):
        (values,) = args
        _require_array(name, values)
        options = options or (RoundOptions() if kind == 0 else RoundToMultipleOptions())
        t = values.type
        mode = _ROUND_MODES.index(options.round_mode)
        ndigits, multiple = (int(options.ndigits), None) if kind == 0 else (0, _round_multiple_as(options.multiple, t))
        n = values.length
        dev = values.device
        lib, stream = _lib_and_stream(dev)
        out = alloc(max(n * t.byte_width, 8), dev)
        errors = torch.zeros(1, dtype=torch.int64, device=dev)
        vspan = _unary_span(values)
        call = (kind, mode, _NUM_TYPE_ID[t.name], C.byref(vspan), ndigits, None if multiple is None else multiple.ctypes.data)
        with tracing.span("arx_round_numeric"):
            check(lib.arx_round_numeric(*call, out.data_ptr(), errors.data_ptr(), stream))
            check(lib.arx_round_status(*call, errors.data_ptr(), stream))
        return _under_input_validity(values, t, out)
    return run


_UNARY_DOC = ("compute::{}: an Array on the device, null where `values` is null (no validity buffer when `values` has none; the "
              "null count is the input's).  See csrc/unary_arith.hip for the semantics.")
negate = _values_wrapper("negate", _UNARY_DOC, "Negate (integers wrap: negate(uint8 1) == 255)")
negate_checked = _values_wrapper("negate_checked", _UNARY_DOC, "NegateChecked (the signed minimum in a valid slot raises ArrowInvalid 'overflow')")
abs = _values_wrapper("abs", _UNARY_DOC, "AbsoluteValue (abs(int8 -128) == -128)")  # noqa: A001
abs_checked = _values_wrapper("abs_checked", _UNARY_DOC, "AbsoluteValueChecked (the signed minimum in a valid slot raises ArrowInvalid 'overflow')")
sign = _values_wrapper("sign", _UNARY_DOC, "Sign (int8 for an integer column, the same float type for a float one)")
floor = _values_wrapper("floor", _UNARY_DOC, "Floor (float32 / float64)")
ceil = _values_wrapper("ceil", _UNARY_DOC, "Ceil (float32 / float64)")
trunc = _values_wrapper("trunc", _UNARY_DOC, "Trunc (float32 / float64)")


def round(values: Array, ndigits: int = 0, round_mode: str = "half_to_even") -> Array:  # noqa: A001
    """compute::Round (scalar_round.cc): the reference's IEEE operations one by one for floats, its `%` rule for integers
    (ndigits >= 0 returns an integer column as it is).  A row that overflows raises ArrowInvalid with the reference's
    text, naming the last failing row; an integer multiple above half the type's maximum in a half_* mode raises
    ArrowNotImplementedError."""
    return call_function("round", [values], RoundOptions(ndigits, round_mode))


def round_to_multiple(values: Array, multiple=1.0, round_mode: str = "half_to_even") -> Array:
    """compute::RoundToMultiple: `multiple` (a Python number or an arrow_amd.Scalar) is cast to the column's type with the
    reference's cast errors; it must be valid and positive.  See round."""
    return call_function("round_to_multiple", [values], RoundToMultipleOptions(multiple, round_mode))


# --------------------------------------------------------------------------- hash join
# The equi-join of HashJoinNode (acero/hash_join_node.cc): key rows -> ids through the Grouper (right input consumed,
# left input looked up), then csrc/hash_join.hip: group offsets, probe count (the one read-back), expand, and the
# build-side mask for right semi / anti and the right-only tail of right / full outer joins.
JOIN_TYPES = ("left semi", "right semi", "left anti", "right anti", "inner", "left outer", "right outer", "full outer")
# Output rows a join may produce before arx_hash_join_probe_count refuses it with a capacity error (two int64 index
# arrays of this many rows are allocated next).  None: what the device's free memory holds.
HASH_JOIN_MAX_OUTPUT_ROWS = None


def _join_type_code(join_type) -> int:
    if isinstance(join_type, int):
        if 0 <= join_type < len(JOIN_TYPES):
            return join_type
    elif str(join_type).lower().replace("_", " ") in JOIN_TYPES:
        return JOIN_TYPES.index(str(join_type).lower().replace("_", " "))
    raise ArrowInvalid(f"hash join: unknown join type {join_type!r}; one of {', '.join(JOIN_TYPES)}")


def _as_device_key(a, device):
    if isinstance(a, Array):
        return a
    import pyarrow as pa

    if isinstance(a, pa.ChunkedArray):
        a = a.combine_chunks() if a.num_chunks else pa.array([], a.type)
    if isinstance(a, pa.Array) and pa.types.is_dictionary(a.type):
        raise ArrowNotImplementedError(f"hash join on the device: dictionary keys ({a.type}) are not supported")
    try:
        return Array.from_pyarrow(a, device=device)
    except (KeyError, ArrowNotImplementedError):
        raise ArrowNotImplementedError(f"hash join on the device: keys of type {a.type}") from None


def _bool_key(a: Array) -> Array:
    """A boolean key column as one byte per row (the Grouper's fixed-width form), same validity and offset."""
    lib, stream = _lib_and_stream(a.device)
    out = alloc(max(1, a.offset + a.length), a.device)
    span = a.span()
    check(lib.arx_hash_join_bool_key(C.byref(span), out.data_ptr() + a.offset, stream))
    return Array(uint8, a.length, [a.buffers[0], out], a.null_count, a.offset)


def _zero_column(t: DataType, n: int, device) -> Array:
    return Array(t, n, [None, alloc(max(1, n) * t.byte_width, device, zero=True)], 0, 0)


def _join_key_columns(left_keys, right_keys):
    """Each key pair as the Grouper's fixed-width columns, the same list of types on both sides: fixed-width keys as
    they are (compared by their bits), booleans as bytes, utf8 / binary as (length, 12-byte chunks) with the shorter
    side's missing chunks zero, which is what its own zero padding would hold."""
    lcols, rcols = [], []
    for a, b in zip(left_keys, right_keys):
        if a.type != b.type:
            raise ArrowInvalid(f"hash join: key types differ: {a.type.name} on the left, {b.type.name} on the right")
        t = a.type
        if is_base_binary(t):
            (la, ca), (lb, cb) = binary_key_columns(a), binary_key_columns(b)
            for _ in range(len(ca), len(cb)):
                ca.append((_zero_column(uint64, a.length, a.device), _zero_column(uint32, a.length, a.device)))
            for _ in range(len(cb), len(ca)):
                cb.append((_zero_column(uint64, b.length, b.device), _zero_column(uint32, b.length, b.device)))
            lcols += [la] + [c for pair in ca for c in pair]
            rcols += [lb] + [c for pair in cb for c in pair]
        elif t == bool_:
            lcols.append(_bool_key(a))
            rcols.append(_bool_key(b))
        elif t.bit_width in (8, 16, 32, 64):
            lcols.append(a)
            rcols.append(b)
        else:
            raise ArrowNotImplementedError(f"hash join on the device: keys of type {t.name}")
    return lcols, rcols


def _key_validity(arrays, n: int, device):
    """The AND of the arrays' validity (arx_hash_join_key_validity) as a bitmap tensor, None if none can be null."""
    arrays = [a for a in arrays if a.may_have_nulls()]
    if not arrays or n == 0:
        return None
    lib, stream = _lib_and_stream(device)
    out = alloc(bitmap_nbytes(n), device)
    spans = (_lib.ArxSpan * len(arrays))(*[a.span() for a in arrays])
    check(lib.arx_hash_join_key_validity(spans, len(arrays), n, out.data_ptr(), stream))
    return out


def _max_output_rows(device, payload_row_bytes: int = 0) -> int:
    """Output rows a join may produce: HASH_JOIN_MAX_OUTPUT_ROWS, or what free device memory holds at two int64 index
    arrays and a bitmap (17 bytes) plus `payload_row_bytes` of gathered columns per row."""
    if HASH_JOIN_MAX_OUTPUT_ROWS is not None:
        return int(HASH_JOIN_MAX_OUTPUT_ROWS)
    if device.type == "cuda":
        free, _ = torch.cuda.mem_get_info(device)
        return int(free) // (17 + payload_row_bytes)
    return 1 << 40


def _payload_row_bytes(columns) -> int:
    """Bytes per output row of gathering `columns` (values, offsets and the average string, validity)."""
    total = 0
    for c in columns:
        if is_base_binary(c.type):
            nbytes = int(c.buffers[2].numel()) if c.buffers[2] is not None else 0
            total += 4 + 1 + -(-nbytes // max(1, c.length))
        else:
            total += max(1, c.type.byte_width) + 1
    return total


def _ptr_or_none(t):
    return None if t is None else t.data_ptr()


def hash_join_indices(left_keys, right_keys, join_type="inner", null_equals_null=False, max_output_rows=None, filter=None):  # noqa: A002
    """The row pairs of the equi-join of the left (probe) and right (build) inputs on their key columns, as
    (left_indices, right_indices): int64 device Arrays, null where a side is unmatched (outer joins).  Semi / anti joins
    return only their side's indices and None for the other.  Keys: lists of equal-typed columns (fixed-width types
    compared by their bits, boolean, utf8 / binary).  null_equals_null: JoinKeyCmp::IS (a bool, or one per key column);
    otherwise a null key matches nothing.  Row order: inner / outer rows follow the left rows, the right rows of one left
    row ascend, the right-only rows of right / full outer joins come last in right-row order; semi / anti rows are in
    input order.  A join of more than max_output_rows rows (default: what free device memory holds) raises
    ArrowCapacityError before the output is allocated.
    filter: the residual predicate of HashJoinNodeOptions::filter as a callable (left_rows, right_rows) -> boolean Array
    over the T candidate pairs (the key-equal pairs in the order above, as two int64 Arrays).  A pair is a match only where
    the result is true (null: no match); which probe and build rows count as matched for outer, semi and anti joins
    follows from the passing pairs, per build row.  The candidate pairs are allocated first and stay live while the
    output is written: the limit is applied to their number and to the output's number of rows, each on its own, not to
    the sum, so peak memory is up to twice what the limit alone suggests."""
    jt = _join_type_code(join_type)
    left_keys, right_keys = list(left_keys), list(right_keys)
    if not left_keys or len(left_keys) != len(right_keys):
        raise ArrowInvalid("hash join: the same positive number of key columns on both sides is required")
    dev = next((k.device for k in left_keys + right_keys if isinstance(k, Array)), None)
    if dev is None:
        from .array import default_device
        dev = default_device()
    left_keys = [_as_device_key(k, dev) for k in left_keys]
    right_keys = [_as_device_key(k, dev) for k in right_keys]
    nl, nb = left_keys[0].length, right_keys[0].length
    if any(k.length != nl for k in left_keys) or any(k.length != nb for k in right_keys):
        raise ArrowInvalid("Array arguments must all be the same length")
    eq_is = list(null_equals_null) if isinstance(null_equals_null, (list, tuple)) else [bool(null_equals_null)] * len(left_keys)
    if len(eq_is) != len(left_keys):
        raise ArrowInvalid("hash join: null_equals_null needs one entry per key column")
    lib, stream = _lib_and_stream(dev)
    lcols, rcols = _join_key_columns(left_keys, right_keys)
    grouper = Grouper([c.type for c in rcols], max(1, nb), dev)
    build_ids = grouper.consume(rcols)
    num_groups = grouper.num_groups
    probe_ids = grouper.lookup(lcols)
    build_valid = _key_validity([k for k, s in zip(right_keys, eq_is) if not s], nb, dev)
    probe_valid = _key_validity([probe_ids] + [k for k, s in zip(left_keys, eq_is) if not s], nl, dev)
    bids = build_ids.values_ptr()

    group_offsets = alloc((num_groups + 1) * 8, dev)
    ws = _workspace(dev, lib.arx_hash_join_workspace_bytes(max(num_groups, nl)), "hash_join")
    check(lib.arx_hash_join_group_offsets(bids, _ptr_or_none(build_valid), nb, num_groups, group_offsets.data_ptr(),
                                          ws.data_ptr(), ws.numel(), stream))
    j = _PreparedJoin(dev, nl, nb, probe_ids, probe_valid, build_ids, build_valid, group_offsets, num_groups,
                      _max_output_rows(dev) if max_output_rows is None else int(max_output_rows))
    if filter is not None:
        return _hash_join_filtered(j, jt, filter)
    right_side = jt in (1, 3, 6, 7)
    matched = alloc(max(1, num_groups), dev, zero=True) if right_side else None
    total = j.probe_count(jt, matched)

    def build_rows(want_matched: int) -> Array:
        mask = alloc(bitmap_nbytes(nb), dev)
        check(lib.arx_hash_join_build_mask(bids, _ptr_or_none(build_valid), nb, matched.data_ptr(), want_matched,
                                           mask.data_ptr(), stream))
        return indices_nonzero(Array(bool_, nb, [None, mask], 0, 0))

    if jt in (1, 3):          # right semi / right anti
        rows = build_rows(1 if jt == 1 else 0)
        return None, Array(int64, rows.length, rows.buffers, 0, rows.offset)
    pairs = jt in (4, 5, 6, 7)
    tail = build_rows(0) if jt in (6, 7) else None
    n_out = j.checked_output_rows(total, tail)
    out_left = alloc(max(1, n_out) * 8, dev)
    out_right = alloc(max(1, n_out) * 8, dev) if pairs else None
    right_valid = alloc(bitmap_nbytes(n_out), dev) if jt in (5, 7) else None
    j.expand(jt, total, out_left, out_right, right_valid)
    return j.finish(tail, total, n_out, out_left, out_right, right_valid)


class _PreparedJoin:
    """What both paths of hash_join_indices share once the key rows are ids and the group offsets exist: the probe count
    into `offsets` (the read-back), the expand over the stably sorted build rows, the capacity check that counts the
    right-only tail, and the tail append."""

    def __init__(self, dev, nl, nb, probe_ids, probe_valid, build_ids, build_valid, group_offsets, num_groups, limit):
        self.dev, self.nl, self.nb, self.limit = dev, nl, nb, limit
        self.probe_ids, self.probe_valid, self.build_ids, self.build_valid = probe_ids, probe_valid, build_ids, build_valid
        self.group_offsets, self.num_groups = group_offsets, num_groups
        self.offsets = alloc((nl + 1) * 8, dev)
        self.lib, self.stream = _lib_and_stream(dev)

    def workspace(self, length: int):
        return _workspace(self.dev, self.lib.arx_hash_join_workspace_bytes(length), "hash_join")

    def probe_count(self, jt: int, matched) -> int:
        ws = self.workspace(max(self.num_groups, self.nl))
        total = C.c_int64(0)
        check(self.lib.arx_hash_join_probe_count(self.probe_ids.values_ptr(), _ptr_or_none(self.probe_valid), self.nl,
                                                 self.group_offsets.data_ptr(), self.num_groups, jt, _ptr_or_none(matched),
                                                 self.limit, self.offsets.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 C.byref(total), self.stream))
        return total.value

    def expand(self, jt: int, total: int, out_left, out_right, right_valid) -> None:
        """Slots [0, total) of the probe count's offsets; the build rows by group come from the stable sort of the ids."""
        sorted_rows = None
        if out_right is not None and total:
            sorted_rows = sort_indices(Array(uint32, self.nb, [self.build_valid, self.build_ids.data],
                                             kUnknownNullCount if self.build_valid is not None else 0, 0))
        check(self.lib.arx_hash_join_expand(self.offsets.data_ptr(), self.probe_ids.values_ptr(),
                                            _ptr_or_none(self.probe_valid), self.nl, self.group_offsets.data_ptr(),
                                            _ptr_or_none(sorted_rows.data if sorted_rows is not None else None), jt, total,
                                            out_left.data_ptr(), _ptr_or_none(out_right), _ptr_or_none(right_valid),
                                            self.stream))

    def checked_output_rows(self, total: int, tail) -> int:
        n_out = total + (tail.length if tail is not None else 0)
        if n_out > self.limit:     # the right-only tail of a right / full outer join counts too
            raise _lib.ArrowCapacityError(f"hash join: the output would have {n_out} rows, more than the {self.limit} "
                                          "that can be allocated")
        return n_out

    def finish(self, tail, total: int, n_out: int, out_left, out_right, right_valid):
        """Appends the right-only tail (null left indices) behind the `total` probe-side rows; the two index Arrays."""
        left_valid = None
        if tail is not None and tail.length:
            left_valid = alloc(bitmap_nbytes(n_out), self.dev)
            check(self.lib.arx_hash_join_append_build_rows(tail.values_ptr(), tail.length, total, out_left.data_ptr(),
                                                           left_valid.data_ptr(), out_right.data_ptr(),
                                                           _ptr_or_none(right_valid), self.stream))
        left = _join_index_array(out_left, n_out, left_valid, tail.length if left_valid is not None else None)
        return left, (_join_index_array(out_right, n_out, right_valid) if out_right is not None else None)


def _join_index_array(buf, n: int, valid=None, nulls=None) -> Array:
    a = Array(int64, n, [valid, buf], kUnknownNullCount if valid is not None else 0, 0)
    if valid is not None and nulls is not None:
        a._null_count = nulls
    return a


def _rows_of_flags(flags: torch.Tensor, n: int, want_set: int, dev) -> Array:
    """The rows whose byte flag is set (want_set 1) or clear (0), ascending: arx_hash_join_flags_to_mask + compaction."""
    lib, stream = _lib_and_stream(dev)
    mask = alloc(bitmap_nbytes(n), dev)
    check(lib.arx_hash_join_flags_to_mask(flags.data_ptr(), n, want_set, mask.data_ptr(), stream))
    return indices_nonzero(Array(bool_, n, [None, mask], 0, 0))


def _hash_join_filtered(j: _PreparedJoin, jt: int, predicate):
    """hash_join_indices with a residual filter: the candidates as an inner join, the predicate over them, then the
    filter kernels of csrc/hash_join.hip (pass words and their prefix, per-row counts, compaction, flag masks).  Semi and
    anti outputs are at most one input long and are not checked against the limit; the candidates and the pair outputs
    are, before they are allocated."""
    lib, stream, dev, nl, nb = j.lib, j.stream, j.dev, j.nl, j.nb
    T = j.probe_count(4, None)
    cand_left, cand_right = alloc(max(1, T) * 8, dev), alloc(max(1, T) * 8, dev)
    passed = None
    if T:
        j.expand(4, T, cand_left, cand_right, None)
        passed = predicate(_join_index_array(cand_left, T), _join_index_array(cand_right, T))
        if not isinstance(passed, Array) or passed.type != bool_ or passed.length != T:
            raise ArrowInvalid(f"hash join: the filter must return a boolean Array of {T} rows (one per candidate pair)")
    span = passed.span() if passed is not None else _lib.ArxSpan(None, None, 0, 0, 0)
    words = (T + 63) // 64
    build_hit = alloc(max(1, nb), dev, zero=True) if jt in (1, 3, 6, 7) else None
    probe_hit = alloc(max(1, nl), dev) if jt in (0, 2) else None
    pass_bits = alloc(max(1, words) * 8, dev)
    prefix = alloc((words + 1) * 8, dev)
    new_offsets = alloc((nl + 1) * 8, dev)
    ws = j.workspace(max(nl, words))
    total = C.c_int64(0)
    check(lib.arx_hash_join_filter_count(C.byref(span), j.offsets.data_ptr(), cand_right.data_ptr(), nl, jt,
                                         _ptr_or_none(build_hit), _ptr_or_none(probe_hit), j.limit, pass_bits.data_ptr(),
                                         prefix.data_ptr(), new_offsets.data_ptr(), ws.data_ptr(), ws.numel(),
                                         C.byref(total), stream))
    total = total.value
    if jt in (0, 2):          # left semi / left anti
        rows = _rows_of_flags(probe_hit, nl, 1 if jt == 0 else 0, dev)
        return Array(int64, rows.length, rows.buffers, 0, rows.offset), None
    if jt in (1, 3):          # right semi / right anti
        rows = _rows_of_flags(build_hit, nb, 1 if jt == 1 else 0, dev)
        return None, Array(int64, rows.length, rows.buffers, 0, rows.offset)
    tail = _rows_of_flags(build_hit, nb, 0, dev) if jt in (6, 7) else None
    n_out = j.checked_output_rows(total, tail)
    out_left, out_right = alloc(max(1, n_out) * 8, dev), alloc(max(1, n_out) * 8, dev)
    right_valid = alloc(bitmap_nbytes(n_out), dev) if jt in (5, 7) else None
    check(lib.arx_hash_join_filter_compact(pass_bits.data_ptr(), prefix.data_ptr(), T, j.offsets.data_ptr(),
                                           new_offsets.data_ptr(), nl, cand_left.data_ptr(), cand_right.data_ptr(), jt,
                                           total, out_left.data_ptr(), out_right.data_ptr(), _ptr_or_none(right_valid),
                                           stream))
    return j.finish(tail, total, n_out, out_left, out_right, right_valid)


class _GatheredColumns(dict):
    """name -> the column gathered at the candidate pairs' rows, taken when first asked for (only what the filter reads)."""

    def __init__(self, columns, rows):
        super().__init__()
        self._columns, self._rows = columns, rows

    def __missing__(self, name):
        self[name] = take(self._columns[name], self._rows, boundscheck=False)
        return self[name]


def hash_join(left_columns, right_columns, left_keys, right_keys, join_type="inner", left_output=None,
              right_output=None, left_suffix="", right_suffix="", null_equals_null=False, filter=None):  # noqa: A002
    """HashJoinNode over whole inputs held on the device: left_columns / right_columns map names to Arrays (fixed-width,
    boolean, utf8 / binary), left_keys / right_keys name the key columns.  Output columns: left_output then right_output
    (default: every column of the side(s) the join type emits), names that occur on both sides get the suffixes
    (HashJoinSchema's rule).  Returns a list of (name, Array), gathered with `take` by hash_join_indices' row pairs.
    filter: the residual predicate, a callable (left, right) -> boolean Array over the candidate pairs; left / right map
    every column name of their side to that column gathered at the pairs (gathered when first read)."""
    jt = _join_type_code(join_type)
    left_columns, right_columns = dict(left_columns), dict(right_columns)
    as_list = lambda k: [k] if isinstance(k, str) else list(k)   # noqa: E731
    lk, rk = as_list(left_keys), as_list(right_keys)
    lo = [] if jt in (1, 3) else (list(left_columns) if left_output is None else as_list(left_output))
    ro = [] if jt in (0, 2) else (list(right_columns) if right_output is None else as_list(right_output))
    payload = [left_columns[n] for n in lo] + [right_columns[n] for n in ro]
    dev = next(iter(left_columns.values())).device
    pair_filter = None
    if filter is not None:
        pair_filter = lambda lrows, rrows: filter(_GatheredColumns(left_columns, lrows),   # noqa: E731
                                                  _GatheredColumns(right_columns, rrows))
    li, ri = hash_join_indices([left_columns[k] for k in lk], [right_columns[k] for k in rk], jt, null_equals_null,
                               max_output_rows=_max_output_rows(dev, _payload_row_bytes(payload)), filter=pair_filter)
    out = []
    for names, cols, ix, suffix, other in ((lo, left_columns, li, left_suffix, ro), (ro, right_columns, ri, right_suffix, lo)):
        for name in names:
            out.append((name + suffix if name in other else name, take(cols[name], ix, boundscheck=False)))
    return out
