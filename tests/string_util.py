"""What the string kernel tests share (test_string_slice, test_string_trim, test_string_replace, test_string_compare,
test_match_substring): seeded generators, the knob that selects a kernel form, the comparison with the reference's
result and the device buffers of a host array for calls through the C ABI."""
import numpy as np

from .util import rng_for  # noqa: F401  (the string test modules call string_util.rng_for(SEED, ...))


class path_set:
    """The module global `knob_name` of arrow_amd.compute (STRING_SLICE_PATH, MATCH_SUBSTRING_PATH, ...) set to `path` for
    the length of a with block; what it found is restored."""

    def __init__(self, amd, knob_name, path):
        self.compute, self.knob_name, self.path = amd.compute, knob_name, path

    def __enter__(self):
        self.saved = getattr(self.compute, self.knob_name)
        setattr(self.compute, self.knob_name, self.path)

    def __exit__(self, *exc):
        setattr(self.compute, self.knob_name, self.saved)


def same(got, want, host, what):
    """The device result equals the reference's: rows, null count, offset 0, and no bitmap when the input has none."""
    assert got.to_pyarrow().equals(want), what
    assert got.null_count == want.null_count, what
    assert got.offset == 0, what
    if host.buffers()[0] is None:
        assert got.validity is None, what


def c_buffers(arr, owidth):
    """The device buffers of a (possibly sliced) binary array with offsets of `owidth` bytes and its ArxBinarySpan."""
    from arrow_amd import _lib
    from arrow_amd.array import to_device

    vb, ob, db = arr.buffers()
    offs = np.frombuffer(ob, dtype=np.int32 if owidth == 4 else np.int64)[: arr.offset + len(arr) + 1]
    nbytes = int(offs[-1])
    keep = [to_device(np.frombuffer(vb, dtype=np.uint8)[: (arr.offset + len(arr) + 7) // 8]) if vb is not None else None,
            to_device(offs), to_device(np.frombuffer(db, dtype=np.uint8)[:nbytes] if db is not None and nbytes else np.zeros(0, np.uint8))]
    span = _lib.ArxBinarySpan(keep[0].data_ptr() if keep[0] is not None else None, keep[1].data_ptr(), keep[2].data_ptr(),
                              arr.offset, len(arr), arr.null_count if vb is not None else 0)
    return span, keep, nbytes


def sync(t):
    if t.is_cuda:
        import torch

        torch.cuda.synchronize()
