"""The rule that picks the compaction kernel, as arx_filter_compact_form states it beside launch_compact, pinned as
a table.  Host code only: no device call is made, no kernel runs, so this needs neither a GPU nor the emulator."""
import itertools
import os

import pytest

from . import util as U

GATHER, PIPELINED, PLAIN, UNALIGNED = 0, 1, 2, 3
NOT_IMPLEMENTED = -10


@pytest.fixture(scope="module")
def lib():
    from arrow_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def expected_form(row_numbers, width, aligned16, invert, length, out_length, sparse, batch, pipe):
    """The rule in words, restated independently of the C++."""
    sweep = PIPELINED if (batch >= 4 and pipe) else PLAIN
    if row_numbers:
        # GetTakeIndices: the gather form unless it is switched off or the bitmap is read inverted; the sweep writes
        # 2- and 4-byte row numbers only and, having no loads, is always an aligned one
        if not invert and sparse != 0 and width in (2, 4, 8):
            return GATHER
        return sweep if width in (2, 4) else NOT_IMPLEMENTED
    if width not in (1, 2, 4, 8, 16, 32):
        return NOT_IMPLEMENTED
    few = 0 <= out_length and out_length * 4 <= length
    if not invert and (sparse == 1 or (sparse == -1 and (width >= 8 or few))):
        return GATHER
    if width == 32:
        return NOT_IMPLEMENTED      # 32-byte values have the gather form only
    return sweep if aligned16 else UNALIGNED


def test_compaction_dispatch_table(lib):
    length = 100_000
    out_lengths = (-1, 0, length // 4, length // 4 + 1, length)      # unknown, and both sides of length / 4
    n = 0
    for sparse, batch, pipe in itertools.product((-1, 0, 1), (1, 4), (0, 1)):
        with U.options(lib, {b"filter_sparse": sparse, b"filter_batch": batch, b"filter_pipe": pipe}):
            for row_numbers, width, aligned16, invert, out_length in itertools.product(
                    (0, 1), (1, 2, 3, 4, 8, 16, 32), (0, 1), (0, 1), out_lengths):
                got = lib.arx_filter_compact_form(row_numbers, width, aligned16, invert, length, out_length)
                want = expected_form(row_numbers, width, aligned16, invert, length, out_length, sparse, batch, pipe)
                assert (got < 0 and want < 0) or got == want, (sparse, batch, pipe, row_numbers, width, aligned16, invert, out_length, got, want)
                n += 1
    assert n == 12 * 2 * 7 * 2 * 2 * 5


def test_compaction_dispatch_named_cases(lib):
    """The rows of the table a reader would look for first."""
    f = lib.arx_filter_compact_form
    with U.options(lib, {b"filter_sparse": -1, b"filter_batch": 4, b"filter_pipe": 1}):
        assert f(0, 8, 1, 0, 1000, 1000) == GATHER              # 8 bytes and wider: always, under the automatic choice
        assert f(0, 16, 0, 0, 1000, -1) == GATHER
        assert f(0, 4, 1, 0, 1000, 250) == GATHER               # 25 % exactly
        assert f(0, 4, 1, 0, 1000, 251) == PIPELINED
        assert f(0, 4, 0, 0, 1000, 251) == UNALIGNED
        assert f(0, 1, 1, 0, 1000, -1) == PIPELINED             # unknown output length: the sweep
        assert f(1, 4, 1, 0, 1000, -1) == GATHER
        assert f(1, 4, 1, 1, 1000, -1) == PIPELINED             # the sort's null partition reads the bitmap inverted
        assert f(1, 8, 1, 1, 1000, -1) < 0
    with U.options(lib, {b"filter_sparse": 0, b"filter_batch": 4, b"filter_pipe": 1}):
        assert f(0, 32, 1, 0, 1000, 10) < 0                     # 32-byte values have no sweep
        assert f(1, 8, 1, 0, 1000, 10) < 0                      # nor have 8-byte row numbers
        assert f(0, 8, 1, 0, 1000, 10) == PIPELINED
        assert f(0, 16, 0, 0, 1000, 10) == UNALIGNED
        with U.options(lib, {b"filter_pipe": 0}):
            assert f(0, 8, 1, 0, 1000, 10) == PLAIN
            assert f(0, 8, 0, 0, 1000, 10) == UNALIGNED         # the unaligned sweep has the plain form only
        with U.options(lib, {b"filter_batch": 1}):
            assert f(0, 8, 1, 0, 1000, 10) == PLAIN
            assert f(1, 2, 1, 0, 1000, 10) == PLAIN
    with U.options(lib, {b"filter_sparse": 1}):
        assert f(0, 1, 0, 0, 1000, 1000) == GATHER
        assert f(0, 32, 1, 0, 1000, 1000) == GATHER
        assert f(0, 3, 1, 0, 1000, 10) < 0
