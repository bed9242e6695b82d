"""is_in / index_in (arrow_amd.compute, csrc/set_lookup.hip) against pyarrow.compute on the same values.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same grid on the MI355X
plus full-size rows (10^9 int64 rows against a 16-value and a 10^6-value set, 10^7 utf8 rows) checked in chunks."""
import numpy as np
import pytest

from . import util as U

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

LENGTHS = [0, 1, 63, 64, 65, 4097, 100_000]
INT_TYPES = [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64()]
TEMPORAL = [pa.date32(), pa.date64(), pa.time32("ms"), pa.time64("us"), pa.timestamp("ns"), pa.duration("s")]


def rng_for(*key):
    return U.rng_for(0x5E7, *key)


def random_values(rng, typ, n, null_p=0.0, card=40):
    """n values drawn from a pool of `card` distinct ones (so that rows hit the set), nulls with probability null_p."""
    mask = (rng.random(n) < null_p) if null_p else None
    if pa.types.is_boolean(typ):
        return pa.array(rng.random(n) < 0.5, mask=mask)
    if pa.types.is_string(typ) or pa.types.is_binary(typ):
        pool = ["", "a", "ab", "abc", "a" * 17, "b" * 40, "x\x00", "x"] + [f"s{i}" * (1 + i % 5) for i in range(card)]
        vals = [pool[i] for i in rng.integers(0, len(pool), n)]
        arr = pa.array(vals, pa.string(), mask=mask)
        return arr.cast(typ) if pa.types.is_binary(typ) else arr
    if pa.types.is_floating(typ):
        pool = rng.standard_normal(card).astype(typ.to_pandas_dtype())
        pool[:4] = [0.0, -0.0, np.nan, np.inf]
        return pa.array(pool[rng.integers(0, card, n)], typ, mask=mask)
    phys = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[typ.bit_width // 8]
    info = np.iinfo(phys)
    pool = rng.integers(info.min, info.max, card, dtype=phys, endpoint=True)
    raw = pool[rng.integers(0, card, n)]
    storage = pa.array(raw, mask=mask)
    if pa.types.is_integer(typ):
        return storage.cast(typ, safe=False) if typ != storage.type else storage
    return storage.view(typ) if mask is None else pa.Array.from_buffers(typ, n, storage.buffers())


def value_set_for(rng, values, m, null_p):
    """m values: some taken from `values` (duplicates included), some fresh."""
    fresh = random_values(rng, values.type, m, null_p, card=max(m, 8))
    if len(values) == 0 or m == 0:
        return fresh
    pick = pa.array(rng.integers(0, len(values), m // 2))
    taken = values.take(pick)
    return pa.concat_arrays([taken, fresh.slice(0, m - m // 2)])


def check(ctx, values, value_set, skip_nulls, offset=0):
    amd = ctx
    sliced = values.slice(offset) if offset else values
    dv = amd.Array.from_pyarrow(values).slice(offset) if offset else amd.Array.from_pyarrow(values)
    want_is = pc.is_in(sliced, value_set=value_set, skip_nulls=skip_nulls)
    want_idx = pc.index_in(sliced, value_set=value_set, skip_nulls=skip_nulls)
    got_is = amd.compute.is_in(dv, value_set, skip_nulls=skip_nulls).to_pyarrow()
    got_idx_arr = amd.compute.index_in(dv, value_set, skip_nulls=skip_nulls)
    got_idx = got_idx_arr.to_pyarrow()
    assert got_is.equals(want_is), (sliced.type, skip_nulls)
    assert got_idx.equals(want_idx), (sliced.type, skip_nulls)
    assert got_idx_arr.null_count == want_idx.null_count


def supported_types():
    return INT_TYPES + [pa.float32(), pa.float64(), pa.bool_(), pa.string(), pa.binary()] + TEMPORAL


def _grid_types(ctx, typ, n):
    rng = rng_for("grid", typ, n)
    values = random_values(rng, typ, n, null_p=0.1)
    vs = value_set_for(rng, values, 16, 0.1)
    for skip in (False, True):
        check(ctx, values, vs, skip)


def _grid_cases(ctx):
    for typ in [pa.int64(), pa.float64(), pa.string()]:
        rng = rng_for("cases", typ)
        n = 5000
        plain = random_values(rng, typ, n)
        nullable = random_values(rng, typ, n, null_p=0.2)
        with_null = value_set_for(rng, plain, 24, 0.3)
        no_null = value_set_for(rng, plain, 24, 0.0)
        for values in (plain, nullable):
            for vs in (with_null, no_null, pa.array([], typ)):
                for skip in (False, True):
                    check(ctx, values, vs, skip)
                    check(ctx, values, vs, skip, offset=13)


# ---------------------------------------------------------------- emu tier

@pytest.mark.emu
@pytest.mark.parametrize("typ", supported_types(), ids=str)
def test_set_lookup_every_type(emu_ctx, typ):
    _grid_types(emu_ctx, typ, 4097)


@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_set_lookup_lengths(emu_ctx, n):
    for typ in (pa.int64(), pa.int8(), pa.string()):
        _grid_types(emu_ctx, typ, n)


@pytest.mark.emu
def test_set_lookup_nulls_duplicates_empty_sets_and_slices(emu_ctx):
    _grid_cases(emu_ctx)


@pytest.mark.emu
def test_set_lookup_issue_examples(emu_ctx):
    amd = emu_ctx
    v = amd.Array.from_pyarrow(pa.array([1, 2, None, 3]))
    vs = pa.array([2, None, 2, 1])
    assert amd.compute.is_in(v, vs).to_pylist() == [True, True, True, False]
    assert amd.compute.index_in(v, vs).to_pylist() == [3, 0, 1, None]
    assert amd.compute.is_in(v, vs, skip_nulls=True).to_pylist() == [True, True, False, False]
    assert amd.compute.index_in(v, vs, skip_nulls=True).to_pylist() == [3, 0, None, None]
    # a Python list, a chunked value set (indexed across its chunks), an arrow_amd.Array as the set
    assert amd.compute.index_in(v, [3, 3, 1]).to_pylist() == [2, None, None, 0]
    chunked = pa.chunked_array([pa.array([7, 8]), pa.array([], pa.int64()), pa.array([3, 2])])
    assert amd.compute.index_in(v, chunked).to_pylist() == [None, 3, None, 2]
    assert amd.compute.is_in(v, amd.Array.from_pyarrow(pa.array([3]))).to_pylist() == [False, False, False, True]
    assert amd.compute.is_in(v, []).to_pylist() == [False] * 4
    assert amd.compute.index_in(v, []).to_pylist() == [None] * 4


def _float_bits(amd):
    nan_a = np.frombuffer(np.uint64(0x7FF8000000000001).tobytes(), np.float64)[0]
    nan_b = np.frombuffer(np.uint64(0x7FF8000000000002).tobytes(), np.float64)[0]
    values = pa.array(np.array([0.0, -0.0, nan_a, nan_b, 1.5]))
    for vs in (pa.array(np.array([-0.0, nan_a])), pa.array(np.array([0.0, nan_b, nan_a]))):
        check(amd, values, vs, False)
    f32 = pa.array(np.array([0.0, -0.0, np.nan], np.float32))
    check(amd, f32, pa.array(np.array([-0.0], np.float32)), False)


@pytest.mark.emu
def test_set_lookup_float_bits(emu_ctx):
    _float_bits(emu_ctx)


@pytest.mark.emu
def test_set_lookup_type_resolution(emu_ctx):
    amd = emu_ctx
    i8 = pa.array([1, 2, 3], pa.int8())
    d = amd.Array.from_pyarrow(i8)
    for vs, want in ((pa.array([300]), [False, False, False]), (pa.array([1.5, 2.0]), [False, True, False]),
                     (pa.array(["1"]), [True, False, False])):
        assert pc.is_in(i8, value_set=vs).to_pylist() == want
        assert amd.compute.is_in(d, vs).to_pylist() == want
        assert amd.compute.index_in(d, vs).to_pylist() == pc.index_in(i8, value_set=vs).to_pylist()
    i32 = pa.array([1, 2], pa.int32())
    ts = pa.array([1], pa.timestamp("s"))
    with pytest.raises(pa.ArrowTypeError) as want:
        pc.is_in(i32, value_set=ts)
    with pytest.raises(pa.ArrowTypeError) as got:
        amd.compute.is_in(amd.Array.from_pyarrow(i32), ts)
    assert str(got.value) == str(want.value)
    # a string input against a large_string set
    s = pa.array(["a", "bb", None, ""])
    check(amd, s, pa.array(["bb", "", None], pa.large_string()), False)


@pytest.mark.emu
def test_set_lookup_strings_with_forced_hash_collisions(emu_ctx, monkeypatch):
    amd = emu_ctx
    rng = rng_for("collide")
    values = random_values(rng, pa.string(), 3000, null_p=0.05)
    vs = value_set_for(rng, values, 40, 0.05)
    for bits in (1, 3, 64):
        monkeypatch.setattr(amd.compute, "SET_LOOKUP_HASH_BITS", bits)
        for skip in (False, True):
            check(amd, values, vs, skip, offset=5)


@pytest.mark.emu
def test_set_lookup_set_larger_than_the_lds_budget(emu_ctx):
    amd = emu_ctx
    from arrow_amd import _lib

    lib = _lib.get_lib()
    rng = rng_for("big")
    m = 9000                      # 2^15 slots of 12 bytes: past the 64 KiB LDS table
    set_vals = rng.integers(-2**40, 2**40, m)
    values = pa.array(np.concatenate([set_vals[rng.integers(0, m, 6000)], rng.integers(-2**40, 2**40, 6000)]),
                      mask=rng.random(12000) < 0.05)
    vs = pa.array(set_vals, mask=rng.random(m) < 0.01)
    before = lib.arx_get_counter(b"set_lookup_global_probes")
    lds_before = lib.arx_get_counter(b"set_lookup_lds_probes")
    check(amd, values, vs, False, offset=3)
    assert lib.arx_get_counter(b"set_lookup_global_probes") == before + 2
    check(amd, values, vs.slice(0, 16), True)
    assert lib.arx_get_counter(b"set_lookup_lds_probes") == lds_before + 2


@pytest.mark.emu
def test_set_lookup_c_abi_decimal128_and_large_strings(emu_ctx):
    """Widths the mirror's Array type does not carry, through the C ABI directly: decimal128 (16-byte keys), large_utf8
    values against a utf8 set and the reverse."""
    import ctypes as C

    import torch

    from arrow_amd import _lib

    lib = _lib.get_lib()
    rng = rng_for("dec")
    n = 5000
    pool = [int(x) for x in rng.integers(-10**18, 10**18, 60)] + [10**37, -10**37]
    values = pa.array([pool[i] * 7 for i in rng.integers(0, len(pool), n)], pa.decimal128(38, 0),
                      mask=rng.random(n) < 0.1)

    def buf(b, nbytes):
        t = torch.zeros(max(nbytes, 8) + 16, dtype=torch.uint8)
        if b is not None and nbytes:
            t[:nbytes] = torch.frombuffer(bytearray(b.to_pybytes()[:nbytes]), dtype=torch.uint8)
        return t

    def span(arr, width):
        vb, db = arr.buffers()[0], arr.buffers()[1]
        keep = [buf(vb, (arr.offset + len(arr) + 7) // 8) if vb is not None else None, buf(db, (arr.offset + len(arr)) * width)]
        sp = _lib.ArxSpan(keep[0].data_ptr() if keep[0] is not None else None, keep[1].data_ptr(), arr.offset, len(arr),
                          arr.null_count)
        return sp, keep

    # 31 values: the 256-slot LDS table; 1001 values: 2048 slots of 20 bytes, the second LDS tier
    for m, skip in ((30, 0), (30, 1), (1000, 0), (1000, 1)):
        vs = pa.array([pool[i] * 7 for i in rng.integers(0, len(pool), m)] + [None], pa.decimal128(38, 0))
        sv, k1 = span(values.slice(7), 16)
        ss, k2 = span(vs, 16)
        state = torch.zeros(lib.arx_set_lookup_state_bytes(len(vs), 16), dtype=torch.uint8)
        assert lib.arx_set_lookup_build(state.data_ptr(), C.byref(ss), 16, None) == 0
        nv = len(values) - 7
        bits = torch.zeros(((nv + 63) // 64) * 8, dtype=torch.uint8)
        idx = torch.zeros(nv * 4, dtype=torch.uint8)
        valid = torch.zeros(((nv + 63) // 64) * 8, dtype=torch.uint8)
        assert lib.arx_set_lookup_is_in(state.data_ptr(), len(vs), 16, C.byref(sv), skip, bits.data_ptr(), None) == 0
        assert lib.arx_set_lookup_index_in(state.data_ptr(), len(vs), 16, C.byref(sv), skip, idx.data_ptr(),
                                           valid.data_ptr(), None) == 0
        got_is = np.unpackbits(bits.numpy(), bitorder="little")[:nv].astype(bool)
        want_is = np.array(pc.is_in(values.slice(7), value_set=vs, skip_nulls=bool(skip)).to_pylist())
        assert (got_is == want_is).all()
        want_idx = pc.index_in(values.slice(7), value_set=vs, skip_nulls=bool(skip)).to_pylist()
        got_valid = np.unpackbits(valid.numpy(), bitorder="little")[:nv].astype(bool)
        got_idx = idx.numpy().view(np.int32)
        assert [int(i) if ok else None for i, ok in zip(got_idx, got_valid)] == want_idx

    def bspan(arr, owidth):
        vb, ob, db = arr.buffers()
        noff = (arr.offset + len(arr) + 1) * owidth
        offs = np.frombuffer(ob, dtype=np.int32 if owidth == 4 else np.int64)[: arr.offset + len(arr) + 1]
        nbytes = int(offs[-1]) if len(offs) else 0
        keep = [buf(vb, (arr.offset + len(arr) + 7) // 8) if vb is not None else None, buf(ob, noff), buf(db, nbytes)]
        sp = _lib.ArxBinarySpan(keep[0].data_ptr() if keep[0] is not None else None, keep[1].data_ptr(), keep[2].data_ptr(),
                                arr.offset, len(arr), arr.null_count)
        return sp, keep

    svals = random_values(rng, pa.string(), 3000, null_p=0.1)
    sset = value_set_for(rng, svals, 20, 0.1)
    for vtype, stype in ((pa.large_string(), pa.string()), (pa.string(), pa.large_string()), (pa.large_binary(), pa.large_binary())):
        v, s = svals.cast(vtype).slice(5), sset.cast(stype)
        vw = 8 if vtype in (pa.large_string(), pa.large_binary()) else 4
        sw = 8 if stype in (pa.large_string(), pa.large_binary()) else 4
        sv, k1 = bspan(v, vw)
        ss, k2 = bspan(s, sw)
        state = torch.zeros(lib.arx_set_lookup_state_bytes(len(s), -1), dtype=torch.uint8)
        assert lib.arx_set_lookup_build_binary(state.data_ptr(), C.byref(ss), sw, 64, None) == 0
        bits = torch.zeros(((len(v) + 63) // 64) * 8, dtype=torch.uint8)
        assert lib.arx_set_lookup_is_in_binary(state.data_ptr(), C.byref(ss), sw, 64, C.byref(sv), vw, 0, bits.data_ptr(), None) == 0
        got = np.unpackbits(bits.numpy(), bitorder="little")[: len(v)].astype(bool)
        assert (got == np.array(pc.is_in(v, value_set=s.cast(v.type)).to_pylist())).all()


# ---------------------------------------------------------------- gpu tier
@pytest.mark.gpu
@pytest.mark.parametrize("typ", supported_types(), ids=str)
def test_gpu_set_lookup_every_type(gpu_ctx, typ):
    for n in LENGTHS:
        _grid_types(gpu_ctx, typ, n)


@pytest.mark.gpu
def test_gpu_set_lookup_cases(gpu_ctx):
    _grid_cases(gpu_ctx)
    _float_bits(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [16, 1_000_000])
def test_gpu_set_lookup_1e9_int64_rows(gpu_ctx, m):
    """10^9 int64 rows against a 16-value and a 10^6-value set, checked against numpy.isin chunk by chunk."""
    import torch

    amd = gpu_ctx
    n = 1_000_000_000
    rng = np.random.default_rng(1234 + m)
    set_vals = rng.integers(0, 4 * m, m, dtype=np.int64)
    gen = torch.Generator(device="cuda").manual_seed(99)
    data = torch.randint(0, 8 * m, (n,), dtype=torch.int64, device="cuda", generator=gen)
    arr = amd.Array(amd.array.int64, n, [None, data.view(torch.uint8)], 0, 0)
    out = amd.compute.is_in(arr, pa.array(set_vals))
    torch.cuda.synchronize()
    bits = out.data
    chunk = 1 << 26
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        vals = data[lo:hi].cpu().numpy()
        got = np.unpackbits(bits[lo // 8: (hi + 7) // 8].cpu().numpy(), bitorder="little")[: hi - lo].astype(bool)
        assert (got == np.isin(vals, set_vals)).all(), lo
    del out, bits, data, arr
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_set_lookup_1e7_utf8_rows(gpu_ctx):
    amd = gpu_ctx
    rng = np.random.default_rng(77)
    n = 10_000_000
    pool = np.array([f"key-{i}-" + "z" * (i % 23) for i in range(5000)], dtype=object)
    values = pa.array(pool[rng.integers(0, len(pool), n)].tolist(), pa.string(), mask=rng.random(n) < 0.02)
    vs = pa.array(pool[rng.integers(0, len(pool), 300)].tolist() + [None], pa.string())
    check(amd, values, vs, False)
    check(amd, values, vs, True, offset=11)


@pytest.mark.emu
@pytest.mark.parametrize("typ", [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.float64(), pa.string()], ids=str)
def test_set_lookup_second_lds_tier(emu_ctx, typ):
    """A set of 1000 values: a 2048-slot table, past the 256-slot tier and within the 64 KiB LDS budget of every width
    (16-byte keys: test_set_lookup_c_abi_decimal128_and_large_strings)."""
    amd = emu_ctx
    from arrow_amd import _lib

    lib = _lib.get_lib()
    rng = rng_for("tier2", typ)
    values = random_values(rng, typ, 6000, null_p=0.05, card=1500)
    vs = value_set_for(rng, values, 1000, 0.01)
    lds0, glob0 = lib.arx_get_counter(b"set_lookup_lds_probes"), lib.arx_get_counter(b"set_lookup_global_probes")
    for skip in (False, True):
        check(amd, values, vs, skip, offset=9)
    assert lib.arx_get_counter(b"set_lookup_lds_probes") == lds0 + 4
    assert lib.arx_get_counter(b"set_lookup_global_probes") == glob0


@pytest.mark.emu
def test_set_lookup_set_length_bound(emu_ctx):
    """Twice the set's length must fit the 32-bit slot count: 2^30 values at most, refused above (no table size, no build,
    no probe) instead of an endless capacity loop."""
    import ctypes as C

    import torch

    from arrow_amd import _lib

    lib = _lib.get_lib()
    assert lib.arx_set_lookup_state_bytes(1 << 30, 8) > (1 << 31) * 12
    for kw in (-1, 0, 1, 8, 16):
        assert lib.arx_set_lookup_state_bytes((1 << 30) + 1, kw) == 0
        assert lib.arx_set_lookup_state_bytes(-1, kw) == 0
    dummy = torch.zeros(1024, dtype=torch.uint8)
    big = _lib.ArxSpan(None, dummy.data_ptr(), 0, (1 << 30) + 1, 0)
    assert lib.arx_set_lookup_build(dummy.data_ptr(), C.byref(big), 8, None) == _lib.ARX_CAPACITY_ERROR
    bbig = _lib.ArxBinarySpan(None, dummy.data_ptr(), dummy.data_ptr(), 0, (1 << 30) + 1, 0)
    assert lib.arx_set_lookup_build_binary(dummy.data_ptr(), C.byref(bbig), 4, 64, None) == _lib.ARX_CAPACITY_ERROR
    rows = _lib.ArxSpan(None, dummy.data_ptr(), 0, 8, 0)
    assert lib.arx_set_lookup_is_in(dummy.data_ptr(), (1 << 30) + 1, 8, C.byref(rows), 0, dummy.data_ptr(), None) == \
        _lib.ARX_CAPACITY_ERROR
    assert b"2^30" in lib.arx_last_error()
