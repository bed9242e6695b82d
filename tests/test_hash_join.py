"""Hash join (arrow_amd.compute.hash_join_indices / hash_join, csrc/hash_join.hip) against pa.Table.join after a
canonical sort, and against a Python restatement of the documented row order exactly.

The emu tier runs the kernel sources under the SIMT emulator (tests/emu); the gpu tier runs the same grid on the MI355X
plus a skewed key and a full-size join (2^27 int64 probe rows against 2^24 build rows) checked in chunks."""
import numpy as np
import pytest

from . import util as U

pa = pytest.importorskip("pyarrow")

JOIN_TYPES = ["left semi", "right semi", "left anti", "right anti", "inner", "left outer", "right outer", "full outer"]
INT_TYPES = [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64()]
KEY_TYPES = INT_TYPES + [pa.float32(), pa.float64(), pa.timestamp("ns"), pa.date32(), pa.bool_(), pa.string(),
                         pa.binary()]
LENGTHS = [0, 1, 63, 64, 65, 4097]


def rng_for(*key):
    return U.rng_for(0x4A0, *key)


def random_keys(rng, typ, n, null_p=0.0, card=30):
    """n keys drawn from `card` distinct ones, so that the two sides meet; floats include 0.0, -0.0 and NaN."""
    mask = (rng.random(n) < null_p) if null_p else None
    if pa.types.is_boolean(typ):
        return pa.array(rng.random(n) < 0.5, mask=mask)
    if pa.types.is_string(typ) or pa.types.is_binary(typ):
        pool = ["", "a", "ab", "x" * 13, "y" * 30, "x\x00"] + [f"k{i}" * (1 + i % 4) for i in range(card)]
        arr = pa.array([pool[i] for i in rng.integers(0, len(pool), n)], pa.string(), mask=mask)
        return arr.cast(typ) if pa.types.is_binary(typ) else arr
    if pa.types.is_floating(typ):
        pool = rng.standard_normal(card).astype(typ.to_pandas_dtype())
        pool[:3] = [0.0, -0.0, np.nan]
        return pa.array(pool[rng.integers(0, card, n)], typ, mask=mask)
    phys = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[typ.bit_width // 8]
    info = np.iinfo(phys)
    raw = rng.integers(info.min, info.max, card, dtype=phys, endpoint=True)[rng.integers(0, card, n)]
    storage = pa.array(raw, mask=mask)
    if pa.types.is_integer(typ):
        return storage.cast(typ, safe=False) if typ != storage.type else storage
    return pa.Array.from_buffers(typ, n, storage.buffers())


def key_tuples(cols):
    """Row keys for the restatement: floats by their bits, None for null."""
    out = []
    for c in cols:
        if pa.types.is_temporal(c.type):
            c = c.view(pa.int32() if c.type.bit_width == 32 else pa.int64())
        vals = c.to_pylist()
        if pa.types.is_floating(c.type):
            bits = np.asarray(c.fill_null(0).to_numpy(zero_copy_only=False)).view(np.uint32 if c.type.bit_width == 32
                                                                                    else np.uint64)
            vals = [None if v is None else int(b) for v, b in zip(vals, bits)]
        out.append(vals)
    return list(zip(*out)) if out else []


def restated(lkeys, rkeys, jt, null_eq=False):
    """The documented row order: probe order, ascending build rows, right-only rows last; semi / anti in input order."""
    lk, rk = key_tuples(lkeys), key_tuples(rkeys)
    usable = (lambda t: True) if null_eq else (lambda t: None not in t)
    groups = {}
    for j, t in enumerate(rk):
        if usable(t):
            groups.setdefault(t, []).append(j)
    hits = [groups.get(t, []) if usable(t) else [] for t in lk]
    matched = set(j for h in hits for j in h)
    if jt == "left semi":
        return [i for i, h in enumerate(hits) if h], None
    if jt == "left anti":
        return [i for i, h in enumerate(hits) if not h], None
    if jt == "right semi":
        return None, sorted(matched)
    if jt == "right anti":
        return None, [j for j in range(len(rk)) if j not in matched]
    left, right = [], []
    for i, h in enumerate(hits):
        if h:
            left += [i] * len(h)
            right += h
        elif jt in ("left outer", "full outer"):
            left.append(i)
            right.append(None)
    if jt in ("right outer", "full outer"):
        tail = [j for j in range(len(rk)) if j not in matched]
        left += [None] * len(tail)
        right += tail
    return left, right


def via_pyarrow(lkeys, rkeys, jt):
    names = [f"k{i}" for i in range(len(lkeys))]
    lt = pa.table(dict(zip(names, lkeys), lid=pa.array(np.arange(len(lkeys[0]), dtype=np.int64))))
    rt = pa.table(dict(zip(names, rkeys), rid=pa.array(np.arange(len(rkeys[0]), dtype=np.int64))))
    j = lt.join(rt, names, join_type=jt)
    cols = [j[c].to_pylist() if c in j.column_names else None for c in ("lid", "rid")]
    return cols


def canonical(left, right):
    n = len(left) if left is not None else len(right)
    rows = list(zip(left if left is not None else [None] * n, right if right is not None else [None] * n))
    return sorted(rows, key=lambda r: tuple(-1 if v is None else v for v in r))


def run_join(amd, lkeys, rkeys, jt, null_eq=False, offset=0):
    dl = [amd.Array.from_pyarrow(k) for k in lkeys]
    dr = [amd.Array.from_pyarrow(k) for k in rkeys]
    if offset:
        dl = [a.slice(offset) for a in dl]
        dr = [a.slice(offset) for a in dr]
    li, ri = amd.compute.hash_join_indices(dl, dr, jt, null_equals_null=null_eq)
    for x in (li, ri):
        assert x is None or x.type.name == "int64"
    return (li.to_pylist() if li is not None else None), (ri.to_pylist() if ri is not None else None)


def check_join(amd, lkeys, rkeys, jt, offset=0):
    got = run_join(amd, lkeys, rkeys, jt, offset=offset)
    if offset:
        lkeys = [k.slice(offset) for k in lkeys]
        rkeys = [k.slice(offset) for k in rkeys]
    assert got == restated(lkeys, rkeys, jt), (jt, lkeys[0].type)
    want = via_pyarrow(lkeys, rkeys, jt)
    assert canonical(*got) == canonical(*want), (jt, lkeys[0].type)


def grid_case(amd, typ, nl, nb, null_p, jts=JOIN_TYPES, offset=0):
    rng = rng_for(typ, nl, nb, null_p)
    card = max(30, nb // 8)    # about 8 build rows per key: the output stays a few times the input
    lk = [random_keys(rng, typ, nl + offset, null_p, card)]
    rk = [random_keys(rng, typ, nb + offset, null_p, card)]
    for jt in jts:
        check_join(amd, lk, rk, jt, offset)


def _every_type(ctx, typ):
    grid_case(ctx, typ, 700, 500, 0.1, offset=3)


def _lengths(ctx, n):
    for null_p in (0.0, 0.1):
        grid_case(ctx, pa.int64(), n, n, null_p, offset=5)
        grid_case(ctx, pa.string(), n, max(n // 2, 1), null_p, jts=["inner", "full outer", "right anti"], offset=1)


def _multi_column(ctx):
    rng = rng_for("multi")
    n = 900
    # two columns (int32, float64) and three (int64, int64, utf8): 16 + 4 bytes -> a chain of Grouper tables
    for types in ([pa.int32(), pa.float64()], [pa.int64(), pa.int64(), pa.string()], [pa.uint16(), pa.bool_()]):
        lk = [random_keys(rng, t, n, 0.05, card=6) for t in types]
        rk = [random_keys(rng, t, n // 2, 0.05, card=6) for t in types]
        for jt in JOIN_TYPES:
            check_join(ctx, lk, rk, jt, offset=2)


def _null_equals_null(ctx):
    rng = rng_for("is")
    lk = [random_keys(rng, pa.int32(), 400, 0.2, card=5), random_keys(rng, pa.string(), 400, 0.2, card=3)]
    rk = [random_keys(rng, pa.int32(), 300, 0.2, card=5), random_keys(rng, pa.string(), 300, 0.2, card=3)]
    for jt in JOIN_TYPES:
        assert run_join(ctx, lk, rk, jt, null_eq=True) == restated(lk, rk, jt, null_eq=True), jt
    # per column: IS on the first, EQ on the second
    got = ctx.compute.hash_join_indices([ctx.Array.from_pyarrow(k) for k in lk], [ctx.Array.from_pyarrow(k) for k in rk],
                                        "inner", null_equals_null=[True, False])
    lt, rt = key_tuples(lk), key_tuples(rk)
    want = [(i, j) for i, a in enumerate(lt) for j, b in enumerate(rt) if a == b and a[1] is not None]
    assert list(zip(got[0].to_pylist(), got[1].to_pylist())) == want


def _float_bits(ctx):
    lk = [pa.array([0.0, -0.0, float("nan"), 1.5, None], pa.float64())]
    rk = [pa.array([-0.0, float("nan"), 0.0, 0.0, None, 1.5], pa.float64())]
    got = run_join(ctx, lk, rk, "inner")
    assert got == ([0, 0, 1, 2, 3], [2, 3, 0, 1, 5])
    assert canonical(*got) == canonical(*via_pyarrow(lk, rk, "inner"))


def _sparse_hits(ctx, nl):
    """One probe row in 10^4 hits: long runs of zero-count rows between the slots of one expand workgroup."""
    rng = rng_for("sparse", nl)
    probe = rng.integers(1 << 20, 1 << 40, nl, dtype=np.int64)
    hits = np.arange(0, nl, 10_000) + rng.integers(0, 10_000, len(range(0, nl, 10_000)))
    hits = hits[hits < nl]
    probe[hits] = rng.integers(0, 50, len(hits))
    build = np.repeat(np.arange(50, dtype=np.int64), 3)
    rng.shuffle(build)
    lk, rk = [pa.array(probe)], [pa.array(build)]
    for jt in ("inner", "left semi", "left outer", "right anti"):
        got = run_join(ctx, lk, rk, jt)
        assert got == restated(lk, rk, jt), jt


@pytest.mark.emu
def test_hash_join_sparse_hits(emu_ctx):
    _sparse_hits(emu_ctx, 40_000)


@pytest.mark.emu
def test_hash_join_capacity_counts_the_right_only_rows(emu_ctx):
    amd = emu_ctx
    left = amd.Array.from_pyarrow(pa.array([1, 1, 1]))
    right = amd.Array.from_pyarrow(pa.array([1, 1, 1, 2, 2, 2, 2, 2]))
    # full outer: 9 matched pairs + 5 right-only rows
    with pytest.raises(amd._lib.ArrowCapacityError):
        amd.compute.hash_join_indices([left], [right], "full outer", max_output_rows=13)
    li, ri = amd.compute.hash_join_indices([left], [right], "full outer", max_output_rows=14)
    assert li.length == ri.length == 14 and li.null_count == 5


@pytest.mark.emu
@pytest.mark.parametrize("typ", KEY_TYPES, ids=str)
def test_hash_join_every_key_type(emu_ctx, typ):
    _every_type(emu_ctx, typ)


@pytest.mark.emu
@pytest.mark.parametrize("n", LENGTHS)
def test_hash_join_lengths(emu_ctx, n):
    _lengths(emu_ctx, n)


@pytest.mark.emu
def test_hash_join_multi_column_keys(emu_ctx):
    _multi_column(emu_ctx)


@pytest.mark.emu
def test_hash_join_null_equals_null(emu_ctx):
    _null_equals_null(emu_ctx)


@pytest.mark.emu
def test_hash_join_float_keys_compare_by_bits(emu_ctx):
    _float_bits(emu_ctx)


@pytest.mark.emu
def test_hash_join_tables(emu_ctx):
    amd = emu_ctx
    left = {"k": pa.array([1, 2, 2, None, 5]), "v": pa.array(["a", "b", "c", "d", "e"]),
            "f": pa.array([True, False, None, True, False])}
    right = {"k": pa.array([2, 5, 7, 2]), "v": pa.array([1.5, 2.5, None, 4.5])}
    dl = {n: amd.Array.from_pyarrow(a) for n, a in left.items()}
    dr = {n: amd.Array.from_pyarrow(a) for n, a in right.items()}
    for jt in JOIN_TYPES:
        out = amd.compute.hash_join(dl, dr, "k", "k", jt, left_suffix="_l", right_suffix="_r")
        want = pa.table(left).join(pa.table(right), "k", join_type=jt, left_suffix="_l", right_suffix="_r",
                                   coalesce_keys=False)
        got = pa.table({n: a.to_pyarrow() for n, a in out})
        assert got.column_names == want.column_names, jt
        order = [(n, "ascending") for n in want.column_names]
        assert got.sort_by(order).equals(want.sort_by(order)), jt


@pytest.mark.emu
def test_hash_join_errors(emu_ctx, monkeypatch):
    amd = emu_ctx
    a = amd.Array.from_pyarrow(pa.array([1, 1, 1, 1]))
    # 4 x 4 = 16 output rows against a limit of 15: refused before the output is allocated
    monkeypatch.setattr(amd.compute, "HASH_JOIN_MAX_OUTPUT_ROWS", 15)
    with pytest.raises(amd._lib.ArrowCapacityError):
        amd.compute.hash_join_indices([a], [a], "inner")
    monkeypatch.setattr(amd.compute, "HASH_JOIN_MAX_OUTPUT_ROWS", 16)
    assert amd.compute.hash_join_indices([a], [a], "inner")[0].length == 16
    with pytest.raises(amd._lib.ArrowNotImplementedError, match="dictionary"):
        amd.compute.hash_join_indices([pa.array(["x", "y"]).dictionary_encode()], [a], "inner")
    with pytest.raises(amd._lib.ArrowInvalid, match="key types differ"):
        amd.compute.hash_join_indices([a], [amd.Array.from_pyarrow(pa.array([1], pa.int32()))], "inner")
    with pytest.raises(amd._lib.ArrowInvalid, match="join type"):
        amd.compute.hash_join_indices([a], [a], "cross")


@pytest.mark.gpu
@pytest.mark.parametrize("typ", KEY_TYPES, ids=str)
def test_gpu_hash_join_every_key_type(gpu_ctx, typ):
    _every_type(gpu_ctx, typ)


@pytest.mark.gpu
def test_gpu_hash_join_cases(gpu_ctx):
    for n in LENGTHS + [100_000]:
        _lengths(gpu_ctx, n)
    _multi_column(gpu_ctx)
    _null_equals_null(gpu_ctx)
    _float_bits(gpu_ctx)


@pytest.mark.gpu
def test_gpu_hash_join_sparse_hits(gpu_ctx):
    _sparse_hits(gpu_ctx, 2_000_000)


@pytest.mark.gpu
def test_gpu_hash_join_more_tiles_than_one_grid(gpu_ctx):
    """2^15 x 2^15 rows of one key: 2^30 output rows, 2^21 expand tiles, more than one launch's grid holds."""
    amd = gpu_ctx
    import torch

    n = 1 << 15
    keys = amd.Array.from_numpy(np.zeros(n, np.int64))
    li, ri = amd.compute.hash_join_indices([keys], [keys], "inner")
    assert li.length == n * n
    ar = torch.arange(n, device=li.data.device)
    assert bool((li.data.view(torch.int64)[: n * n].view(n, n) == ar.unsqueeze(1)).all())
    assert bool((ri.data.view(torch.int64)[: n * n].view(n, n) == ar.unsqueeze(0)).all())


@pytest.mark.gpu
def test_gpu_hash_join_skewed_key(gpu_ctx):
    """One key holding 10^5 build rows hit by 10^3 probe rows: 10^8 output rows, checked whole."""
    amd = gpu_ctx
    import torch

    nb, nl = 100_000, 1_000
    build = np.full(nb, 7, np.int64)
    build[::10] = np.arange(nb // 10) + 100          # 10 % other keys
    probe = np.where(np.arange(nl) % 2 == 0, 7, -1).astype(np.int64)
    li, ri = amd.compute.hash_join_indices([amd.Array.from_numpy(probe)], [amd.Array.from_numpy(build)], "inner")
    hot = np.flatnonzero(build == 7)
    assert li.length == (nl // 2) * len(hot)
    got_l = li.data[: 8 * li.length].view(torch.int64).reshape(nl // 2, len(hot))
    got_r = ri.data[: 8 * ri.length].view(torch.int64).reshape(nl // 2, len(hot))
    want_l = torch.arange(0, nl, 2, device=got_l.device).unsqueeze(1)
    assert bool((got_l == want_l).all())
    assert bool((got_r == torch.from_numpy(hot).to(got_r.device).unsqueeze(0)).all())


@pytest.mark.gpu
def test_gpu_hash_join_full_size(gpu_ctx):
    """2^27 int64 probe rows against 2^24 build rows, a quarter of the build keys duplicated, inner and left outer:
    the totals against the known multiplicities of the generated keys, the rows in chunks of probe rows spread over the
    whole output against a host restatement (np.searchsorted over the stably sorted build keys)."""
    amd = gpu_ctx
    import torch

    rng = np.random.default_rng(27)
    nb, nl = 1 << 24, 1 << 27
    nd = nb - nb // 4
    distinct = (np.arange(nd, dtype=np.int64) * 0x9E3779B1) & ((1 << 40) - 1)   # odd multiplier: a bijection
    dup = rng.integers(0, nd, nb // 4)
    mult = 1 + np.bincount(dup, minlength=nd)                # build rows per distinct key
    build = np.concatenate([distinct, distinct[dup]])
    rng.shuffle(build)
    # half the probe rows hit a build key, half miss (keys above the build range)
    pick = rng.integers(0, nd, nl)
    hit_row = rng.random(nl) < 0.5
    probe = np.where(hit_row, distinct[pick], (1 << 41) + pick)
    cnt = np.where(hit_row, mult[pick], 0)
    order = np.argsort(build, kind="stable")
    sk = build[order]
    dprobe, dbuild = amd.Array.from_numpy(probe), amd.Array.from_numpy(build)
    chunk = 1 << 20
    for jt in ("inner", "left outer"):
        li, ri = amd.compute.hash_join_indices([dprobe], [dbuild], jt)
        out_cnt = np.maximum(cnt, 1) if jt == "left outer" else cnt
        offs = np.concatenate([[0], np.cumsum(out_cnt)])
        assert li.length == offs[-1] == ri.length
        gl, gr = li.data.view(torch.int64), ri.data.view(torch.int64)
        for r0 in (0, nl // 3, nl // 2 + 12345, nl - chunk):
            r1 = r0 + chunk
            s0, s1 = int(offs[r0]), int(offs[r1])
            c = out_cnt[r0:r1]
            assert np.array_equal(gl[s0:s1].cpu().numpy(), np.repeat(np.arange(r0, r1), c))
            k = np.arange(s1 - s0) - np.repeat(offs[r0:r1] - s0, c)   # slot k of a row: its key's k-th build row
            hit = np.repeat(cnt[r0:r1] > 0, c)
            lo = np.searchsorted(sk, probe[r0:r1])
            want_r = order[np.minimum(np.repeat(lo, c) + k, nb - 1)]
            got_r = gr[s0:s1].cpu().numpy()
            assert np.array_equal(got_r[hit], want_r[hit])
            if jt == "left outer":
                w0, w1 = s0 // 8, (s1 + 7) // 8
                bits = np.unpackbits(ri.validity[w0:w1].cpu().numpy(), bitorder="little")[s0 - 8 * w0: s1 - 8 * w0]
                assert np.array_equal(bits.astype(bool), hit)
        del li, ri, gl, gr
