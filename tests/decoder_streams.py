"""Hand-made deflate, Snappy and LZ4 streams: the ones no encoder writes.  A helper, not a test module.  Every stream meant
to be valid comes with the payload a plain Python replay of its elements gives and has been accepted by the reference
(zlib for deflate here; tests/test_parquet.py asks the Snappy and LZ4 codecs) before a decoder under test sees it."""
import functools
import struct
import zlib

import numpy as np

from . import deflate_writer as DW


def _rand(rng, n, hi=256):
    return bytes(rng.integers(0, hi, n, dtype=np.uint8))


# --------------------------------------------------------------------------- deflate
PAD = 0x70                                   # the literal with the one-bit code of the small block
SMALL_LITS = list(range(0x30, 0x40))
SMALL_DIST = [1, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 2]           # distances 1, 25..32, 49..64


def small_litlen():
    l = [0] * 286                                            # 1/2 + 3/8 + 1/16 + 16/256 = 1
    l[PAD], l[256], l[285], l[257], l[279] = 1, 3, 3, 3, 4
    for s in SMALL_LITS:
        l[s] = 8
    return l


def small_tokens(rng, pad=0):
    """The small dynamic block of the window tests: 0..7 one-bit literals, 50 literals, then matches with and without extra bits."""
    return [PAD] * pad + [SMALL_LITS[i] for i in rng.integers(0, 16, 50)] + [(258, 1), (3, 32), (100, 50)]


def rle_ops(lengths):
    """Code lengths -> code-length symbols with the longest repeats (16: 3..6 of the previous, 17: 3..10 zeros, 18: 11..138)."""
    ops, i = [], 0
    while i < len(lengths):
        v, run = lengths[i], 1
        while i + run < len(lengths) and lengths[i + run] == v:
            run += 1
        i += run
        if v != 0:
            ops.append((v, 0))
            run -= 1
        while run >= 3:
            if v == 0:
                take = min(run, 138)
                ops.append((18, take - 11) if take >= 11 else (17, take - 3))
            else:
                take = min(run, 6)
                ops.append((16, take - 3))
            run -= take
        ops += [(v, 0)] * run
    return ops


def repeat_lengths():
    """Literal / length (286) and distance (30) lengths whose longest-repeat coding uses 16, 17 and 18 with their smallest
    and largest extra bits and one repeat that runs from the literal / length lengths into the distance lengths."""
    lit = [0] * 286
    for s in (138, 150, 161, 172, 173, 174, 175, 180):
        lit[s] = 9
    for s in list(range(165, 172)) + [256]:
        lit[s] = 8
    for s in (179, 282, 283, 284, 285):
        lit[s] = 6
    lit[176], lit[177], lit[178] = 1, 2, 3
    dist = [6, 6, 1, 2, 3, 4, 5] + [0] * 23
    return lit, dist


class _Stream:
    def __init__(self):
        self.d, self.payload = DW.Deflate(), bytearray()

    def tokens(self, toks):
        self.payload += DW.replay(toks, bytes(self.payload[-32768:]))
        return toks

    def stored(self, data, last=False):
        self.d.stored(data, last)
        self.payload += data

    def done(self, name):
        return name, DW.checked(self.d.raw(), bytes(self.payload)), bytes(self.payload)


@functools.lru_cache(None)
def valid_deflate(seed=5):
    """[(name, raw deflate stream, payload)], each accepted by zlib with that payload."""
    rng = np.random.default_rng(seed)
    out = []
    # long codes: nearly every symbol of both codes beyond the decoder's lookup tables
    for k in (6, 4, 2):
        s = _Stream()
        lit, dist = DW.complete_lengths(286, k, rng), DW.complete_lengths(30, 10, rng)
        toks, produced, used_d, used_l = [int(x) for x in rng.integers(0, 256, 3000)], 3000, set(), set()
        for i in range(1500):
            if rng.random() < 0.5:
                toks.append(int(rng.integers(0, 256)))
                produced += 1
                continue
            ds = i % 30 if DW.DIST_BASE[i % 30] <= produced else int(rng.integers(0, 10))
            distance = min(DW.DIST_BASE[ds] + int(rng.integers(0, 1 << DW.DIST_EXTRA[ds])), produced, 32768)
            ls = int(rng.integers(0, 29))                                          # (every length symbol as likely)
            length = DW.LEN_BASE[ls] + int(rng.integers(0, 1 << DW.LEN_EXTRA[ls]))
            toks.append((length, distance))
            produced += length
            used_d.add(DW.symbol_of(distance, DW.DIST_BASE))
            used_l.add(DW.symbol_of(length, DW.LEN_BASE))
        assert len(used_d) == 30 and len(used_l) == 29
        s.d.dynamic_block(s.tokens(toks), lit, dist, last=True)
        out.append(s.done("long codes k=%d" % k))
    # the input window: a stored block of `shift` bytes, then the small dynamic block
    for shift in list(range(2030, 2060)) + [4090, 4096, 4097]:
        s = _Stream()
        s.stored(_rand(rng, shift))
        s.d.dynamic_block(s.tokens(small_tokens(rng)), small_litlen(), SMALL_DIST, last=True)
        out.append(s.done("stored %d then dynamic" % shift))
    # ... the dynamic block first: the stored block's header at every bit offset
    for pad in range(8):
        s = _Stream()
        s.d.dynamic_block(s.tokens(small_tokens(rng, pad)), small_litlen(), SMALL_DIST)
        s.stored(_rand(rng, 40), last=True)
        out.append(s.done("dynamic then stored, %d pad bits" % pad))
    # ... and behind m nine-bit literals of a fixed block, which (unlike a stored block) do not restart the window: the
    # restage after 2048 bytes falls on every byte of a dynamic block with long codes and of the stored header behind it
    lit, dist = DW.complete_lengths(286, 6, rng), DW.complete_lengths(30, 10, rng)
    for m in range(1540, 1830):
        s = _Stream()
        s.d.fixed_block(s.tokens([int(x) for x in rng.integers(144, 256, m)]))
        toks = [int(x) for x in rng.integers(0, 256, 50)] + [(258, 1), (3, 32), (100, 50), (int(rng.integers(3, 259)), int(rng.integers(1, m)))]
        s.d.dynamic_block(s.tokens(toks), lit, dist)
        s.stored(_rand(rng, 16))
        s.d.dynamic_block(s.tokens(small_tokens(rng)), small_litlen(), SMALL_DIST, last=True)
        out.append(s.done("fixed %d literals, dynamic, stored, dynamic" % m))
    # the ring: a stored block longer than it, then matches at its size
    s = _Stream()
    s.stored(_rand(rng, 65535))
    s.stored(b"")
    s.d.fixed_block(s.tokens([(258, 32768), (3, 32768), (258, 32767), (258, 32768 - 257), (258, 1), (4, 3)]), last=True)
    out.append(s.done("ring"))
    # the code-length code: 19 and 5 lengths (4 can only spell zeros), the repeat symbols, HLIT = 286, HDIST = 30, 284 + 31
    s = _Stream()
    lit, dist = repeat_lengths()
    ops = rle_ops(lit + dist)
    assert {(16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)} <= set(ops)
    at, crosses = 0, False
    for sym, extra in ops:
        n = {16: 3, 17: 3, 18: 11}.get(sym, 1) + extra
        crosses |= at < 286 < at + n
        at += n
    assert at == 316 and crosses
    toks = [138, 150, 161, 165, 171, 172, 175, 176, 177, 178, 179, 180] * 3
    toks += [(258, 1, 27), (258, 2), (163, 3), (200, 4), (257, 6), (194, 8), (226, 12), (258, 9, 27)] + [176, 165, 138]
    s.d.dynamic_block(s.tokens(toks), lit, dist, cl_ops=ops)
    cl = [0] * 19
    cl[0] = cl[8] = 1
    toks = [int(x) for x in rng.integers(1, 256, 300)]
    s.d.dynamic_block(s.tokens(toks), [0] + [8] * 256, [0], last=True, cl_lengths=cl, hclen=5)
    out.append(s.done("code-length code"))
    # small ends
    only_end = [0] * 256 + [1]
    s = _Stream()
    s.d.dynamic_block([], only_end, [0], last=True)
    out.append(s.done("only the end-of-block code"))
    s = _Stream()
    s.d.dynamic_block([], only_end, [0])
    s.stored(b"after an empty block", last=True)
    out.append(s.done("only the end-of-block code, then stored"))
    s = _Stream()
    s.d.dynamic_block(s.tokens([PAD] + SMALL_LITS * 3), small_litlen(), [0], last=True)
    out.append(s.done("no distance code"))
    s = _Stream()
    s.d.dynamic_block(s.tokens([0x31, (258, 1), 0x32, 0x33, (3, 1), (100, 1)]), small_litlen(), [1], last=True)
    out.append(s.done("a single one-bit distance code"))
    s = _Stream()
    s.d.fixed_block(s.tokens(list(range(256)) + [(258, 256), (3, 1), (100, 24577 // 64), (258, 300, 27)]), last=True)
    out.append(s.done("fixed block"))
    s = _Stream()
    for r in range(3):
        s.stored(_rand(rng, 700 + r))
        s.d.fixed_block(s.tokens([int(x) for x in rng.integers(0, 256, 100)] + [(40, 650), (258, 1)]))
        s.d.dynamic_block(s.tokens(small_tokens(rng, r)), small_litlen(), SMALL_DIST, last=(r == 2))
    out.append(s.done("blocks of all three types"))
    return out


# FEXTRA, FNAME, FCOMMENT and FHCRC (RFC 1952 2.3.1: the low 16 bits of the CRC-32 of the header before it)
GZIP_FULL_HEADER = bytes([0x1F, 0x8B, 8, 0x1E, 0, 0, 0, 0, 0, 3]) + struct.pack("<H", 5) + b"extra" + b"name.bin\0" + b"a comment\0"
GZIP_FULL_HEADER += struct.pack("<H", zlib.crc32(GZIP_FULL_HEADER) & 0xFFFF)


# --------------------------------------------------------------------------- Snappy
def sn_varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append(0x80 | (n & 0x7F))
        n >>= 7
    out.append(n)
    return bytes(out)


class SnappyBlock:
    """Elements of one Snappy block and what they mean.  literal(form): 0 = length in the tag (1..60 bytes), 60..63 = the tag
    value that announces 1..4 length bytes.  copy(kind): 1, 2 or 3 = one-, two- or four-byte offset."""

    def __init__(self):
        self.body, self.payload = bytearray(), bytearray()

    def literal(self, data, form=None):
        n = len(data) - 1
        if form is None:
            form = 0 if n < 60 else 60 if n < 256 else 61 if n < 65536 else 62
        if form == 0:
            assert n < 60
            self.body.append(n << 2)
        else:
            self.body.append(form << 2)
            self.body += n.to_bytes(form - 59, "little")
        self.body += data
        self.payload += data
        return self

    def copy(self, kind, length, offset):
        if kind == 1:
            assert 4 <= length <= 11 and offset < 2048
            self.body += bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 0xFF])
        else:
            assert 1 <= length <= 64
            self.body += bytes([kind | ((length - 1) << 2)]) + offset.to_bytes(2 if kind == 2 else 4, "little")
        assert 0 < offset <= len(self.payload)
        for _ in range(length):
            self.payload.append(self.payload[-offset])
        return self

    def at(self):
        """Where the next element's tag will stand in the finished block (the preamble's length is that of the final size)."""
        return len(self.body)

    def block(self):
        return sn_varint(len(self.payload)) + bytes(self.body)


@functools.lru_cache(None)
def valid_snappy(seed=6):
    """[(name, block, payload)]"""
    rng = np.random.default_rng(seed)
    out = []

    def done(name, b):
        out.append((name, b.block(), bytes(b.payload)))

    b = SnappyBlock()
    b.literal(_rand(rng, 60)).literal(_rand(rng, 61), 60).literal(_rand(rng, 5), 60).literal(_rand(rng, 300), 61)
    b.literal(_rand(rng, 100), 62).literal(_rand(rng, 100), 63).literal(_rand(rng, 1), 0).literal(_rand(rng, 70000), 62)
    done("literal length forms", b)
    for n in (2047, 2048, 2049):
        b = SnappyBlock().literal(_rand(rng, 7)).literal(_rand(rng, n)).copy(1, 11, 5).copy(2, 64, n).copy(2, 30, n + 40)
        done("literal of %d" % n, b.literal(_rand(rng, 9)).copy(1, 8, 20))
    b = SnappyBlock().literal(_rand(rng, 1100)).literal(_rand(rng, 1000))
    for off in (1, 255, 256, 2047):
        for length in (4, 11):
            b.copy(1, length, off).literal(_rand(rng, 3))
    done("copies with a one-byte offset", b)
    b = SnappyBlock()
    for _ in range(45):
        b.literal(_rand(rng, 1500))
    for off in (1, 16320, 16321, 16383, 16384, 65535):
        for length in (1, 64):
            b.copy(2, length, off).literal(_rand(rng, 2))
    b.copy(3, 64, 40000).literal(_rand(rng, 2)).copy(3, 33, 65536 + 500).copy(3, 1, 3).copy(3, 64, 67000)
    done("copies with two- and four-byte offsets", b)
    b = SnappyBlock().literal(_rand(rng, 70))
    for off in (1, 2, 3, 63, 64):
        b.copy(2, 64, off).copy(1, 11, off).literal(_rand(rng, 5))
    done("overlapping copies", b)
    b = SnappyBlock().literal(_rand(rng, 30)).literal(_rand(rng, 2048)).literal(_rand(rng, 10)).copy(2, 20, 20).copy(2, 64, 2100)
    done("a copy across the end of a long literal", b.copy(1, 10, 25))
    # a tag on each of the last six bytes of the first 1024-byte window: a 2-byte preamble, a 3-byte literal header
    for pos in range(1018, 1024):
        for name, tail in (("copy 1", lambda b: b.copy(1, 9, 700)), ("copy 2", lambda b: b.copy(2, 50, 1000)), ("copy 3", lambda b: b.copy(3, 64, 1)),
                           ("literal 63", lambda b: b.literal(_rand(rng, 200), 63)), ("literal 61", lambda b: b.literal(_rand(rng, 1500), 61))):
            b = SnappyBlock().literal(_rand(rng, pos - 5), 61)
            assert 2 + b.at() == pos
            tail(b)
            b.copy(2, 12, 900).literal(_rand(rng, 20))
            assert len(sn_varint(len(b.payload))) == 2
            done("%s at input byte %d" % (name, pos), b)
    done("the last tag is the second-to-last byte: a copy", SnappyBlock().literal(_rand(rng, 40)).copy(1, 7, 33))
    done("the last tag is the second-to-last byte: a literal", SnappyBlock().literal(_rand(rng, 40)).copy(1, 7, 33).literal(b"z"))
    return out


# --------------------------------------------------------------------------- LZ4
def xxh32(data, seed=0):
    """XXH32 of fewer than 16 bytes (the frame descriptor's check byte is bits 8..15 of it)."""
    p1, p2, p3, p5, m = 2654435761, 2246822519, 3266489917, 374761393, 0xFFFFFFFF
    assert len(data) < 4
    h = (seed + p5 + len(data)) & m
    for c in data:
        h = (h + c * p5) & m
        h = (((h << 11) | (h >> 21)) & m) * p1 & m
    h ^= h >> 15
    h = h * p2 & m
    h ^= h >> 13
    h = h * p3 & m
    return h ^ (h >> 16)


def lz4_header(linked):
    """Version 1, no checksums, no content size, 64 KB blocks: the reference writer's header (independent blocks), or the
    same with linked blocks."""
    flg_bd = bytes([0x40 if linked else 0x60, 0x40])
    return bytes([0x04, 0x22, 0x4D, 0x18]) + flg_bd + bytes([(xxh32(flg_bd) >> 8) & 0xFF])


def lz4_length(n):
    """(nibble, extension bytes) of a literal length, or of a match length minus 4."""
    if n < 15:
        return n, b""
    n -= 15
    return 15, b"\xFF" * (n // 255) + bytes([n % 255])


class Lz4Frame:
    """Sequences, blocks and what they mean; block() closes the block under construction."""

    def __init__(self, linked=False):
        self.linked, self.blocks, self.cur, self.payload = linked, [], bytearray(), bytearray()

    def sequence(self, literals, match=None, offset=None):
        ln, lext = lz4_length(len(literals))
        mn, mext = lz4_length(match - 4) if match is not None else (0, b"")
        self.cur += bytes([(ln << 4) | mn]) + lext + literals
        self.payload += literals
        if match is not None:
            self.cur += struct.pack("<H", offset) + mext
            for _ in range(match):
                self.payload.append(self.payload[-offset])
        return self

    def block(self):
        self.blocks.append(struct.pack("<I", len(self.cur)) + bytes(self.cur))
        self.cur = bytearray()
        return self

    def stored(self, data):
        assert not self.cur
        self.blocks.append(struct.pack("<I", len(data) | 0x80000000) + data)
        self.payload += data
        return self

    def frame(self):
        assert not self.cur
        return lz4_header(self.linked) + b"".join(self.blocks) + bytes(4)


@functools.lru_cache(None)
def valid_lz4(seed=7):
    """[(name, frame, payload)]"""
    rng = np.random.default_rng(seed)
    out = []

    def done(name, f):
        out.append((name, f.frame(), bytes(f.payload)))

    f = Lz4Frame()
    for lit in (14, 15, 270, 524):
        for mat in (14, 15, 270, 524):
            f.sequence(_rand(rng, lit), mat + 4, int(rng.integers(1, lit + 1)))
    done("literal and match length forms", f.sequence(_rand(rng, 16)).block())
    f = Lz4Frame().sequence(b"q", 700, 1).sequence(_rand(rng, 3), 300, 2).sequence(_rand(rng, 16)).block()
    done("offset 1", f)
    f = Lz4Frame(linked=True).sequence(_rand(rng, 65000)).block()
    f.sequence(_rand(rng, 600), 40, 65535).sequence(_rand(rng, 5), 300, 64000).sequence(_rand(rng, 16)).block()
    done("offset 65535 into the previous linked block", f)
    f = Lz4Frame(linked=True).sequence(_rand(rng, 50), 20, 7).sequence(_rand(rng, 16)).block().stored(_rand(rng, 300))
    f.sequence(b"", 30, 10).sequence(_rand(rng, 2), 100, 350).sequence(_rand(rng, 16)).block()
    done("a stored block between two compressed ones, linked", f)
    f = Lz4Frame().sequence(_rand(rng, 50), 20, 7).sequence(_rand(rng, 16)).block().stored(_rand(rng, 300))
    f.sequence(_rand(rng, 20), 30, 10).sequence(_rand(rng, 16)).block()
    done("a stored block between two compressed ones", f)
    f = Lz4Frame()
    for _ in range(300):
        f.sequence(_rand(rng, int(rng.integers(5, 20)))).block()
    done("many one-sequence blocks", f)
    return out


# --------------------------------------------------------------------------- streams meant to be invalid
def _sparse(n, lengths):
    out = [0] * n
    for sym, l in lengths.items():
        out[sym] = l
    return out


def zlib_header(cmf, fdict=False):
    flg = 0x20 if fdict else 0
    return bytes([cmf, flg + (31 - ((cmf << 8) | flg) % 31) % 31])


@functools.lru_cache(None)
def invalid_deflate(seed=8):
    """[(name, raw deflate stream, dst_size, the status the decoder documents for it)]: what the reference must reject (or
    not end at dst_size bytes).  Status 2 = the stream or a block runs past the input or the destination, 3 = a distance
    before the output, 4 = an invalid code / block type / stored length."""
    rng = np.random.default_rng(seed)
    D = DW.Deflate
    out = [("incomplete literal/length set", D().dynamic_block([65, 66, 65], _sparse(257, {65: 2, 66: 2, 256: 2}), [0], True).raw(), 3, 4),
           ("incomplete distance set", D().dynamic_block([65, (3, 1)], _sparse(258, {65: 1, 256: 2, 257: 2}), [2, 2], True).raw(), 4, 4),
           ("over-subscribed set", D().dynamic_block([65], _sparse(257, {65: 1, 66: 1, 256: 1}), [0], True).raw(), 1, 4),
           ("incomplete code-length code", D().dynamic_block([5], [0] + [8] * 256, [0], True, cl_lengths=_sparse(19, {0: 2, 8: 2})).raw(), 1, 4),
           ("four code-length lengths spell only zeros",
            D().dynamic_block([], [0] * 257, [0], True, cl_lengths=_sparse(19, {0: 1, 18: 2, 17: 3, 16: 3}), hclen=4, end=False).raw(), 0, 4),
           ("repeat symbol 16 first", D().dynamic_block([], [8] * 257, [0], True, cl_ops=[(16, 0)] + [(8, 0)] * 254, end=False).raw(), 0, 4),
           ("a repeat past HLIT + HDIST", D().dynamic_block([], [8] * 257, [0], True, cl_ops=[(8, 0)] * 255 + [(18, 127)], end=False).raw(), 0, 4),
           ("HLIT = 287", D().dynamic_block([1], [0] + [8] * 256 + [0] * 30, [0], True).raw(), 1, 4),
           ("HDIST = 31", D().dynamic_block([1], [0] + [8] * 256, [0] * 31, True).raw(), 1, 4),
           ("no end-of-block code", D().dynamic_block([65, 66], _sparse(257, {65: 1, 66: 1}), [0], True, end=False).raw(), 2, 4),
           ("literal/length symbol 286", D().fixed_block([65, 286], True).raw(), 1, 4),
           ("literal/length symbol 287", D().fixed_block([65, 287], True).raw(), 1, 4),
           ("distance symbol 30", D().fixed_block([65, 66, 67, ("rawdist", 3, 30)], True).raw(), 6, 4),
           ("distance symbol 31", D().fixed_block([65, 66, 67, ("rawdist", 3, 31)], True).raw(), 6, 4),
           ("block type 3", D().dynamic_block([], [0] * 257, [0], True, block_type=3, end=False).raw(), 0, 4),
           ("stored LEN / NLEN mismatch", D().stored(b"abcdef", True, nlen=0x1234).raw(), 6, 4),
           ("stored LEN past the input", D().stored(b"abcdef", True, length=100).raw(), 100, 2),
           ("stored LEN past the destination", D().stored(_rand(rng, 100), True).raw(), 50, 2),
           ("a distance one past the output", D().fixed_block([65, 66, (3, 3)], True).raw(), 5, 3),
           ("a match one byte past dst_size", D().fixed_block([65, (10, 1)], True).raw(), 10, 2)]
    # truncation inside the block header, the code lengths, a symbol (14 or 15 bits), the extra bits (13 of them)
    lit, dist = DW.complete_lengths(286, 6), DW.complete_lengths(30, 10)
    long_literal = max(range(256), key=lambda s: lit[s])
    d = D().stored(_rand(rng, 30000))
    d.dynamic_block([long_literal] * 3, lit, dist, end=False)
    before_symbol = len(d.out) * 8 + d.n
    d.code(DW.canonical(lit)[long_literal])
    d.code(DW.canonical(lit)[257])
    d.code(DW.canonical(dist)[29])
    before_extra = len(d.out) * 8 + d.n
    d.bits(0x1555, 13)
    d.code(DW.canonical(lit)[256])
    whole = d.raw()
    block_at = 5 + 30000
    for name, cut in (("the block header", block_at + 1), ("the code lengths", block_at + 40), ("a symbol", before_symbol // 8 + 1),
                      ("the extra bits", before_extra // 8 + 1)):
        out.append(("truncated inside " + name, whole[:cut], 30007, 2))
    return out


@functools.lru_cache(None)
def invalid_containers():
    """[(name, whole page, dst_size)]: container headers zlib (window bits 15 | 32, as the reference codec opens it) rejects."""
    payload = b"container " * 30
    raw = DW.Deflate().fixed_block(list(payload[:40]) + [(200, 10), (60, 10)], True).raw()
    trailer = struct.pack("<II", 0, len(payload))
    return [("zlib header with CINFO = 8", zlib_header(0x88) + raw + bytes(4), len(payload)),
            ("zlib header with FDICT", zlib_header(0x78, True) + raw + bytes(4), len(payload)),
            ("gzip header cut inside FEXTRA", bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 3]) + struct.pack("<H", 1000) + b"x" * 30 + trailer, len(payload)),
            ("gzip header cut inside FNAME", bytes([0x1F, 0x8B, 8, 8, 0, 0, 0, 0, 0, 3]) + b"n" * 40, len(payload))]    # (no zero byte to its end)


def damage(rng, data, lo, hi):
    """The damage model of the random-damage tests, on data[lo:hi) (what lies behind hi — a trailer — is kept): 60 % one to
    three byte overwrites, 20 % one bit flip, 10 % truncation, 10 % intact."""
    what = rng.random()
    data = bytearray(data)
    if what < 0.6:
        for _ in range(int(rng.integers(1, 4))):
            data[int(rng.integers(lo, hi))] = int(rng.integers(0, 256))
    elif what < 0.8:
        data[int(rng.integers(lo, hi))] ^= 1 << int(rng.integers(0, 8))
    elif what < 0.9:
        del data[int(rng.integers(lo, hi)): hi]
    return bytes(data)


@functools.lru_cache(None)
def invalid_snappy():
    """[(name, block, dst_size, the status the decoder documents)]: 1 = bad preamble or another length than the page's, 2 = an
    element runs past the input or the output (or the block ends early), 3 = a bad offset."""
    lit = SnappyBlock().literal(b"abcdefgh")
    body = bytes(lit.body)
    return [("a literal tag on the last byte", sn_varint(9) + body + bytes([0 << 2]), 9, 2),
            ("a copy tag on the last byte", sn_varint(12) + body + bytes([1]), 12, 2),
            ("a two-byte-offset copy cut after one offset byte", sn_varint(12) + body + bytes([2 | (3 << 2), 4]), 12, 2),
            ("a preamble whose fifth byte does not fit 32 bits", bytes([0x88, 0x80, 0x80, 0x80, 0x10]) + body, 8, 1),
            ("a preamble of six bytes", bytes([0x88, 0x80, 0x80, 0x80, 0x80, 0x00]) + body, 8, 1),
            ("offset 0", sn_varint(12) + body + bytes([2 | (3 << 2), 0, 0]), 12, 3),
            ("an offset one past the output", sn_varint(12) + body + bytes([3 | (3 << 2), 9, 0, 0, 0]), 12, 3),
            ("a four-byte literal length of 2^32", sn_varint(12) + body + bytes([63 << 2, 0xFF, 0xFF, 0xFF, 0xFF]) + b"wxyz", 12, 2),
            ("a literal longer than the input", sn_varint(40) + bytes([39 << 2]) + b"short", 40, 2),
            ("a literal longer than the output", sn_varint(6) + body, 6, 2),
            ("a copy longer than the output", sn_varint(10) + body + bytes([1 | (0 << 2), 3]), 10, 2),
            ("another length than the page's", lit.block(), 9, 1),
            ("the block ends early", sn_varint(20) + body, 20, 2),
            ("no bytes at all", b"", 0, 1)]


@functools.lru_cache(None)
def invalid_lz4():
    """[(name, frame, dst_size, the status the decoder documents)]: 1 = another output length than the stream's, 2 = a sequence
    runs past the block or the output, 3 = a bad offset."""
    def frame(block):
        f = Lz4Frame()
        f.cur += block
        return f.block().frame()

    tail = bytes([0xC0]) + b"twelve bytes"
    return [("offset 0", frame(bytes([0x40]) + b"abcd" + bytes([0, 0]) + tail), 24, 3),
            ("an offset one past the output", frame(bytes([0x40]) + b"abcd" + bytes([5, 0]) + tail), 24, 3),
            ("literals past the block", frame(bytes([0xF0, 0x10]) + b"abc"), 31, 2),
            ("the block ends inside an offset", frame(bytes([0x40]) + b"abcd" + bytes([1])), 8, 2),
            ("a literal length that runs off the block", frame(bytes([0xF0, 0xFF, 0xFF])), 600, 2),
            ("a match length that runs off the block", frame(bytes([0x4F]) + b"abcd" + bytes([1, 0, 0xFF, 0xFF])), 600, 2),
            ("a match past the output", frame(bytes([0x4F]) + b"abcd" + bytes([1, 0, 100]) + tail), 60, 2),
            ("fewer bytes than the stream's", frame(bytes([0x40]) + b"abcd" + bytes([2, 0]) + tail), 27, 1)]
