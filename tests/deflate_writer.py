"""A bit-level deflate writer (RFC 1951) for hand-made streams: the caller chooses the block types, the code lengths, the
code-length code and its repeat symbols, i.e. everything an encoder decides for itself.  A helper, not a test module.  The
expected payload is `replay(tokens)`; a stream meant to be valid is first given to zlib (`checked`), so the writer is
checked against the reference before any decoder under test sees its output.

Tokens: an int is a literal / length SYMBOL written as it is (0..255 a literal; 256.. only make sense in streams meant to
be invalid), `(length, distance)` a match, `(length, distance, k)` a match with the length symbol forced to 257 + k (k = 27: 284
with extra bits 31 also says 258), `("rawdist", length, distance_symbol)` a match whose distance symbol is written raw
with no extra bits (30, 31)."""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# a complete code over all 19 code-length symbols (13/16 + 6/32 = 1): what dynamic_block uses unless told otherwise
CL_DEFAULT = [4] * 13 + [5] * 6


def canonical(lengths):
    """RFC 1951 3.2.2: per symbol (code, length), codes of one length consecutive in symbol order; the code comes back
    bit-reversed, i.e. as the least-significant-bit-first writer has to be given it so that its most significant bit goes out
    first.  An incomplete or over-subscribed set is assigned by the same rule (the streams meant to be invalid need one)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        out.append((int(format(nxt[l] & ((1 << l) - 1), "0%db" % l)[::-1], 2) if l else 0, l))
        nxt[l] += 1 if l else 0
    return out


def symbol_of(value, base):
    return max(s for s in range(len(base)) if base[s] <= value)


def replay(tokens, history=b""):
    """What the tokens mean, in plain Python (a match byte by byte, so an overlapping one repeats)."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out[len(history):])


class Deflate:
    """One deflate stream under construction: bits least-significant first, Huffman codes most-significant bit first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, pair):
        code, n = pair
        assert n > 0, "symbol without a code"
        self.bits(code, n)

    def raw(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")

    def stored(self, data, last=False, length=None, nlen=None):
        self.bits(1 if last else 0, 1)
        self.bits(0, 2)
        self.bits(0, -self.n % 8)
        length = len(data) if length is None else length
        self.out += struct.pack("<HH", length, (length ^ 0xFFFF) if nlen is None else nlen) + data
        return self

    def _tokens(self, tokens, lit, dist, end):
        for t in tokens:
            if isinstance(t, int):
                self.code(lit[t])
                continue
            raw_dist = t[0] == "rawdist"
            length = t[1] if raw_dist else t[0]
            ls = t[2] if (len(t) == 3 and not raw_dist) else symbol_of(length, LEN_BASE)
            self.code(lit[257 + ls])
            self.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
            if raw_dist:
                self.code(dist[t[2]])
            else:
                ds = symbol_of(t[1], DIST_BASE)
                self.code(dist[ds])
                self.bits(t[1] - DIST_BASE[ds], DIST_EXTRA[ds])
        if end:
            self.code(lit[256])

    def fixed_block(self, tokens, last=False, end=True):
        self.bits(1 if last else 0, 1)
        self.bits(1, 2)
        self._tokens(tokens, canonical(FIXED_LITLEN), canonical(FIXED_DIST), end)
        return self

    def dynamic_block(self, tokens, litlen, distlen, last=False, cl_lengths=None, hclen=19, cl_ops=None, hlit=None, hdist=None,
                      end=True, block_type=2):
        """litlen / distlen: code lengths of symbols 0..len-1 (at least 257 and 1).  cl_lengths: the 19 lengths of the
        code-length code; hclen of them are written, in CL_ORDER.  cl_ops: the code-length symbols as (symbol, extra bits
        value) pairs — by default one plain symbol per length, no repeats.  hlit / hdist: the counts the header announces,
        when they are to differ from the lists."""
        cl_lengths = CL_DEFAULT if cl_lengths is None else cl_lengths
        self.bits(1 if last else 0, 1)
        self.bits(block_type, 2)
        self.bits((len(litlen) if hlit is None else hlit) - 257, 5)
        self.bits((len(distlen) if hdist is None else hdist) - 1, 5)
        self.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.bits(cl_lengths[s], 3)
        cl = canonical(cl_lengths)
        for sym, extra in ([(l, 0) for l in list(litlen) + list(distlen)] if cl_ops is None else cl_ops):
            self.code(cl[sym])
            self.bits(extra, {16: 2, 17: 3, 18: 7}.get(sym, 0))
        self._tokens(tokens, canonical(litlen), canonical(distlen), end)
        return self


def checked(raw, payload):
    """The raw deflate stream, after the reference has agreed that it is valid and means `payload`."""
    d = zlib.decompressobj(-15)
    got = d.decompress(raw)
    assert got == payload and d.eof and d.unused_data == b"", "the hand-made stream is not what it was meant to be"
    return raw


def wrap(raw, payload, container, gzip_header=bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3])):
    if container == "zlib":
        return bytes([0x78, 0x9C]) + raw + struct.pack(">I", zlib.adler32(payload))
    assert container == "gzip"
    return gzip_header + raw + struct.pack("<II", zlib.crc32(payload), len(payload) & 0xFFFFFFFF)


def complete_lengths(n, k, rng=None):
    """A complete code over n symbols whose long codes all take 14 or 15 bits: one code of each length 1..k, three codes at
    every second length from k + 2 up to 6 where k < 6 (so that the short codes leave 2^-6, or 2^-k for k > 6), and the rest
    at 14 and 15 bits as Kraft's sum dictates — n = 286, k = 6: 232 codes of 14 bits and 48 of 15; n = 30, k = 10: 12 and 8.
    Shuffled over the symbols by rng."""
    short = list(range(1, k + 1)) + [l for l in range(k + 2, 7, 2) for _ in range(3)]
    units = (1 << 15) - sum(1 << (15 - l) for l in short)          # what is left, in codes of 15 bits
    rest = n - len(short)
    a, b = units - rest, 2 * rest - units                           # 2 a + b = units, a + b = rest
    assert a >= 0 and b >= 0, (n, k)
    lengths = short + [14] * a + [15] * b
    assert sum(1 << (15 - l) for l in lengths) == 1 << 15
    if rng is not None:
        lengths = [lengths[i] for i in rng.permutation(n)]
    return lengths
