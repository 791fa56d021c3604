"""zlib streams for the inflate tests (csrc/inflate_core.hpp): a helper, not a test.

``valid_cases()``: (name, stream, payload) for payloads and encodings that reach every part of the
decoder; most streams are Python's ``zlib``'s, the rest are written bit by bit here where zlib never
emits what is wanted (a match at the full distance of 32768, a code set with a single distance code).
Every one is checked here against ``zlib.decompress`` before it is handed out.

``malformed_cases()``: (name, stream, D, status): streams that must end with that status.  ``D`` is the
length the caller claims.  ``zlib.decompress`` refuses each of them too (the two with a wrong ``D``
aside, which are valid streams).
"""
import struct
import zlib

import numpy as np

import bgen_ref as R

OK, BAD_HEADER, INPUT_EXHAUSTED, BAD_BLOCK_TYPE, STORED_LEN, BAD_CODE_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, \
    OUTPUT_OVERFLOW, OUTPUT_SHORT, BAD_ADLER = range(11)


# ---------------------------------------------------------------------- payloads
def _periodic(period, total, seed):
    base = np.random.default_rng(seed).integers(0, 256, size=period, dtype=np.uint8)
    return np.resize(base, total).tobytes()


def _fibonacci():
    """Byte frequencies 1, 1, 2, 3, 5 ...: an unbounded Huffman tree 23 deep, so zlib's lengths reach 15."""
    counts, a, b = [], 1, 1
    for _ in range(24):
        counts.append(a)
        a, b = b, a + b
    data = np.repeat(np.arange(len(counts), dtype=np.uint8) * 7 + 3, counts)
    np.random.default_rng(11).shuffle(data)
    return data.tobytes()


def _bgen_block():
    rng = np.random.default_rng(5)
    n, bits = 3001, 11
    a = rng.integers(0, 2 ** bits, size=n, dtype=np.uint64)
    b = rng.integers(0, 2 ** bits, size=n, dtype=np.uint64) % (np.uint64(2 ** bits) - a)
    return R.make_block(np.stack([a, b], axis=1), bits, missing=[0, 17, n - 1])


def payloads():
    rng = np.random.default_rng(1)
    half = rng.integers(0, 256, size=32768, dtype=np.uint8).tobytes()
    return [
        ("empty", b""),
        ("one", b"\x5a"),
        ("zeros", bytes(100 * 1024)),
        ("period3", _periodic(3, 5000, 3)),
        ("period63", _periodic(63, 5000, 63)),
        ("period64", _periodic(64, 5000, 64)),
        ("period65", _periodic(65, 5000, 65)),
        ("back32768", half + half + half[:4096]),  # 68 KB: the second half repeats the first
        ("random", rng.integers(0, 256, size=50000, dtype=np.uint8).tobytes()),
        ("fibonacci", _fibonacci()),
        ("bgen", _bgen_block()),
        ("text", b"".join(b"variant %d of chromosome %d\n" % (i * i % 977, i % 23) for i in range(3000))),
    ]


def _deflate(data, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=False):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if not flushes:
        return c.compress(data) + c.flush()
    third = len(data) // 3
    return (c.compress(data[:third]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[third:2 * third])
            + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[2 * third:]) + c.flush())


ENCODINGS = [
    ("level0", dict(level=0)),
    ("level1", dict(level=1)),
    ("level6", dict(level=6)),
    ("level9", dict(level=9)),
    ("fixed", dict(strategy=zlib.Z_FIXED)),
    ("rle", dict(strategy=zlib.Z_RLE)),
    ("huffman", dict(strategy=zlib.Z_HUFFMAN_ONLY)),
    ("wbits9", dict(wbits=9)),
    ("flushes", dict(flushes=True)),
    ("flushes0", dict(level=0, flushes=True)),
]


# ---------------------------------------------------------------------- streams written bit by bit
class Bits(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, count):
        """``count`` bits of ``value``, least significant first."""
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):
        """A Huffman code: most significant bit first."""
        for k in range(count - 1, -1, -1):
            self.put((value >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def fixed_literal(self, v):
        if v < 144:
            self.code(0x30 + v, 8)
        elif v < 256:
            self.code(0x190 + v - 144, 9)
        elif v < 280:
            self.code(v - 256, 7)
        else:
            self.code(0xc0 + v - 280, 8)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _fixed_match(w, length, dist):
    ls = max(k for k in range(29) if LEN_BASE[k] <= length and (k == 28 or length < 258))
    w.fixed_literal(257 + ls)
    w.put(length - LEN_BASE[ls], LEN_EXTRA[ls])
    ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
    w.code(ds, 5)
    w.put(dist - DIST_BASE[ds], DIST_EXTRA[ds])


def _wrap(w, payload):
    w.align()
    return b"\x78\x9c" + bytes(w.out) + struct.pack(">I", zlib.adler32(payload))


def _stored(w, data, final):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xffff, 16)
    for v in data:
        w.put(v, 8)


def full_distance_stream():
    """32768 stored bytes, then fixed-code matches at distance 32768 (zlib itself stops at 32506),
    every length symbol once, and a distance-1 run."""
    first = np.random.default_rng(2).integers(0, 256, size=32768, dtype=np.uint8).tobytes()
    w = Bits()
    _stored(w, first, False)
    w.put(1, 1)
    w.put(1, 2)
    out = bytearray(first)
    for length in [258, 3] + LEN_BASE + [b + (1 << e) - 1 for b, e in zip(LEN_BASE, LEN_EXTRA)]:
        _fixed_match(w, length, 32768)
        for _ in range(length):
            out.append(out[-32768])
    w.fixed_literal(200)
    out.append(200)
    _fixed_match(w, 258, 1)
    out += bytes([200]) * 258
    for ds in range(30):  # every distance symbol, at its base and with all extra bits set
        for dist in (DIST_BASE[ds], DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1):
            _fixed_match(w, 70, dist)
            for _ in range(70):
                out.append(out[-dist])
    w.fixed_literal(256)
    return _wrap(w, bytes(out)), bytes(out)


def _dynamic_header(w, lit_lens, dist_lens, final=True):
    """A dynamic block header giving exactly these code lengths, each sent as a literal length with
    a flat 4-bit code-length code over the lengths 0 ... 15."""
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(lit_lens) - 257, 5)
    w.put(len(dist_lens) - 1, 5)
    w.put(19 - 4, 4)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    for sym in order:
        w.put(4 if sym < 16 else 0, 3)
    for v in list(lit_lens) + list(dist_lens):
        w.code(v, 4)  # canonical: sixteen 4-bit codes in symbol order


def single_codes_stream():
    """A dynamic block whose distance set is one 1-bit code (incomplete, accepted), and a second
    whose distance set is empty and which holds literals only."""
    w = Bits()
    lit = [0] * 258
    lit[65], lit[256], lit[257] = 1, 2, 2  # 'A' = 0, end = 10, length 3 = 11
    _dynamic_header(w, lit, [1], final=False)
    w.code(0, 1)  # A
    for _ in range(5):
        w.code(3, 2)  # length 3
        w.code(0, 1)  # distance symbol 0: distance 1
    w.code(2, 2)
    lit = [0] * 257
    lit[66], lit[256] = 1, 1
    _dynamic_header(w, lit, [0], final=True)
    for _ in range(7):
        w.code(0, 1)
    w.code(1, 1)
    payload = b"A" * 16 + b"B" * 7
    return _wrap(w, payload), payload


_VALID = []


def valid_cases():
    """[(name, stream, payload)], computed once."""
    if _VALID:
        return _VALID
    for pname, data in payloads():
        seen = set()
        for ename, kw in ENCODINGS:
            stream = _deflate(data, **kw)
            if stream in seen:
                continue
            seen.add(stream)
            _VALID.append((pname + "-" + ename, stream, data))
    stream, data = full_distance_stream()
    _VALID.append(("full-distance", stream, data))
    stream, data = single_codes_stream()
    _VALID.append(("single-codes", stream, data))
    text = dict(payloads())["text"]
    _VALID.append(("trailing-bytes", _deflate(text) + b"\x00\x01garbage", text))
    for name, stream, data in _VALID:
        assert zlib.decompress(stream) == data, name
    return _VALID


# ---------------------------------------------------------------------- malformed
def _raw(bits_fn, payload=b""):
    w = Bits()
    bits_fn(w)
    return _wrap(w, payload)


def malformed_cases():
    """[(name, stream, D, status)]"""
    text = dict(payloads())["text"]
    dyn = _deflate(text)           # one dynamic block
    fixed = _deflate(text[:2000], strategy=zlib.Z_FIXED)
    stored = _deflate(text[:3000], level=0)
    n = len(text)
    cases = [
        ("cut-in-header", dyn[:1], n, INPUT_EXHAUSTED),
        ("cut-empty", b"", 0, INPUT_EXHAUSTED),
        ("cut-in-dynamic-table", dyn[:12], n, INPUT_EXHAUSTED),
        ("cut-in-code-length-code", dyn[:5], n, INPUT_EXHAUSTED),
        ("cut-mid-data", dyn[:len(dyn) // 2], n, INPUT_EXHAUSTED),
        ("cut-mid-fixed", fixed[:len(fixed) // 2], 2000, INPUT_EXHAUSTED),
        ("cut-mid-stored", stored[:1000], 3000, INPUT_EXHAUSTED),
        ("cut-before-trailer", dyn[:-4], n, INPUT_EXHAUSTED),
        ("cut-in-trailer", dyn[:-1], n, INPUT_EXHAUSTED),
        ("adler", stored[:500] + bytes([stored[500] ^ 0x10]) + stored[501:], 3000, BAD_ADLER),
        ("d-too-small", dyn, n - 1, OUTPUT_OVERFLOW),
        ("d-too-small-stored", stored, 2999, OUTPUT_OVERFLOW),
        ("d-too-large", dyn, n + 1, OUTPUT_SHORT),
        ("d-zero", dyn, 0, OUTPUT_OVERFLOW),
        ("block-type-3", _raw(lambda w: (w.put(1, 1), w.put(3, 2))), 0, BAD_BLOCK_TYPE),
        ("stored-nlen", stored[:5] + bytes([stored[5] ^ 1]) + stored[6:], 3000, STORED_LEN),
        ("distance-before-start", _raw(lambda w: (w.put(1, 1), w.put(1, 2), w.fixed_literal(97), _fixed_match(w, 3, 2),
                                                  w.fixed_literal(256))), 4, BAD_DISTANCE),
        ("fdict", b"\x78\x20" + dyn[2:], n, BAD_HEADER),
        ("cm-7", b"\x77\x09" + dyn[2:], n, BAD_HEADER),
        ("cinfo-8", b"\x88\x1c" + dyn[2:], n, BAD_HEADER),
        ("fcheck", b"\x78\x9d" + dyn[2:], n, BAD_HEADER),
        ("code-lengths-oversubscribed",
         _raw(lambda w: (w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4),
                         [w.put(1, 3) for _ in range(19)])) + bytes(64), 0, BAD_CODE_LENGTHS),
        ("code-lengths-incomplete",
         _raw(lambda w: (w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4),
                         [w.put(2 if k < 3 else 0, 3) for k in range(19)])) + bytes(64), 0, BAD_CODE_LENGTHS),
        ("hlit-287", _raw(lambda w: (w.put(1, 1), w.put(2, 2), w.put(30, 5), w.put(0, 5), w.put(15, 4))) + bytes(64), 0,
         BAD_CODE_LENGTHS),
        ("hdist-31", _raw(lambda w: (w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(30, 5), w.put(15, 4))) + bytes(64), 0,
         BAD_CODE_LENGTHS),
    ]

    def no_end(w):
        lit = [0] * 257
        lit[65], lit[66] = 1, 1
        _dynamic_header(w, lit, [0])
        w.put(0, 16)

    def literal_set_oversubscribed(w):
        lit = [0] * 257
        lit[65], lit[66], lit[256] = 1, 1, 1
        _dynamic_header(w, lit, [0])
        w.put(0, 16)

    def literal_set_incomplete(w):
        lit = [0] * 257
        lit[65], lit[256] = 2, 2
        _dynamic_header(w, lit, [0])
        w.put(0, 16)

    def distance_set_incomplete(w):
        lit = [0] * 257
        lit[65], lit[256] = 1, 1
        _dynamic_header(w, lit, [2, 2])
        w.put(0, 16)

    def repeat_first(w):  # the first length is "repeat the previous"
        w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
        for k in range(19):  # lengths 1 for the symbols 16 and 17 only: 16 = code 0
            w.put(1 if k < 2 else 0, 3)
        w.put(0, 16)

    def repeat_past_end(w):  # 258 lengths wanted; 18 (138 zeros) twice overruns
        w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
        for k in range(19):  # symbols 17 and 18, one bit each: 17 = 0, 18 = 1
            w.put(1 if k in (1, 2) else 0, 3)
        for _ in range(2):
            w.code(1, 1), w.put(127, 7)
        w.put(0, 16)

    def match_without_distance_code(w):
        lit = [0] * 258
        lit[65], lit[256], lit[257] = 1, 2, 2
        _dynamic_header(w, lit, [0])
        w.code(0, 1), w.code(3, 2), w.put(0, 16)

    def unused_single_code(w):  # a lone 1-bit code: the other bit value belongs to nobody
        lit = [0] * 257
        lit[256] = 1
        _dynamic_header(w, lit, [0])
        w.code(1, 1), w.put(0, 16)

    cases += [
        ("no-end-of-block-code", _raw(no_end) + bytes(64), 0, BAD_CODE_LENGTHS),
        ("literal-set-oversubscribed", _raw(literal_set_oversubscribed) + bytes(64), 0, BAD_CODE_LENGTHS),
        ("literal-set-incomplete", _raw(literal_set_incomplete) + bytes(64), 0, BAD_CODE_LENGTHS),
        ("distance-set-incomplete", _raw(distance_set_incomplete) + bytes(64), 0, BAD_CODE_LENGTHS),
        ("repeat-without-previous", _raw(repeat_first) + bytes(64), 0, BAD_CODE_LENGTHS),
        ("repeat-past-the-end", _raw(repeat_past_end) + bytes(64), 0, BAD_CODE_LENGTHS),
        ("match-without-distance-code", _raw(match_without_distance_code) + bytes(64), 4, BAD_SYMBOL),
        ("unused-single-code", _raw(unused_single_code) + bytes(64), 0, BAD_SYMBOL),
        ("length-symbol-286", _raw(lambda w: (w.put(1, 1), w.put(1, 2), w.fixed_literal(286))) + bytes(64), 0,
         BAD_SYMBOL),
        ("distance-symbol-30", _raw(lambda w: (w.put(1, 1), w.put(1, 2), w.fixed_literal(97), w.fixed_literal(257),
                                               w.code(30, 5))) + bytes(64), 4, BAD_SYMBOL),
    ]
    for name, stream, d, status in cases:
        if status in (OUTPUT_OVERFLOW, OUTPUT_SHORT):
            assert len(zlib.decompress(stream)) != d, name
            continue
        try:
            zlib.decompress(stream)
        except zlib.error:
            continue
        raise AssertionError("zlib accepts the malformed stream " + name)
    return cases
