"""An independent BGEN decoder and writer for the tests: ``struct`` + ``zlib`` + NumPy integer
arithmetic from the BGEN specification (layout 2), importing nothing from the package.

Values: with D = 2**B - 1 and a sample's two B-bit integers (a, b): a / D, b / D and
(D - (a + b)) / D, each one float64 division; three NaNs where the sample's missing bit is set.
float32 is that float64 value cast once.
"""
import struct
import zlib

import numpy as np


def walk(path):
    """(header dict, list of variant dicts) of a layout-2 file."""
    raw = open(path, "rb").read()
    offset, lh, m, n = struct.unpack_from("<IIII", raw, 0)
    flags, = struct.unpack_from("<I", raw, 4 + lh - 4)
    header = {"m": m, "n": n, "flags": flags, "compression": flags & 3, "layout": (flags >> 2) & 15, "samples": None}
    at = 4 + lh
    if flags >> 31:
        _, ns = struct.unpack_from("<II", raw, at)
        at += 8
        samples = []
        for _ in range(ns):
            ln, = struct.unpack_from("<H", raw, at)
            samples.append(raw[at + 2:at + 2 + ln].decode())
            at += 2 + ln
        header["samples"] = samples
    at = offset + 4
    variants = []
    for _ in range(m):
        text = []
        for _ in range(3):
            ln, = struct.unpack_from("<H", raw, at)
            text.append(raw[at + 2:at + 2 + ln].decode())
            at += 2 + ln
        pos, k = struct.unpack_from("<IH", raw, at)
        at += 6
        alleles = []
        for _ in range(k):
            ln, = struct.unpack_from("<I", raw, at)
            alleles.append(raw[at + 4:at + 4 + ln].decode())
            at += 4 + ln
        c, = struct.unpack_from("<I", raw, at)
        at += 4
        if header["compression"]:
            d, = struct.unpack_from("<I", raw, at)
            at += 4
            c -= 4
        else:
            d = c
        variants.append({"id": text[0], "rsid": text[1], "chrom": text[2], "pos": pos, "alleles": alleles,
                         "offset": at, "stored": c, "inflated": d, "bytes": raw[at:at + c]})
        at += c
    return header, variants


def decode_block(data):
    """float64 [N, 3] of an inflated layout-2 block (diploid, unphased, biallelic)."""
    n, k, pmin, pmax = struct.unpack_from("<IHBB", data, 0)
    assert (k, pmin, pmax) == (2, 2, 2)
    flag = np.frombuffer(data, dtype=np.uint8, count=n, offset=8)
    phased, bits = data[8 + n], data[9 + n]
    assert phased == 0 and 1 <= bits <= 32 and len(data) == 10 + n + (2 * bits * n + 7) // 8
    stream = np.unpackbits(np.frombuffer(data, dtype=np.uint8, offset=10 + n), bitorder="little")
    fields = stream[:2 * bits * n].reshape(2 * n, bits).astype(np.uint64)
    ints = (fields << np.arange(bits, dtype=np.uint64)).sum(axis=1, dtype=np.uint64).reshape(n, 2)
    a, b = ints[:, 0], ints[:, 1]
    D = np.float64(2 ** bits - 1)
    out = np.empty((n, 3))
    out[:, 0] = a.astype(np.float64) / D
    out[:, 1] = b.astype(np.float64) / D
    out[:, 2] = (D - (a + b).astype(np.float64)) / D
    out[(flag & 0x80) != 0] = np.nan
    return out


def inflate(header, variant):
    return zlib.decompress(variant["bytes"]) if header["compression"] else variant["bytes"]


def decode_file(path):
    """float64 [N, M, 3], F order."""
    header, variants = walk(path)
    out = np.empty((header["n"], header["m"], 3), order="F")
    for j, v in enumerate(variants):
        out[:, j, :] = decode_block(inflate(header, v))
    return out


# ---------------------------------------------------------------------- hand-made files
def pack_fields(values, bits):
    values = np.asarray(values, dtype=np.uint64).reshape(-1)
    one = ((values[:, None] >> np.arange(bits, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(one.reshape(-1), bitorder="little").tobytes()


def make_block(ab, bits, missing=(), k=2, phased=0, ploidy=2, n_field=None, extra=b""):
    """An inflated block of len(ab) samples; ``ab``: integer pairs."""
    ab = np.asarray(ab, dtype=np.uint64).reshape(-1, 2)
    n = len(ab)
    flag = np.full(n, ploidy, dtype=np.uint8)
    flag[list(missing)] |= 0x80
    return (struct.pack("<IHBB", n if n_field is None else n_field, k, ploidy, ploidy) + flag.tobytes()
            + struct.pack("<BB", phased, bits) + pack_fields(ab, bits) + extra)


def make_file(path, blocks, n, layout=2, compression=0, samples=True, k=2, inflated_lie=0, truncate=0,
              chroms=None, rsids=None):
    """A BGEN file of the inflated ``blocks`` (one variant each) over ``n`` samples.  compression 1
    deflates them; any other non-zero value only sets the flag.  ``inflated_lie`` is added to the
    stored uncompressed length; ``truncate`` bytes are cut from the end."""
    flags = compression | (layout << 2) | ((1 << 31) if samples else 0)
    sb = b""
    if samples:
        ids = b"".join(struct.pack("<H", len(s)) + s for s in (("s%d" % i).encode() for i in range(n)))
        sb = struct.pack("<II", 8 + len(ids), n) + ids
    header = struct.pack("<III4sI", 20, len(blocks), n, b"bgen", flags)
    body = struct.pack("<I", len(header) + len(sb)) + header + sb
    for j, block in enumerate(blocks):
        text = ("v%d" % j, "0" if rsids is None else rsids[j], "1" if chroms is None else chroms[j])
        body += b"".join(struct.pack("<H", len(t)) + t.encode() for t in text)
        body += struct.pack("<IH", 100 + j, k) + b"".join(struct.pack("<I", 1) + a for a in [b"A", b"G", b"T"][:k])
        if compression:
            stored = zlib.compress(block) if compression == 1 else block
            body += struct.pack("<II", len(stored) + 4, len(block) + inflated_lie) + stored
        else:
            body += struct.pack("<I", len(block)) + block
    with open(path, "wb") as f:
        f.write(body[:len(body) - truncate] if truncate else body)
    return path
