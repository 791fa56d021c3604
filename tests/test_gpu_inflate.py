"""Device-side inflate (csrc/inflate.hip, csrc/inflate_core.hpp) and ``Bgen(..., inflate="device")``.

The streams are those of ``inflate_cases``.  The malformed ones run on the GPU only because the very
same list passes tests/test_inflate_host.py and the host fuzz program (tools/inflate_fuzz.cpp, under
ASan + UBSan) first: the decoder's bounds checks are proven there, on the same source, before a
wave is given bytes it must refuse.  Every launch here is also given a destination filled with a
sentinel, and every byte outside the tabled ranges must still hold it afterwards.

Values are compared bit for bit throughout: against the payloads, against ``inflate="host"`` and
against ``bgen_ref``'s independent decoder."""
import os
import zlib

import numpy as np
import pytest

import bgen_ref as R
import inflate_cases as C
from conftest import DATA
from pysnptools_amd import _grm as G
from pysnptools_amd import _native as N
from pysnptools_amd import hbm
from pysnptools_amd.distreader import Bgen
from pysnptools_amd.standardizer import Unit

pytestmark = pytest.mark.gpu

SENTINEL = 0xa5


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def launch(streams, lengths):
    """One ``snpmi_dev_inflate`` of ``streams`` claiming ``lengths``: the sources packed with gaps of
    0 ... 2 bytes (every byte alignment), the outputs at 8-byte boundaries with gaps of 0 or 8 bytes.
    Returns (status array, list of output bytes); asserts the sentinel outside the outputs."""
    count = len(streams)
    table = np.zeros((count, 4), dtype=np.uint64)
    s_at, d_at = 1, 8
    for k, (stream, d) in enumerate(zip(streams, lengths)):
        table[k] = (s_at, len(stream), d_at, d)
        s_at += len(stream) + k % 3
        d_at = (d_at + d + 7) // 8 * 8 + 8 * (k % 2)
    src = np.zeros(s_at + 1, dtype=np.uint8)
    for k, stream in enumerate(streams):
        src[int(table[k, 0]):int(table[k, 0]) + len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    dst = hbm.asarray(np.full(d_at + 8, SENTINEL, dtype=np.uint8))
    src_dev = hbm.asarray(src)
    status = np.full(count, 99, dtype=np.uint32)
    N.call("snpmi_dev_inflate", N.ptr(src_dev), src.nbytes, N.ptr(dst), dst.nbytes, N.ptr(table), count,
           N.ptr(status))
    got = dst.get()
    outside = np.ones(len(got), dtype=bool)
    outs = []
    for k in range(count):
        a, d = int(table[k, 2]), int(table[k, 3])
        outside[a:a + d] = False
        outs.append(got[a:a + d].tobytes())
    assert np.all(got[outside] == SENTINEL), "a byte outside the tabled ranges was written"
    return status, outs


def check_valid(cases):
    status, outs = launch([c[1] for c in cases], [len(c[2]) for c in cases])
    for (name, _, payload), st, out in zip(cases, status, outs):
        assert st == C.OK, (name, int(st))
        assert out == payload, name


# ------------------------------------------------------------------------- valid streams
def test_every_valid_stream_in_one_launch():
    cases = C.valid_cases()
    names = {c[0] for c in cases}
    for want in ("empty-level6", "one-level6", "zeros-level9", "period3-level6", "period63-level6",
                 "period64-level6", "period65-level6", "back32768-level9", "random-level0", "fibonacci-huffman",
                 "bgen-level6", "text-fixed", "text-rle", "text-wbits9", "text-flushes", "full-distance",
                 "single-codes", "trailing-bytes"):
        assert want in names, want
    assert max(len(c[2]) for c in cases) < 300 * 1024
    check_valid(cases)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_launch_shapes(count):
    cases = C.valid_cases()
    check_valid([cases[(7 * k + count) % len(cases)] for k in range(count)])  # mixed sizes, 0 bytes ... 100 KB


def test_more_streams_than_the_grid_has_waves():
    rng = np.random.default_rng(8)
    pool = []
    for k in range(64):
        data = rng.integers(0, 4, size=k % 41, dtype=np.uint8).tobytes()
        pool.append(("tiny%d" % k, zlib.compress(data, (0, 1, 6, 9)[k % 4]), data))
    check_valid([pool[(k * 13) % 64] for k in range(20000)])


# ------------------------------------------------------------------------- malformed streams
def test_malformed_streams_among_valid_ones():
    valid = [c for c in C.valid_cases() if len(c[2]) < 6000]
    bad = C.malformed_cases()
    assert {c[3] for c in bad} == set(range(1, 11))
    streams, lengths, want = [], [], []
    for k, (name, stream, d, status) in enumerate(bad):
        good = valid[k % len(valid)]
        streams += [good[1], stream]
        lengths += [len(good[2]), d]
        want += [(good[0], C.OK, good[2]), (name, status, None)]
    streams.append(valid[0][1]), lengths.append(len(valid[0][2])), want.append((valid[0][0], C.OK, valid[0][2]))
    status, outs = launch(streams, lengths)
    for (name, st_want, payload), st, out in zip(want, status, outs):
        assert st == st_want, (name, int(st))
        assert payload is None or out == payload, name


# ------------------------------------------------------------------------- the table is checked first
def test_table_refusals_before_any_launch():
    stream = zlib.compress(b"abc" * 10)
    src = hbm.asarray(np.frombuffer(stream + bytes(8), dtype=np.uint8))
    dst = hbm.asarray(np.full(128, SENTINEL, dtype=np.uint8))
    n, status = len(stream), np.zeros(2, dtype=np.uint32)

    def call(rows, src_bytes=src.nbytes, dst_bytes=128):
        table = np.array(rows, dtype=np.uint64)
        N.call("snpmi_dev_inflate", N.ptr(src), src_bytes, N.ptr(dst), dst_bytes, N.ptr(table), len(rows), N.ptr(status))

    for rows, err in (([[0, n + 9, 0, 30]], IndexError),            # the stored range leaves src
                      ([[n + 9, 1, 0, 30]], IndexError),
                      ([[0, n, 104, 30]], IndexError),              # the output leaves dst
                      ([[0, n, 136, 0]], IndexError),
                      ([[0, n, 0, 30], [0, n, 24, 30]], ValueError),  # outputs overlap
                      ([[0, n, 32, 30], [0, n, 32, 30]], ValueError),
                      ([[0, n, 4, 30]], ValueError),                # not on an 8-byte boundary
                      ([[0, 1 << 28, 0, 30]], ValueError),
                      ([[0, n, 0, 1 << 31]], ValueError)):
        with pytest.raises(err):
            call(rows)
    with pytest.raises(IndexError):
        call([[0, n, 0, 30]], dst_bytes=24)
    assert np.all(dst.get() == SENTINEL)  # nothing ran
    call([])  # no stream: nothing to do
    call([[0, n, 0, 30], [0, n, 32, 30]])
    got = dst.get()
    assert list(status) == [0, 0] and got[:30].tobytes() == b"abc" * 10 and got[32:62].tobytes() == b"abc" * 10
    assert np.all(got[30:32] == SENTINEL) and np.all(got[62:] == SENTINEL)


def test_check_records():
    n = 5
    blocks = [R.make_block([[1, 2]] * n, 7), R.make_block([[1, 2]] * n, 3, k=3, phased=1, ploidy=1, n_field=9),
              b"\x05\0\0\0\x02\0\x02", R.make_block([[1, 2]] * n, 2)[:12]]
    flags = bytearray(blocks[0])
    flags[8 + 3] = 0x80 | 5  # one sample: missing, ploidy 5
    blocks.append(bytes(flags))
    table, at = [], 0
    for b in blocks:
        table.append([at, len(b)])
        at += (len(b) + 7) // 8 * 8
    host = np.zeros(at, dtype=np.uint8)
    for (off, ln), b in zip(table, blocks):
        host[off:off + ln] = np.frombuffer(b, dtype=np.uint8)
    rec = np.zeros((len(blocks), 10), dtype=np.uint64)
    dev, table, outside = hbm.asarray(host), np.array(table, dtype=np.uint64), np.array([[8, at]], dtype=np.uint64)
    N.call("snpmi_dev_bgen_check", N.ptr(dev), at, N.ptr(table), len(blocks), n, N.ptr(rec))
    assert rec.tolist() == [[0, 7, 5, 2, 2, 2, 2, 2, 0, 15 + 9], [0, 3, 9, 3, 1, 1, 1, 1, 1, 15 + 4],
                            [1, 0, 0, 0, 0, 0, 255, 0, 0, 15], [1, 0, 5, 2, 2, 2, 255, 0, 0, 15],
                            [0, 7, 5, 2, 2, 2, 2, 5, 0, 15 + 9]]
    with pytest.raises(IndexError):
        N.call("snpmi_dev_bgen_check", N.ptr(dev), at, N.ptr(outside), 1, n, N.ptr(rec))


# ------------------------------------------------------------------------- Bgen(inflate="device")
FIXTURES = sorted(f for f in os.listdir(DATA) if f.endswith(".bgen") and R.walk(os.path.join(DATA, f))[0]["compression"] == 1)
_REF = {}


def ref(name):
    if name not in _REF:
        _REF[name] = R.decode_file(os.path.join(DATA, name))
        _REF[name].setflags(write=False)
    return _REF[name]


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_reads_are_the_host_route_bit_for_bit(name, dtype, order):
    path = os.path.join(DATA, name)
    dev = Bgen(path, inflate="device").read(dtype=dtype, order=order).val
    host = Bgen(path, inflate="host").read(dtype=dtype, order=order).val
    assert dev.flags["F_CONTIGUOUS" if order == "F" else "C_CONTIGUOUS"]
    assert same_bits(dev, host) and same_bits(dev, np.asarray(ref(name).astype(dtype), order=order))


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_selections_with_repeats(dtype, order):
    assert "example.bgen" in FIXTURES and "2500x100.bgen" in FIXTURES  # both golden cohorts are zlib files
    path = os.path.join(DATA, "example.bgen")
    rng = np.random.default_rng(4)
    iids, sids = rng.integers(0, 500, size=41), np.concatenate((rng.integers(0, 199, size=13), [5, 5, 198, 0]))
    dev = Bgen(path, inflate="device")[iids, sids].read(dtype=dtype, order=order).val
    host = Bgen(path)[iids, sids].read(dtype=dtype, order=order).val
    want = np.asarray(ref("example.bgen")[iids][:, sids].astype(dtype), order=order)
    assert same_bits(dev, host) and same_bits(dev, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_read_in_three_chunks(monkeypatch, dtype):
    path = os.path.join(DATA, "2500x100.bgen")
    monkeypatch.setattr(G, "BGEN_CHUNK_BYTES", 3 * 2500 * np.dtype(dtype).itemsize * 34)  # 34 + 34 + 32 SNPs
    bgen = Bgen(path, inflate="device")
    bgen._run_once()
    assert len(list(bgen._chunks(np.arange(100), 2500, np.dtype(dtype).itemsize, G.BGEN_CHUNK_BYTES))) == 3
    calls = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    dev = bgen.read(dtype=dtype).val
    assert [c for c in calls if "inflate" in c or "bgen_" in c] == \
        ["snpmi_dev_inflate", "snpmi_dev_bgen_check", "snpmi_dev_bgen_decode_" + N.suffix(dtype)] * 3
    assert same_bits(dev, np.asfortranarray(ref("2500x100.bgen").astype(dtype)))
    K3 = bgen[:, ::-1].as_snp().read_kernel(Unit(), dtype=dtype).val
    Kh = Bgen(path)[:, ::-1].as_snp().read_kernel(Unit(), dtype=dtype).val  # the same three chunks, inflated on the host
    assert same_bits(K3, Kh)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_as_snp_and_read_kernel_equal_the_host_route(dtype):
    path = os.path.join(DATA, "2500x100.bgen")
    dev, host = Bgen(path, inflate="device"), Bgen(path)
    assert same_bits(dev.as_snp().read(dtype=dtype).val, host.as_snp().read(dtype=dtype).val)
    K = dev.as_snp().read_kernel(Unit(), dtype=dtype).val
    assert K.shape == (2500, 2500) and np.isfinite(K).all()
    assert same_bits(K, host.as_snp().read_kernel(Unit(), dtype=dtype).val)
    sub = dev[::5, :].as_snp().read_kernel(Unit(), dtype=dtype).val  # an iid subset: the generic block loop
    assert same_bits(sub, host[::5, :].as_snp().read_kernel(Unit(), dtype=dtype).val)


def _blocks(n, m, bits, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(m):
        a = rng.integers(0, 2 ** bits, size=n, dtype=np.uint64)
        b = rng.integers(0, 2 ** bits, size=n, dtype=np.uint64) % (np.uint64(2 ** bits) - a)
        out.append(R.make_block(np.stack([a, b], axis=1), bits, missing=[0, n - 1]))
    return out


def test_uncompressed_file_reads_the_same(tmp_path, monkeypatch):
    path = R.make_file(str(tmp_path / "u.bgen"), _blocks(70, 9, 13, 1), 70, compression=0)
    calls = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    dev = Bgen(path, inflate="device").read().val
    assert "snpmi_dev_inflate" not in calls  # staged as with inflate="host"
    assert same_bits(dev, Bgen(path).read().val) and same_bits(dev, R.decode_file(path))


def test_written_file_with_mixed_block_sizes(tmp_path):
    blocks = _blocks(333, 5, 32, 2) + _blocks(333, 4, 1, 3) + _blocks(333, 3, 9, 4)
    path = R.make_file(str(tmp_path / "z.bgen"), blocks, 333, compression=1)
    dev = Bgen(path, inflate="device").read(dtype=np.float32, order="C").val
    assert same_bits(dev, np.ascontiguousarray(R.decode_file(path).astype(np.float32)))


# ------------------------------------------------------------------------- bad files
def _good():
    return R.make_block([[1, 2]] * 3, 2)


def _bits_byte(bits):
    good = _good()
    return good[:12] + bytes([bits]) + good[13:]


def _message(path, inflate):
    with pytest.raises(ValueError) as e:
        Bgen(path, inflate=inflate).read()
    return str(e.value)


@pytest.mark.parametrize("name, block", [
    ("k3", R.make_block([[1, 2]] * 3, 2, k=3)),
    ("phased", R.make_block([[1, 2]] * 3, 2, phased=1)),
    ("ploidy1", R.make_block([[1, 2]] * 3, 2, ploidy=1)),
    ("n-mismatch", R.make_block([[1, 2]] * 3, 2, n_field=4)),
    ("bits0", _bits_byte(0)),
    ("bits33", _bits_byte(33)),
    ("one-byte-more", R.make_block([[1, 2]] * 3, 2, extra=b"\0")),
    ("one-byte-fewer", R.make_block([[1, 2]] * 3, 2)[:-1]),
    ("too-short", _good()[:9]),
    ("one-odd-ploidy", _good()[:9] + b"\x83" + _good()[10:]),
])
def test_block_content_errors_read_as_on_the_host(tmp_path, name, block):
    path = R.make_file(str(tmp_path / "b.bgen"), [_good(), block, _good()], 3, compression=1)
    dev = _message(path, "device")
    assert dev == _message(path, "host") and "variant 1 ('v1')" in dev and path in dev


def test_lying_inflated_length(tmp_path):
    for lie in (2, -2):
        path = R.make_file(str(tmp_path / "l.bgen"), [_good(), _good()], 3, compression=1, inflated_lie=lie)
        dev = _message(path, "device")
        assert dev == _message(path, "host") and "inflates to 15 bytes, its header says %d" % (15 + lie) in dev


def test_truncated_file(tmp_path):
    path = R.make_file(str(tmp_path / "t.bgen"), [_good(), _good()], 3, compression=1, truncate=5)
    assert "truncated" in _message(path, "device") and "truncated" in _message(path, "host")


def test_stream_that_does_not_inflate(tmp_path):
    path = R.make_file(str(tmp_path / "c.bgen"), [_good(), _good()], 3, compression=1)
    at = R.walk(path)[1][1]["offset"]
    raw = bytearray(open(path, "rb").read())
    raw[at + 3] ^= 0x40  # inside the deflate data of variant 1
    with open(path, "wb") as f:
        f.write(raw)
    dev, host = _message(path, "device"), _message(path, "host")
    assert "variant 1 ('v1')" in dev and "does not inflate" in dev and "does not inflate" in host
