"""Bgen on the GPU (csrc/bgen.hip).  Nobody can run cbgen where these tests run, so the values are
checked bit for bit against ``bgen_ref``, an independent decoder (struct + zlib + NumPy integers)
of the BGEN specification's formula -- p0 = a / D, p1 = b / D, p2 = (D - (a + b)) / D with D = 2^B - 1,
each one float64 division, float32 = that value cast once -- and against the digits the reference
pins (bgen.py:861-898) within its own 6 decimals.  Then what is built on the decode: selections,
``as_snp()``, its GRM, and the round trip through ``Bgen.write``.

GRM comparisons: one chunk against a DistData of the same triples adds the same block in the same
order and is asserted bit for bit; three chunks order the sums differently and carry
tests/test_gpu_dist.py's dense-operand bounds (1e-5 of max diag in float32, 1e-10 in float64)."""
import os

import numpy as np
import pytest

import bgen_ref as R
from conftest import DATA
from pysnptools_amd import _grm as G
from pysnptools_amd import _native as N
from pysnptools_amd import hbm
from pysnptools_amd.distreader import Bgen, DistData, DistGen
from pysnptools_amd.kernelreader import SnpKernel
from pysnptools_amd.snpreader._dist2snp import dist_to_snp
from pysnptools_amd.standardizer import Unit
from test_gpu_dist import same_bits
from test_gpu_parity import grm_close

pytestmark = pytest.mark.gpu

FILES = {"example": "example.bgen", "big": "2500x100.bgen", "bits1": "bits1.bgen"}
DTYPES = [np.float32, np.float64]
_REF = {}


def path(name):
    return os.path.join(DATA, FILES[name])


def ref(name):
    """float64 [N, M, 3] of a fixture by the independent decoder: computed once, read-only."""
    if name not in _REF:
        _REF[name] = R.decode_file(path(name))
        _REF[name].setflags(write=False)
    return _REF[name]


def exact(got, want64, dtype):
    want = np.asarray(want64).astype(dtype)  # float32: the float64 value cast once
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.dtype(dtype)
    assert same_bits(got, want)


# ------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(FILES))
def test_fixture_read_whole(name, dtype, order):
    val = Bgen(path(name)).read(dtype=dtype, order=order).val
    assert isinstance(val, np.ndarray) and val.flags["F_CONTIGUOUS" if order == "F" else "C_CONTIGUOUS"]
    exact(val, ref(name), dtype)


def test_order_a_is_f_and_values_stay_in_hbm(monkeypatch):
    val = Bgen(path("bits1")).read(order="A").val
    assert val.flags["F_CONTIGUOUS"] and val.dtype == np.float64
    monkeypatch.setenv("ARRAY_MODULE", "hbm")
    dev = Bgen(path("bits1")).read(dtype=np.float32).val
    assert isinstance(dev, hbm.HbmArray) and dev.order == "F"
    exact(dev.get(), ref("bits1"), np.float32)


def test_reference_digit_pins():
    bgen = Bgen(path("example"))
    assert np.all(np.isnan(bgen[[0], [0]].read().val))
    np.testing.assert_array_almost_equal(bgen[[1], [0]].read().val[0, 0],
                                         [0.027802362811705648, 0.00863673794284387, 0.9635608992454505])
    np.testing.assert_array_almost_equal(bgen[[2], [1]].read().val[0, 0],
                                         [0.97970582847010945, 0.01947019668749305, 0.00082397484239749366])
    val = bgen.read().val
    assert val[1, 0, 2] == 0.9635608992454505  # (D - (a + b)) / D: the pin from bgen-reader's own suite, to the digit


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_selections(dtype, order):
    bgen, want = Bgen(path("example")), ref("example")
    rng = np.random.default_rng(3)
    perm_i, perm_s = rng.integers(0, 500, size=37), rng.integers(0, 199, size=11)  # permutations with repeats
    mask_i, mask_s = rng.random(500) < 0.3, rng.random(199) < 0.2
    for sel in ((slice(None, None, -1), slice(None, None, -3)), (perm_i, perm_s), (mask_i, mask_s),
                (slice(None, 2), slice(None, None, 3)), (slice(None), [5, 5, 5]), (perm_i, slice(None))):
        got = bgen[sel[0], sel[1]].read(dtype=dtype, order=order).val
        exact(got, want[sel[0]][:, sel[1]], dtype)


def test_metadata_on_the_gpu_box():
    bgen = Bgen(path("example"), sample=os.path.join(DATA, "other.sample"))
    data = bgen[:3, :2].read()
    assert tuple(data.iid[0]) == ("0", "other_001") and data.sid[0] == "SNPID_2,RSID_2" and data.pos[0, 2] == 2000


# ------------------------------------------------------------------------- bit depths, written files
BITS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 31, 32]
SHAPES = [(1, 1), (3, 2), (5, 3), (64, 4), (257, 5)]


def _dist(n, m, seed):
    """Exact distributions with missing samples at the first, the last and interior positions."""
    rng = np.random.default_rng(seed)
    val = rng.dirichlet((1, 1, 1), size=(n, m))
    val[0, 0] = np.nan
    val[-1, -1] = np.nan
    val[n // 2, m // 2] = np.nan
    if n > 4:
        val[1:n - 1:3, 0] = np.nan
    return DistData(iid=[["0", "i%d" % i] for i in range(n)], sid=["s%d" % j for j in range(m)], val=val,
                    pos=[[1, 0, j] for j in range(m)])


@pytest.mark.parametrize("compression", [None, "zlib"])
@pytest.mark.parametrize("bits", BITS)
def test_bit_depths(tmp_path, bits, compression):
    for k, (n, m) in enumerate(SHAPES):
        bgen = Bgen.write(str(tmp_path / ("b%d.bgen" % k)), _dist(n, m, 100 * bits + k), bits=bits,
                          compression=compression)
        want = R.decode_file(bgen.filename)
        assert np.isnan(want[0, 0, 0]) and np.isnan(want[-1, -1, 0]) and (n == 1 or np.isnan(want).sum() < want.size)
        for dtype, order in ((np.float64, "F"), (np.float32, "C"), (np.float32, "F"), (np.float64, "C")):
            exact(bgen.read(dtype=dtype, order=order).val, want, dtype)


# ------------------------------------------------------------------------- the native entry
def _stage(blocks):
    """(HbmArray of the blocks at 8-byte boundaries + 16 spare bytes, offsets, byte count)."""
    offsets, at = [], 0
    for b in blocks:
        offsets.append(at)
        at += (len(b) + 7) // 8 * 8
    host = np.zeros(at + 16, dtype=np.uint8)
    for off, b in zip(offsets, blocks):
        host[off:off + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return hbm.asarray(host), offsets, len(host)


def _random_block(rng, n, bits):
    D = 2 ** bits - 1
    a = rng.integers(0, D + 1, size=n, dtype=np.uint64)
    b = rng.integers(0, D + 1, size=n, dtype=np.uint64) % (np.uint64(D) - a + np.uint64(1))
    ab = np.stack([a, b], axis=1)
    if n > 1:
        ab[1] = (D, D)  # a + b > D: the third value is simply negative
    return R.make_block(ab, bits, missing=sorted({0, n - 1, n // 2} if n > 3 else {0}))


def _decode(dev, nbytes, table, idx, rows, dtype, order, cols_total=None, col0=0):
    cols = len(table)
    cols_total = cols if cols_total is None else cols_total
    out = hbm.zeros((rows, cols_total, 3), dtype=dtype, order=order)
    table = np.ascontiguousarray(table, dtype=np.uint64)
    N.call("snpmi_dev_bgen_decode_" + N.suffix(dtype), N.ptr(dev), nbytes, N.ptr(table), cols,
           None if idx is None else N.ptr(idx), rows, N.ptr(out), cols_total, col0, 1 if order == "C" else 0)
    return out.get()


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [64, 65, 66, 67, 1])  # rows % 4 (and % 2): every F-order store form
def test_native_mixed_depths_shared_blocks_and_gather(n, dtype, order):
    rng = np.random.default_rng(n)
    depths = [32, 1, 9, 17, 31, 5]
    blocks = [_random_block(rng, n, b) for b in depths]
    dev, offsets, nbytes = _stage(blocks)
    pick = [0, 1, 2, 2, 3, 4, 5, 0]  # columns 2 and 3 name one block, as do 0 and 7
    table = [[offsets[k], depths[k], n] for k in pick]
    want = np.stack([R.decode_block(blocks[k]) for k in pick], axis=1)
    assert n == 1 or np.any(want[~np.isnan(want)] < 0)
    exact(_decode(dev, nbytes, table, None, n, dtype, order), want, dtype)
    # a gather index with repeats, reversed, on the host and in device memory
    for idx in (np.arange(n - 1, -1, -1), rng.integers(0, n, size=2 * n + 3), np.zeros(4, dtype=np.int64)):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        exact(_decode(dev, nbytes, table, idx, len(idx), dtype, order), want[idx.astype(np.int64)], dtype)
    idx_dev = hbm.asarray(np.arange(n - 1, -1, -1, dtype=np.uint64))
    exact(_decode(dev, nbytes, table, idx_dev, n, dtype, order), want[::-1], dtype)
    # into the middle of a wider array: only those SNPs are written
    wide = _decode(dev, nbytes, table[:3], None, n, dtype, order, cols_total=6, col0=2)
    exact(wide[:, 2:5], want[:, :3], dtype)
    assert not wide[:, :2].any() and not wide[:, 5:].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_native_tile_edges_and_many_blocks(dtype):
    """130 x 70: more than one 64 x 32 tile each way, neither a multiple; 1030 rows: several
    workgroups along a column in F order."""
    rng = np.random.default_rng(9)
    for n, m, bits in ((130, 70, 13), (1030, 3, 24)):
        blocks = [_random_block(rng, n, bits) for _ in range(m)]
        dev, offsets, nbytes = _stage(blocks)
        table = [[offsets[k], bits, n] for k in range(m)]
        want = np.stack([R.decode_block(b) for b in blocks], axis=1)
        for order in ("C", "F"):
            exact(_decode(dev, nbytes, table, None, n, dtype, order), want, dtype)


def test_native_refusals():
    blocks = [_random_block(np.random.default_rng(0), 8, 4)]
    dev, offsets, nbytes = _stage(blocks)
    ok = [[0, 4, 8]]
    for table, idx, rows, err in (([[4, 4, 8]], None, 8, IndexError),  # not on an 8-byte boundary
                                  ([[0, 33, 8]], None, 8, ValueError),  # bit depth
                                  ([[0, 4, 20]], None, 20, IndexError),  # the block would leave the buffer
                                  ([[8, 4, 8]], None, 8, IndexError),   # so would this one's spare bytes
                                  (ok, None, 9, IndexError),            # more rows than samples
                                  (ok, np.array([8], dtype=np.uint64), 1, IndexError)):
        with pytest.raises(err):
            _decode(dev, nbytes, table, idx, rows, np.float32, "F")
    with pytest.raises(IndexError):
        _decode(dev, nbytes - 8, ok, None, 8, np.float32, "F")


# ------------------------------------------------------------------------- fused routes
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_as_snp_read(dtype, order):
    bgen = Bgen(path("example"))
    triples = bgen.read(dtype=dtype, order="F").val
    want = dist_to_snp(triples, 0, 199, 2, order)
    for block_size in (None, 50):
        got = bgen.as_snp(max_weight=2, block_size=block_size).read(dtype=dtype, order=order).val
        assert isinstance(got, np.ndarray) and same_bits(got, want)
    sel = [7, 3, 3, 198]
    got = bgen[:, sel].as_snp(max_weight=2).read(dtype=dtype, order=order).val
    assert same_bits(got, dist_to_snp(np.asfortranarray(triples[:, sel]), 0, 4, 2, order))


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_as_snp_read_in_blocks(tmp_path, monkeypatch, dtype, order, on_device):
    """More SNPs than iids and a block_size below the SNP count that does not divide it: the block
    loop of ``_convert_generated`` (no fixture has sid_count > iid_count), to the host and to HBM."""
    n, m, block = 20, 60, 16
    bgen = Bgen.write(str(tmp_path / "wide.bgen"), _dist(n, m, 7), bits=9, compression="zlib")
    triples = bgen.read(dtype=dtype, order="F").val
    exact(triples, R.decode_file(bgen.filename), dtype)
    want = dist_to_snp(triples, 0, m, 2, order)
    sel = [59, 0, 31, 31] + list(range(3, 40))  # 41 SNPs: three blocks, the last of 9
    want_sel = dist_to_snp(np.asfortranarray(triples[:, sel]), 0, len(sel), 2, order)
    assert np.isnan(want).any() and np.isfinite(want).any()
    if on_device:
        monkeypatch.setenv("ARRAY_MODULE", "hbm")
    calls = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for reader, ref_val, launches in ((bgen, want, 4), (bgen[:, sel], want_sel, 3)):
        del calls[:]
        got = reader.as_snp(max_weight=2, block_size=block).read(dtype=dtype, order=order).val
        assert [c for c in calls if "bgen_decode" in c] == ["snpmi_dev_bgen_decode_" + N.suffix(dtype)] * launches
        assert isinstance(got, hbm.HbmArray if on_device else np.ndarray)
        if on_device:
            assert got.order == order
            got = got.get()
        assert got.flags["F_CONTIGUOUS" if order == "F" else "C_CONTIGUOUS"] and same_bits(got, ref_val)
        del calls[:]
        whole = reader.as_snp(max_weight=2).read(dtype=dtype, order=order).val  # no block_size: one launch
        assert len([c for c in calls if "bgen_decode" in c]) == 1
        assert same_bits(whole.get() if on_device else whole, ref_val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_read_kernel_equals_the_distdata_route(dtype):
    bgen = Bgen(path("big"))
    assert G.source_kind(bgen.as_snp()) == G.BGEN
    data = bgen.read(dtype=dtype)
    stored = DistData(iid=data.iid, sid=data.sid, val=data.val, pos=data.pos)
    # one chunk here, one whole block there (100 SNPs <= 2500 iids): the same add
    K = bgen.as_snp().read_kernel(Unit(), dtype=dtype).val
    Kref = stored.as_snp().read_kernel(Unit(), dtype=dtype).val
    assert K.shape == (2500, 2500) and np.isfinite(K).all() and same_bits(K, Kref)
    K2 = SnpKernel(bgen.as_snp(), Unit()).read(dtype=dtype).val
    K2ref = SnpKernel(stored.as_snp(), Unit()).read(dtype=dtype).val
    assert same_bits(K2, K2ref)


@pytest.mark.parametrize("dtype,tol", [(np.float32, 1e-5), (np.float64, 1e-10)])
def test_read_kernel_in_three_chunks(monkeypatch, dtype, tol):
    bgen = Bgen(path("big"))
    reader = bgen[:, ::-1].as_snp()  # any SNP selection: here reversed
    K1, trained1 = reader._read_kernel(Unit(), dtype=dtype, return_trained=True)
    monkeypatch.setattr(G, "BGEN_CHUNK_BYTES", 3 * 2500 * np.dtype(dtype).itemsize * 34)  # 34 + 34 + 32 SNPs
    bgen._run_once()
    assert len(list(bgen._chunks(np.arange(100), 2500, np.dtype(dtype).itemsize, G.BGEN_CHUNK_BYTES))) == 3
    calls = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    K3, trained3 = reader._read_kernel(Unit(), dtype=dtype, return_trained=True)
    assert [c for c in calls if "bgen_decode" in c or "add_dist" in c] == \
        ["snpmi_dev_bgen_decode_" + N.suffix(dtype), "snpmi_grm_add_dist_" + N.suffix(dtype)] * 3
    grm_close(K3, K1, tol)
    assert same_bits(trained3.stats, trained1.stats)  # per-SNP stats do not depend on the chunking
    # an iid subset takes the generic block loop and agrees with the rows of the triples
    sub = bgen[::5, :].as_snp().read_kernel(Unit(), dtype=dtype).val
    data = bgen[::5, :].read(dtype=dtype)
    ref_sub = DistData(iid=data.iid, sid=data.sid, val=data.val).as_snp().read_kernel(Unit(), dtype=dtype).val
    grm_close(sub, ref_sub, tol)


# ------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("bits", [1, 2, 8, 16, 32])
def test_round_trip_within_the_reference_tolerance(tmp_path, bits):
    """The reference's test_read_write_round_trip: atol = 1 / 2^b, times 1.4 at b = 1; the
    largest-remainder rule keeps every component within (2/3) / (2^b - 1), which is below it."""
    gen = DistGen(seed=332, iid_count=50, sid_count=5)
    want = gen.read().val
    bgen = Bgen.write(str(tmp_path / "rt.bgen"), gen, bits=bits, compression="zlib" if bits % 2 else None)
    got = bgen.read().val
    assert list(bgen.sid) == list(gen.sid) and [tuple(r) for r in bgen.iid] == [tuple(r) for r in gen.iid]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    atol = 1.0 / 2 ** bits * (1.4 if bits == 1 else 1.0)
    assert (2 / 3) / (2 ** bits - 1) <= atol
    err = np.nanmax(np.abs(got - want))
    print("bits", bits, "max error", err, "atol", atol)
    assert err <= atol


def test_bgen_to_bgen_is_exact_at_32_bits(tmp_path):
    src = Bgen(path("example"))[:, 10]
    want = src.read().val
    again = Bgen.write(str(tmp_path / "again.bgen"), src, bits=32, compression="zlib").read().val
    assert same_bits(again, want) and np.isfinite(want).all()  # (this SNP has no missing sample)


# ------------------------------------------------------------------------- empty selections
def test_empty_selections_launch_nothing(monkeypatch):
    bgen = Bgen(path("example"))
    bgen._run_once()
    calls = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for sel, shape in (((slice(None), []), (500, 0, 3)), (([], slice(None)), (0, 199, 3)), (([], []), (0, 0, 3))):
        for dtype in DTYPES:
            val = bgen[sel[0], sel[1]].read(dtype=dtype, order="C").val
            assert val.shape == shape and val.dtype == dtype
    assert bgen[:, []].as_snp().read().val.shape == (500, 0)
    assert not [c for c in calls if "decode" in c or "memcpy" in c]
