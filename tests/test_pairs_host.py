"""Pairs (pysnptools_amd.snpreader.pairs) and its two C-ABI entries, as far as no device is needed: the
pair order against the reference's double loops (pairs.py:51-57, 68-73, written out below as data), the
closed-form pair <-> (i, j) maps and block tables, which sources it takes, the checks that come before
any device work, empty selections, and the ctypes binding."""
import ctypes
import os

import numpy as np
import pytest

from conftest import DATA, has_gpu_device
from pysnptools_amd import _native as N
from pysnptools_amd.snpreader import Bed, SnpData, SnpGen, SnpMemMap

BED = os.path.join(DATA, "n300.bed")
ONE = [0, 1, 2, 3, 7, 64, 65]
TWO = [(1, 1), (3, 5), (64, 2)]


def _bed():
    return Bed(BED, count_A1=False)


def brute_one(sid, singles):
    """The reference's loop over one reader: (sids, index0_list, index1_list)."""
    col, i0, i1 = [], [], []
    for index0 in range(len(sid)):
        start1 = index0 if singles else index0 + 1
        for index1 in range(start1, len(sid)):
            col.append("{0},{1}".format(sid[index0], sid[index1]))
            i0.append(index0)
            i1.append(index1)
    return np.array(col, dtype=str), np.array(i0, dtype=np.int64), np.array(i1, dtype=np.int64)


def brute_two(sid0, sid1):
    col, i0, i1 = [], [], []
    for index0 in range(len(sid0)):
        for index1 in range(len(sid1)):
            col.append("{0},{1}".format(sid0[index0], sid1[index1]))
            i0.append(index0)
            i1.append(index1)
    return np.array(col, dtype=str), np.array(i0, dtype=np.int64), np.array(i1, dtype=np.int64)


def test_exported_and_bound():
    from pysnptools_amd.snpreader import Pairs, _Pairs
    from pysnptools_amd.snpreader import pairs as module

    assert Pairs is _Pairs is module.Pairs
    assert module.PAIR_BLOCK >= 1
    lib = N.lib()
    for name, nargs in (("snpmi_dev_pair_values", 14), ("snpmi_dev_pair_tdot", 17)):
        assert name in N.symbols()
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
        assert fn.argtypes[0] is ctypes.c_void_p and fn.argtypes[1] is ctypes.c_uint64  # packed, pitch
    from pysnptools_amd import _grm as G

    assert G.PAIRS == "pairs" and G.PAIRS_CHUNK_BYTES == 1 << 30


@pytest.mark.parametrize("singles", [False, True], ids=["pairs", "singles"])
@pytest.mark.parametrize("m", ONE)
def test_one_reader_metadata_and_maps(m, singles):
    from pysnptools_amd.snpreader import Pairs
    from pysnptools_amd.snpreader.pairs import ij_to_pair, pair_to_ij

    gen = SnpGen(seed=3, iid_count=5, sid_count=70)[:, :m]
    pairs = Pairs(gen, _include_single_times_single=singles)
    col, i0, i1 = brute_one(gen.sid, singles)
    assert pairs.sid_count == len(col) == ((m * m + m) // 2 if singles else (m * m - m) // 2)
    assert pairs.iid_count == 5 and np.array_equal(pairs.iid, gen.iid)
    assert pairs.sid.shape == col.shape and np.array_equal(pairs.sid, col)
    assert pairs.pos.shape == (len(col), 3) and pairs.pos.dtype == np.int64 and not pairs.pos.any()
    i, j = pair_to_ij(np.arange(len(col)), m, None, singles)
    assert i.dtype == j.dtype == np.int64 and np.array_equal(i, i0) and np.array_equal(j, i1)
    assert np.array_equal(ij_to_pair(i0, i1, m, None, singles), np.arange(len(col)))
    assert np.array_equal(pairs.pair_to_ij(np.arange(len(col))), (i0, i1))  # the reader's own form of the maps
    assert np.array_equal(pairs.ij_to_pair(i0, i1), np.arange(len(col)))
    # the formula of the pair index, spelled out
    if not singles and len(col):
        assert np.array_equal(i0 * (m - 1) - i0 * (i0 - 1) // 2 + (i1 - i0 - 1), np.arange(len(col)))
    # any order, repeats, scalars
    if len(col):
        pick = np.array([len(col) - 1, 0, 0, len(col) // 2])
        i, j = pair_to_ij(pick, m, None, singles)
        assert np.array_equal(i, i0[pick]) and np.array_equal(j, i1[pick])


@pytest.mark.parametrize("m0,m1", TWO)
def test_two_reader_metadata_and_maps(m0, m1):
    from pysnptools_amd.snpreader import Pairs
    from pysnptools_amd.snpreader.pairs import ij_to_pair, pair_to_ij

    gen = SnpGen(seed=3, iid_count=4, sid_count=m0 + m1)
    r0, r1 = gen[:, :m0], gen[:, m0:]
    pairs = Pairs(r0, r1)
    col, i0, i1 = brute_two(r0.sid, r1.sid)
    assert pairs.sid_count == m0 * m1 == len(col)
    assert np.array_equal(pairs.sid, col) and np.array_equal(pairs.iid, gen.iid)
    assert pairs.pos.shape == (len(col), 3) and not pairs.pos.any()
    i, j = pair_to_ij(np.arange(len(col)), m0, m1)
    assert np.array_equal(i, i0) and np.array_equal(j, i1)
    assert np.array_equal(ij_to_pair(i0, i1, m0, m1), np.arange(len(col)))
    assert np.array_equal(pairs.pair_to_ij(np.arange(len(col))), (i0, i1))
    assert np.array_equal(pairs.ij_to_pair(i0, i1), np.arange(len(col)))
    assert np.array_equal(i0 * m1 + i1, np.arange(len(col)))


def test_maps_far_beyond_any_list():
    """M = 3,000,001 SNPs (4.5e12 pairs): the first and last pair of some rows, no list involved."""
    from pysnptools_amd.snpreader.pairs import ij_to_pair, pair_count, pair_to_ij

    m = 3000001
    for singles in (False, True):
        d = 0 if singles else 1
        rows = np.array([0, 1, 2, 1000, m // 2, m - 3, m - 2 - d + 1], dtype=np.int64)
        first = ij_to_pair(rows, rows + d, m, None, singles)
        last = ij_to_pair(rows, np.full_like(rows, m - 1), m, None, singles)
        assert last.max() == pair_count(m, None, singles) - 1 and first[0] == 0
        for idx, j_expected in ((first, rows + d), (last, np.full_like(rows, m - 1))):
            i, j = pair_to_ij(idx, m, None, singles)
            assert np.array_equal(i, rows) and np.array_equal(j, j_expected)


def _covered(blocks, count):
    """How often each pair index is written by the rectangles' tables."""
    seen = np.zeros(count, dtype=np.int64)
    for (a0, a1, b0, b1), (row_off, b_lo) in blocks:
        assert row_off.dtype == np.int64 and b_lo.dtype == np.uint32 and len(row_off) == len(b_lo) == a1 - a0
        for a in range(a1 - a0):
            for b in range(int(b_lo[a]), b1 - b0):
                row = int(row_off[a]) + b
                assert 0 <= row < count
                seen[row] += 1
    return seen


@pytest.mark.parametrize("block", [3, 64])
def test_block_tables_cover_every_pair_once(block):
    from pysnptools_amd.snpreader.pairs import block_tables, ij_to_pair

    for m in ONE:
        for singles in (False, True):
            _, i0, i1 = brute_one(np.arange(m), singles)
            blocks = []
            for a0 in range(0, m, block):
                for b0 in range(a0, m, block):  # only the blocks I <= J
                    r = (a0, min(a0 + block, m), b0, min(b0 + block, m))
                    blocks.append((r, block_tables(*r, m, None, singles)))
            assert (_covered(blocks, len(i0)) == 1).all(), (m, singles)
            # and each row is the pair it should be
            for (a0, a1, b0, b1), (row_off, b_lo) in blocks:
                for a in range(a1 - a0):
                    b = np.arange(int(b_lo[a]), b1 - b0)
                    assert np.array_equal(row_off[a] + b, ij_to_pair(np.full(len(b), a0 + a), b0 + b, m, None, singles))
    for m0, m1 in TWO:
        blocks = []
        for a0 in range(0, m0, block):
            for b0 in range(0, m1, block):
                r = (a0, min(a0 + block, m0), b0, min(b0 + block, m1))
                blocks.append((r, block_tables(*r, m0, m1)))
        assert (_covered(blocks, m0 * m1) == 1).all(), (m0, m1)


def test_reference_asserts():
    from pysnptools_amd.snpreader import Pairs

    gen, other = SnpGen(seed=1, iid_count=6, sid_count=8), SnpGen(seed=1, iid_count=7, sid_count=8)
    with pytest.raises(AssertionError, match="Expect snpreaders to have the same iids in the same order"):
        Pairs(gen[:, :4], other[1:, 4:]).iid
    with pytest.raises(AssertionError, match="Expect snpreaders to have the same iids in the same order"):
        Pairs(gen[:, :4], gen[::-1, 4:]).iid_count
    with pytest.raises(AssertionError, match="Pairs currently requires two snpreaders to have no sids in common"):
        Pairs(gen[:, :4], gen[:, 3:]).sid


def test_sid_raises_at_the_limit_sid_count_does_not():
    from pysnptools_amd.snpreader import Pairs

    gen = SnpGen(seed=1, iid_count=6, sid_count=5)  # 10 pairs
    assert len(Pairs(gen, sid_materialize_limit=11).sid) == 10
    at = Pairs(gen, sid_materialize_limit=10)
    assert at.sid_count == 10 and at.iid_count == 6
    with pytest.raises(AssertionError, match="10 is too many sids to materialize"):
        at.sid
    big = Pairs(SnpGen(seed=1, iid_count=6, sid_count=3000))
    assert big.sid_count == 4498500
    with pytest.raises(AssertionError, match="4,498,500 is too many sids to materialize"):
        big.sid


def test_other_sources_raise_type_error():
    from pysnptools_amd.distreader import DistGen
    from pysnptools_amd.snpreader import Pairs

    data = SnpData(iid=[["f", "a"], ["f", "b"]], sid=["s0", "s1", "s2"], val=np.array([[0., 1, 2], [2, 1, 0]]))
    with pytest.raises(TypeError, match="Bed or a SnpGen"):
        Pairs(data)
    with pytest.raises(TypeError, match="Bed or a SnpGen"):
        Pairs(data[:, 1:])
    with pytest.raises(TypeError, match="Bed or a SnpGen"):
        Pairs(_bed()[:, :3], data)
    with pytest.raises(TypeError, match="_Dist2Snp"):
        Pairs(DistGen(seed=1, iid_count=4, sid_count=3).as_snp())
    with pytest.raises(TypeError, match="ndarray"):
        Pairs(np.zeros((3, 2)))


def test_snpmemmap_raises_type_error(tmp_path):
    from pysnptools_amd.snpreader import Pairs

    data = SnpData(iid=[["f", "a"], ["f", "b"]], sid=["s0", "s1", "s2"], val=np.array([[0., 1, 2], [2, 1, 0]]))
    mm = SnpMemMap.write(str(tmp_path / "x.snp.memmap"), data)
    with pytest.raises(TypeError, match="SnpMemMap"):
        Pairs(mm)


def test_int8_and_bad_order_raise_value_error(monkeypatch):
    from pysnptools_amd.snpreader import Pairs

    pairs = Pairs(_bed()[:, :6])
    assert len(pairs.sid) == 15 and len(pairs.iid) == 300  # (the .fam / .bim are read natively)
    called = []
    monkeypatch.setattr(N, "call", lambda name, *a: called.append(name))
    with pytest.raises(ValueError, match="int8"):
        pairs.read(dtype=np.int8, _require_float32_64=False)
    with pytest.raises(ValueError, match="int8"):
        pairs[:, [3, 1]].read(dtype="int8", _require_float32_64=False)
    with pytest.raises(ValueError, match="order"):
        pairs._read(None, None, "K", np.float32, False, False, None)
    assert called == []


def test_rmatmat_operand_errors_come_before_any_device_work(monkeypatch):
    from pysnptools_amd.snpreader import Pairs

    pairs = Pairs(_bed()[::2, 5:17])
    assert pairs.iid_count == 150 and len(pairs.sid) == 66
    called = []
    monkeypatch.setattr(N, "call", lambda name, *a: called.append(name))
    with pytest.raises(ValueError, match="rows"):
        pairs.rmatmat(np.ones(151))
    with pytest.raises(ValueError, match="rows"):
        pairs.rmatmat(np.ones((149, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="float64"):
        pairs.rmatmat(np.ones(150, dtype=np.float32), dtype=np.float64)
    with pytest.raises(ValueError, match="float32 or float64"):
        pairs.rmatmat(np.ones((150, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="dimensions"):
        pairs.rmatmat(np.ones((150, 2, 2)))
    with pytest.raises(TypeError, match="subsetted inner readers"):
        pairs[:, :5].rmatmat(np.ones(150))
    with pytest.raises(TypeError, match="subsetted inner readers"):
        pairs[::2, :][:, :5].rmatmat(np.ones(75))
    assert called == []


def test_empty_selections_need_no_device(monkeypatch):
    from pysnptools_amd.snpreader import Pairs

    pairs, one = Pairs(_bed()[:, :6]), Pairs(_bed()[:, :1])  # one SNP: no pair
    none = Pairs(_bed()[:, []], _include_single_times_single=True)
    assert len(pairs.sid) == 15 and len(pairs.iid) == len(one.iid) == len(none.iid) == 300
    called = []
    monkeypatch.setattr(N, "call", lambda name, *a: called.append(name))
    for dtype in (np.float32, np.float64):
        for order in "FCA":
            v = pairs[:, []].read(dtype=dtype, order=order).val
            assert v.shape == (300, 0) and v.dtype == dtype
            v = pairs[[], :].read(dtype=dtype, order=order).val
            assert v.shape == (0, 15) and v.dtype == dtype
    assert one.sid_count == 0 and one.read().val.shape == (300, 0) and len(one.sid) == 0
    assert none.sid_count == 0 and none.read().val.shape == (300, 0)
    # empty scans: the zero product, 1-D for a vector
    g = one.rmatmat(np.ones(300, dtype=np.float32))
    assert g.shape == (0,) and g.dtype == np.float32
    assert one.rmatmat(np.ones((300, 3))).shape == (0, 3)
    assert pairs.rmatmat(np.ones((300, 0))).shape == (15, 0)
    assert called == []


@pytest.mark.skipif(has_gpu_device(), reason="checks the no-device error path")
def test_no_cpu_fallback_without_device():
    from pysnptools_amd.snpreader import Pairs
    from pysnptools_amd.standardizer import Unit

    pairs = Pairs(_bed()[:, :6])
    with pytest.raises(N.NativeError):
        pairs.read()
    with pytest.raises(N.NativeError):
        pairs.rmatmat(np.ones(300, dtype=np.float32))
    with pytest.raises(N.NativeError):
        pairs.read_kernel(Unit())
