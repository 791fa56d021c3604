"""Host side of the distreader package (no GPU): the file formats, ids, subsets and the push-down of
selections through ``as_snp`` / ``as_dist``.  Nothing here computes.

``tiny.dist.memmap`` is the reference's own example file: 25 iids x 10 SNPs, the values of
``toydata10.dist.npz`` (the reference's TestDistMemMap.test1 asserts those counts).  The 2 x 3 file
of the reference's ``DistMemMap.empty`` docstring (distmemmap.py:113-118) is written and reopened
here."""
import os

import numpy as np
import pytest

from conftest import DATA
from pysnptools_amd.distreader import DistData, DistMemMap, DistNpz, DistReader, _DistSubset, _Snp2Dist
from pysnptools_amd.snpreader import Bed, SnpData
from pysnptools_amd.snpreader._dist2snp import _Dist2Snp

DOC_IID = [["fam0", "iid0"], ["fam0", "iid1"]]
DOC_SID = ["snp334", "snp349", "snp921"]
DOC_VAL = np.array([[[.5, .5, 0], [0, 0, 1], [.5, .5, 0]], [[0, 1., 0], [0, .75, .25], [.5, .5, 0]]])


def _fixture(name):
    return os.path.join(DATA, name)


def test_memmap_reads_the_reference_file():
    mm = DistMemMap(_fixture("tiny.dist.memmap"))
    assert (mm.iid_count, mm.sid_count, mm.val_shape) == (25, 10, 3)
    assert isinstance(mm.val, np.memmap) and mm.val.shape == (25, 10, 3) and mm.val.dtype == np.float64
    assert mm.val.flags["F_CONTIGUOUS"] and mm.offset == 2208
    assert mm.iid.dtype.type is np.str_ and list(mm.iid[0]) == ["per0", "per0"]
    assert mm.sid.dtype.type is np.str_ and list(mm.sid[:3]) == ["null_0", "null_1", "null_2"]
    assert mm.pos.shape == (10, 3) and list(mm.pos[1]) == [1, 0, 2]
    with np.load(_fixture("toydata10.dist.npz"), allow_pickle=False) as z:
        assert np.array_equal(mm.val, z["val"])
    np.testing.assert_allclose(mm.val.sum(axis=-1), 1.0, rtol=0, atol=1e-15)
    data = mm.read(view_ok=True)
    assert isinstance(data, DistData) and isinstance(data.val, np.memmap)


@pytest.mark.parametrize("name,shape,iid0,sid0,pos0", [
    ("toydata10.dist.npz", (25, 10), ["per0", "per0"], "null_0", [1, 0, 1]),
    ("distgen.dist.npz", (1000, 5), ["0", "iid_0"], "sid_0", [1, 0, 1025]),
])
def test_npz_reads_the_reference_files(name, shape, iid0, sid0, pos0):
    npz = DistNpz(_fixture(name))
    assert (npz.iid_count, npz.sid_count) == shape and npz.val_shape == 3
    assert npz.iid.dtype.type is np.str_ and npz.iid.shape == (shape[0], 2) and list(npz.iid[0]) == iid0
    assert npz.sid.dtype.type is np.str_ and npz.sid[0] == sid0
    assert npz.pos.shape == (shape[1], 3) and list(npz.pos[0]) == pos0
    assert list(npz.iid_to_index([npz.iid[3]])) == [3] and list(npz.sid_to_index([npz.sid[2]])) == [2]
    assert npz._load_val().shape == shape + (3,)


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_memmap_empty_flush_reopen(tmp_path, order, dtype):
    path = str(tmp_path / "doc.dist.memmap")
    mm = DistMemMap.empty(iid=DOC_IID, sid=DOC_SID, filename=path, order=order, dtype=dtype)
    assert isinstance(mm.val, np.memmap) and mm.val.shape == (2, 3, 3) and mm.val_shape == 3
    mm.val[:, :, :] = DOC_VAL
    mm.flush()
    assert isinstance(mm.val, np.memmap)  # reopened on access
    again = DistMemMap(path)
    assert again.filename == path and again.offset == mm.offset
    assert again.val.dtype == dtype and again.val.flags[order + "_CONTIGUOUS"]
    assert np.array_equal(again.val, DOC_VAL.astype(dtype))
    assert [list(r) for r in again.iid] == DOC_IID and list(again.sid) == DOC_SID
    assert again.pos.shape == (3, 0)  # no pos given: stored empty, as the reference stores it
    with pytest.raises(Exception, match="cannot be set to a different array"):
        again.val = np.zeros((2, 3, 3))
    # a memmap reads through NumPy: subsets need no GPU
    sub = again[[1], [1]].read(view_ok=True)
    assert np.array_equal(sub.val, np.array([[[0, .75, .25]]], dtype=dtype))


def test_memmap_write_of_a_reader(tmp_path):
    src = DistMemMap(_fixture("tiny.dist.memmap"))
    out = DistMemMap.write(str(tmp_path / "copy.dist.memmap"), src, order="C", dtype=np.float32)
    assert out.val.dtype == np.float32 and out.val.flags["C_CONTIGUOUS"]
    assert np.array_equal(out.val, src.val.astype(np.float32))
    assert np.array_equal(out.iid, src.iid) and np.array_equal(out.sid, src.sid) and np.array_equal(out.pos, src.pos)
    # a reader without `val` is written in blocks
    blocked = DistMemMap.write(str(tmp_path / "blocked.dist.memmap"), src[:, 2:9], block_size=3)
    assert np.array_equal(blocked.val, src.val[:, 2:9]) and blocked.val.flags["F_CONTIGUOUS"]
    assert list(blocked.sid) == list(src.sid[2:9])


def test_npz_write_read_round_trip(tmp_path):
    data = DistData(iid=DOC_IID, sid=DOC_SID, val=DOC_VAL, pos=[[1, 0, 10], [1, 0, 20], [2, 0, 5]])
    npz = DistNpz.write(str(tmp_path / "doc.dist.npz"), data)
    assert [list(r) for r in npz.iid] == DOC_IID and list(npz.sid) == DOC_SID
    assert np.array_equal(npz.pos, data.pos) and np.array_equal(npz._load_val(), DOC_VAL)
    with np.load(npz.filename, allow_pickle=False) as z:  # ids as byte strings, as the reference writes them
        assert z["row"].dtype.kind == "S" and z["col"].dtype.kind == "S"


def test_distdata_checks_and_repr():
    data = DistData(iid=DOC_IID, sid=DOC_SID, val=DOC_VAL, name="doc")
    assert isinstance(data, DistReader) and data.val_shape == 3 and repr(data) == "DistData(doc)"
    assert data.allclose(DistData(iid=DOC_IID, sid=DOC_SID, val=DOC_VAL + 1e-12))
    assert not data.allclose(DistData(iid=DOC_IID, sid=DOC_SID, val=DOC_VAL + 1e-3))
    nan = DOC_VAL.copy()
    nan[0, 0] = np.nan
    assert DistData(iid=DOC_IID, sid=DOC_SID, val=nan).allclose(DistData(iid=DOC_IID, sid=DOC_SID, val=nan))
    assert not DistData(iid=DOC_IID, sid=DOC_SID, val=nan).allclose(DistData(iid=DOC_IID, sid=DOC_SID, val=nan),
                                                                     equal_nan=False)
    with pytest.raises(AssertionError, match="val should have 3 dimensions and the last dimension should have size 3"):
        DistData(iid=DOC_IID, sid=DOC_SID, val=DOC_VAL[:, :, :2])
    with pytest.raises(AssertionError, match="val should have 3 dimensions"):
        DistData(iid=DOC_IID, sid=DOC_SID, val=DOC_VAL[:, :, 0])
    with pytest.raises(AssertionError):
        DistData(iid=DOC_IID, sid=DOC_SID[:2], val=DOC_VAL)
    with pytest.raises(AssertionError, match="iid should be dtype str"):
        DistData(iid=[["a", "b", "c"], ["d", "e", "f"]], sid=DOC_SID, val=DOC_VAL)
    same = DistReader._as_distdata(data, force_python_only=False, order="A", dtype=np.float64, num_threads=None)
    assert same is data


def test_subsets_compose_and_as_snp_pushes_down():
    mm = DistMemMap(_fixture("tiny.dist.memmap"))
    sub = mm[::2, 1:9][[3, 1], ::2]
    assert isinstance(sub, _DistSubset) and sub.val_shape == 3
    assert [list(r) for r in sub.iid] == [list(mm.iid[6]), list(mm.iid[2])]
    assert list(sub.sid) == [mm.sid[1], mm.sid[3], mm.sid[5], mm.sid[7]]
    assert np.array_equal(sub.pos, mm.pos[[1, 3, 5, 7]])
    assert np.array_equal(sub.read().val, mm.val[[6, 2]][:, [1, 3, 5, 7]])

    snp = mm.as_snp(max_weight=1, block_size=4)
    assert isinstance(snp, _Dist2Snp) and snp.max_weight == 1.0 and isinstance(snp.max_weight, float)
    assert (snp.iid_count, snp.sid_count) == (25, 10) and np.array_equal(snp.pos, mm.pos)
    assert repr(snp) == "DistMemMap('%s').as_snp(block_size=4)" % _fixture("tiny.dist.memmap")
    picked = snp[[4, 0], 2:5]
    assert isinstance(picked, _Dist2Snp) and isinstance(picked.distreader, _DistSubset)
    assert picked.max_weight == 1.0 and picked.block_size == 4
    assert [list(r) for r in picked.iid] == [list(mm.iid[4]), list(mm.iid[0])]
    assert list(picked.sid) == list(mm.sid[2:5])
    assert repr(mm.as_snp()).endswith(".as_snp()")


def test_as_dist_pushes_down():
    bed = Bed(os.path.join(DATA, "n300.bed"), count_A1=False)
    dist = bed.as_dist(max_weight=2, block_size=7)
    assert isinstance(dist, _Snp2Dist) and isinstance(dist, DistReader) and dist.val_shape == 3
    assert (dist.iid_count, dist.sid_count) == (300, 1015) and isinstance(dist.max_weight, float)
    sub = dist[10:20, [5, 3]]
    assert isinstance(sub, _Snp2Dist) and sub.block_size == 7
    assert np.array_equal(sub.iid, bed.iid[10:20]) and list(sub.sid) == [bed.sid[5], bed.sid[3]]
    assert np.array_equal(sub.pos, bed.pos[[5, 3]])
    assert repr(sub).endswith(".as_dist(block_size=7)")
    back = sub.as_snp()
    assert isinstance(back, _Dist2Snp) and back.sid_count == 2
    data = SnpData(iid=DOC_IID, sid=DOC_SID, val=np.zeros((2, 3)))
    assert isinstance(data.as_dist(), _Snp2Dist)
