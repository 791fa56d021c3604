"""SnpGen's host side (no GPU): metadata against the reference's, __repr__, block_size defaults,
the cache file, the deprecated argument, the seed range and the two C-ABI entry points."""
import os
import re

import numpy as np
import pytest

from conftest import DATA, GOLDEN, ROOT
from pysnptools_amd import _native as N
from pysnptools_amd.snpreader import SnpGen


def cases():
    return np.load(os.path.join(GOLDEN, "snpgen_cases.npz"), allow_pickle=False)


def test_pos_matches_the_reference():
    C = cases()
    assert np.array_equal(SnpGen(seed=0, iid_count=100, sid_count=100).pos, C["pos_0_100_100"], equal_nan=True)
    gen = SnpGen(seed=3, iid_count=10, sid_count=1000, chrom_count=5)
    assert np.array_equal(gen.pos, C["pos_3_10_1000_c5"], equal_nan=True)
    assert set(gen.pos[:, 0]) == {1.0, 2.0, 3.0, 4.0, 5.0} and np.isnan(gen.pos[:, 1]).all()
    assert gen.pos.shape == (1000, 3) and gen.col_property is gen.pos


def test_metadata_matches_the_files_the_reference_wrote():
    """dist_x.{fam,bim} are Bed.write of SnpGen(0, 100, 100)."""
    gen = SnpGen(seed=0, iid_count=100, sid_count=100)
    fam = [line.split() for line in open(os.path.join(DATA, "dist_x.fam")) if line.strip()]
    bim = [line.split() for line in open(os.path.join(DATA, "dist_x.bim")) if line.strip()]
    assert gen.iid_count == 100 and gen.sid_count == 100
    assert gen.iid.dtype.type is np.str_ and gen.iid.shape == (100, 2)
    assert [list(r) for r in gen.iid] == [f[:2] for f in fam]
    assert list(gen.sid) == [b[1] for b in bim]
    assert np.array_equal(gen.pos[:, 0], np.array([float(b[0]) for b in bim]))
    assert np.array_equal(gen.pos[:, 2], np.array([float(b[3]) for b in bim]))
    assert gen.iid[3, 1] == "iid_3" and gen.sid[7] == "sid_7"


def test_repr():
    assert repr(SnpGen(seed=0, iid_count=100, sid_count=100)) == \
        "SnpGen(seed=0,iid_count=100,sid_count=100,chrom_count=22,block_size=1000,cache_file=None)"
    assert repr(SnpGen(seed=5, iid_count=3, sid_count=9, chrom_count=2, block_size=4)) == \
        "SnpGen(seed=5,iid_count=3,sid_count=9,chrom_count=2,block_size=4,cache_file=None)"
    assert str(SnpGen(seed=5, iid_count=3, sid_count=9)[:, 1:3]).startswith("SnpGen(seed=5,")


@pytest.mark.parametrize("iid_count,block", [(0, 100000), (1, 100000), (99999, 1), (100000, 1), (100001, 1),
                                             (1000, 100), (3, 33333)])
def test_block_size_default(iid_count, block):
    assert SnpGen(seed=1, iid_count=iid_count, sid_count=10)._block_size == block
    assert SnpGen(seed=1, iid_count=iid_count, sid_count=10, block_size=7)._block_size == 7


def test_sid_batch_size_is_deprecated():
    with pytest.warns(DeprecationWarning, match="sid_batch_size"):
        gen = SnpGen(seed=1, iid_count=10, sid_count=10, sid_batch_size=5)
    assert gen._block_size == 5
    with pytest.warns(DeprecationWarning):
        assert SnpGen(seed=1, iid_count=10, sid_count=10, block_size=3, sid_batch_size=5)._block_size == 3


def test_cache_file_round_trip(tmp_path):
    path = str(tmp_path / "sub" / "cache.npz")
    a = SnpGen(seed=0, iid_count=12, sid_count=30, chrom_count=3, cache_file=path)
    assert os.path.exists(path)
    with np.load(path, allow_pickle=True) as z:
        assert sorted(z.files) == ["_col", "_col_property", "_row"]
    b = SnpGen(seed=0, iid_count=12, sid_count=30, chrom_count=3, cache_file=path)
    assert b._ran_once
    assert np.array_equal(a.iid, b.iid) and np.array_equal(a.sid, b.sid)
    assert np.array_equal(a.pos, b.pos, equal_nan=True)
    assert repr(b).endswith("cache_file={0})".format(path))
    with pytest.raises(AssertionError, match="iid in the cache file"):
        SnpGen(seed=0, iid_count=13, sid_count=30, cache_file=path)
    with pytest.raises(AssertionError, match="sid in the cache file"):
        SnpGen(seed=0, iid_count=12, sid_count=31, cache_file=path)

    class Copier(object):
        seen = []

        def input(self, item):
            self.seen.append(item)

    b.copyinputs(Copier())
    assert Copier.seen == [path]


def test_seed_out_of_range_is_a_host_side_value_error():
    """The second batch's seed is 2**32 + 1 (numpy: "Seed must be between 0 and 2**32 - 1");
    checked before anything is launched, so no device is needed to see it."""
    with pytest.raises(ValueError, match="Seed must be between 0 and 2"):
        SnpGen(seed=2 ** 32 - 1, iid_count=5, sid_count=4, block_size=2).read()
    with pytest.raises(ValueError, match="Seed must be between 0 and 2"):
        SnpGen(seed=-1, iid_count=5, sid_count=4, block_size=2)[:, :1].read()
    with pytest.raises(ValueError, match="Seed must be between 0 and 2"):
        SnpGen(seed=2 ** 32 - 1, iid_count=5, sid_count=4, block_size=2)._packed(np.array([3]))


def test_abi_lists_the_entry_points():
    text = open(os.path.join(ROOT, "include", "snpmi.h")).read()
    declared = set(re.findall(r"\b(snpmi_[a-z0-9_]+)\s*\(", text))
    for name in ("snpmi_dev_snpgen_bed", "snpmi_dev_mt19937_random_sample", "snpmi_dev_snpgen_rounds",
                 "snpmi_dev_memcpy_2d"):
        assert name in declared and name in N.symbols() and hasattr(N.lib(), name)
    assert len(N._SIGS["snpmi_dev_snpgen_bed"]) == 11 and len(N._SIGS["snpmi_dev_mt19937_random_sample"]) == 3


def test_maf_table_is_the_reference_distribution():
    x, cdf = SnpGen(seed=0, iid_count=1000, sid_count=10)._maf_tables()
    assert x.shape == cdf.shape == (100,) and x[0] == pytest.approx(1e-4) and x[-1] == pytest.approx(0.5)
    assert cdf[-1] == 1.0 and np.all(np.diff(cdf) > 0)
