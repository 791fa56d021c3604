"""Readers of genotype distributions: a probability triple (0, 1 or 2 copies) per iid and SNP
(reference distreader/__init__.py).  ``as_snp`` turns a DistReader into a SnpReader of expected
values and ``SnpReader.as_dist`` goes the other way; both conversions, and the GRM of
``dist.as_snp()``, run on the GPU (csrc/dist.hip).  ``DistGen`` generates the reference's seeded
distributions in HBM (csrc/distgen.hip); ``Bgen`` decodes BGEN files into HBM (csrc/bgen.hip)."""
from pysnptools_amd.distreader.distreader import DistReader
from pysnptools_amd.distreader.distdata import DistData
from pysnptools_amd.distreader.distnpz import DistNpz
from pysnptools_amd.distreader.distmemmap import DistMemMap
from pysnptools_amd.distreader.distgen import DistGen
from pysnptools_amd.distreader.bgen import Bgen
from pysnptools_amd.distreader._subset import _DistSubset
from pysnptools_amd.distreader._snp2dist import _Snp2Dist
