"""``snpreader.as_dist()``: SNP values as one-hot genotype distributions (reference distreader/_snp2dist.py).

``_snpval_to_distval`` (_snp2dist.py:41-54) runs as ``snpmi_snp_to_dist_*``.  Over a Bed or a SnpGen
(or a subset of one) the values are decoded into HBM and converted there: they never exist on the
host.
"""
import numpy as np

from pysnptools_amd import _native as N
from pysnptools_amd.distreader.distreader import DistReader


def snp_to_dist(val, max_weight, order="A", to_hbm=None):
    """iid x sid x 3 one-hot triples of the iid x sid array ``val`` (NumPy or HbmArray, float32 /
    float64) in its dtype: slot c is 1 where val * (2 / max_weight) == c, and a value that matches no
    slot gives a NaN triple.  ``order`` 'A' follows ``val``; the result is an HbmArray when
    ``to_hbm`` (default: when ``val`` is one)."""
    from pysnptools_amd import hbm

    if order == "A":
        order = "C" if (val.flags["C_CONTIGUOUS"] and not val.flags["F_CONTIGUOUS"]) else "F"
    if not val.flags[order + "_CONTIGUOUS"]:
        val = np.asarray(val, order=order) if isinstance(val, np.ndarray) else hbm.asarray(val, order=order)
    rows, cols = int(val.shape[0]), int(val.shape[1])
    on_dev = isinstance(val, hbm.HbmArray) if to_hbm is None else to_hbm
    out = (hbm.empty if on_dev else np.empty)((rows, cols, 3), dtype=val.dtype, order=order)
    if rows and cols:
        N.call("snpmi_snp_to_dist_" + N.suffix(val.dtype), N.ptr(val), rows, cols, 1 if order == "C" else 0,
               float(max_weight), N.ptr(out))
    return out


class _Snp2Dist(DistReader):
    def __init__(self, snpreader, max_weight=2.0, block_size=None):
        super(_Snp2Dist, self).__init__()
        self.snpreader = snpreader
        self.max_weight = float(max_weight)  # a Python float: the factor is rounded to the value dtype
        self.block_size = block_size

    @property
    def row(self):
        return self.snpreader.iid

    @property
    def col(self):
        return self.snpreader.col

    @property
    def sid(self):
        return self.snpreader.sid

    @property
    def sid_count(self):
        return self.snpreader.sid_count

    @property
    def pos(self):
        return self.snpreader.pos

    @property
    def col_property(self):
        return self.snpreader.pos

    def __repr__(self):
        return "{0}.as_dist({1})".format(self.snpreader,
                                         "" if self.block_size is None else "block_size={0}".format(self.block_size))

    def copyinputs(self, copier):
        copier.input(self.snpreader)

    def __getitem__(self, iid_indexer_and_snp_indexer):
        iid_indexer, snp_indexer = iid_indexer_and_snp_indexer
        return _Snp2Dist(self.snpreader[iid_indexer, snp_indexer], max_weight=self.max_weight,
                         block_size=self.block_size)

    def _values(self, reader, order, dtype, force_python_only, num_threads):
        """``reader``'s values in ``order``: decoded straight into HBM when it is file- or
        generator-backed (Bed, SnpGen), else as the reference reads them."""
        from pysnptools_amd import _grm as G
        from pysnptools_amd.snpreader.snpreader import SnpReader, _resolve
        from pysnptools_amd.standardizer import Identity

        if not force_python_only and G.source_kind(*_resolve(reader)[:2]) in (G.BED, G.SNPGEN, G.SNPGEN_IIDS):
            return reader.read(order=order, dtype=dtype, num_threads=num_threads, xp="hbm").val
        snpdata, _ = SnpReader._as_snpdata(reader, dtype=dtype, order=order, force_python_only=force_python_only,
                                           standardizer=Identity(), num_threads=num_threads)
        return snpdata.val

    def _read(self, row_index_or_none, col_index_or_none, order, dtype, force_python_only, view_ok, num_threads):
        from pysnptools_amd import hbm
        from pysnptools_amd.util import _on_device

        assert row_index_or_none is None and col_index_or_none is None  # indexing is pushed to the snpreader
        dtype = np.dtype(dtype)
        if dtype not in (np.float32, np.float64):
            raise ValueError("dtype '{0}' not supported; use float32 or float64".format(dtype))
        order = "F" if order == "A" else order
        to_hbm = _on_device(getattr(self.snpreader, "val", None))
        # all at once unless the SNPs outnumber both the block and the iids (_snp2dist.py:61-62)
        if self.block_size is None or self.sid_count <= self.block_size or self.sid_count <= self.iid_count:
            val = self._values(self.snpreader, order, dtype, force_python_only, num_threads)
            return snp_to_dist(val, self.max_weight, order, to_hbm=to_hbm)
        out = np.zeros([self.iid_count, self.sid_count, 3], dtype=dtype, order=order)
        for start in range(0, self.sid_count, self.block_size):
            val = self._values(self.snpreader[:, start:start + self.block_size], order, dtype, force_python_only,
                               num_threads)
            out[:, start:start + val.shape[1]] = snp_to_dist(val, self.max_weight, order, to_hbm=False)
        return hbm.asarray(out, order=order) if to_hbm else out
