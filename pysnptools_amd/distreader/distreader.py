"""DistReader: iid x sid x 3 readers of genotype distributions (reference distreader/distreader.py)."""
import numpy as np

from pysnptools_amd.pstreader import PstReader


class DistReader(PstReader):
    """Reader of a probability triple per individual (iid) and SNP (sid): the chances of 0, 1 and 2
    copies of the counted allele."""

    def __init__(self, *args, **kwargs):
        super(DistReader, self).__init__(*args, **kwargs)

    @property
    def iid(self):
        return self.row

    @property
    def iid_count(self):
        return self.row_count

    @property
    def sid(self):
        return self.col

    @property
    def sid_count(self):
        return self.col_count

    @property
    def pos(self):
        return self.col_property

    @property
    def row_property(self):
        if not hasattr(self, "_row_property"):
            self._row_property = np.empty((self.row_count, 0))
        return self._row_property

    @property
    def val_shape(self):
        return 3

    def _read(self, iid_index_or_none, sid_index_or_none, order, dtype, force_python_only, view_ok, num_threads):
        raise NotImplementedError

    def read(self, order="F", dtype=np.float64, force_python_only=False, view_ok=False, num_threads=None):
        """Values as a :class:`DistData` (order 'F' | 'C' | 'A', dtype float64 | float32)."""
        from pysnptools_amd.distreader.distdata import DistData

        val = self._read(None, None, order, np.dtype(dtype), force_python_only, view_ok, num_threads)
        return DistData(self.iid, self.sid, val, pos=self.pos, name=str(self))

    def iid_to_index(self, list):
        return self.row_to_index(list)

    def sid_to_index(self, list):
        return self.col_to_index(list)

    def __getitem__(self, iid_indexer_and_snp_indexer):
        from pysnptools_amd.distreader._subset import _DistSubset

        iid_indexer, snp_indexer = iid_indexer_and_snp_indexer
        return _DistSubset(self, iid_indexer, snp_indexer)

    def as_snp(self, max_weight=2.0, block_size=None):
        """A SnpReader of the expected values: 0 * p0 + max_weight / 2 * p1 + max_weight * p2
        (distreader.py:296-322), converted on the GPU."""
        from pysnptools_amd.snpreader._dist2snp import _Dist2Snp

        return _Dist2Snp(self, max_weight=max_weight, block_size=block_size)

    @staticmethod
    def _as_distdata(distreader, force_python_only, order, dtype, num_threads):
        """``distreader`` itself when it already holds values of that dtype and order, else its read
        (distreader.py:364-376)."""
        dtype = np.dtype(dtype)
        if (hasattr(distreader, "val") and distreader.val.dtype == dtype
                and (order == "A" or (order == "C" and distreader.val.flags["C_CONTIGUOUS"])
                     or (order == "F" and distreader.val.flags["F_CONTIGUOUS"]))):
            return distreader
        return distreader.read(order=order, dtype=dtype, view_ok=True, num_threads=num_threads)

    def copyinputs(self, copier):
        raise NotImplementedError

    def _assert_iid_sid_pos(self, check_val):
        if check_val:
            assert len(self._val.shape) == 3 and self._val.shape[-1] == 3, \
                "val should have 3 dimensions and the last dimension should have size 3"
            assert tuple(self._val.shape) == (len(self._row), len(self._col), 3), \
                "val shape should match that of iid_count x sid_count"
        assert self._row.dtype.type is np.str_ and len(self._row.shape) == 2 and self._row.shape[1] == 2, \
            "iid should be dtype str, have two dimensions, and the second dimension should be size 2"
        assert self._col.dtype.type is np.str_ and len(self._col.shape) == 1, \
            "sid should be of dtype of str and one dimensional"
