"""DistNpz: genotype distributions on disk as .npz (reference distreader/distnpz.py + pstreader/pstnpz.py).

Keys ``row``, ``col``, ``row_property``, ``col_property``, ``val`` (pstnpz.py:114-131).  Files are
loaded with ``allow_pickle=False``: ids are stored as NumPy string arrays, as the reference writes
them.
"""
import logging

import numpy as np

from pysnptools_amd.distreader.distreader import DistReader


class DistNpz(DistReader):
    def __init__(self, filename):
        super(DistNpz, self).__init__()
        self._ran_once = False
        self._filename = filename

    def __repr__(self):
        return "{0}('{1}')".format(self.__class__.__name__, self._filename)

    @property
    def filename(self):
        return self._filename

    def _run_once(self):
        if self._ran_once:
            return
        self._ran_once = True
        with np.load(self._filename, allow_pickle=False) as data:
            self._row = np.array(data["row"], dtype="str")
            self._col = np.array(data["col"], dtype="str")
            self._row_property = data["row_property"]
            self._col_property = data["col_property"]

    @property
    def row(self):
        self._run_once()
        return self._row

    @property
    def col(self):
        self._run_once()
        return self._col

    @property
    def row_property(self):
        self._run_once()
        return self._row_property

    @property
    def col_property(self):
        self._run_once()
        return self._col_property

    def copyinputs(self, copier):
        copier.input(self._filename)

    def _load_val(self):
        """The file's whole ``val`` (read fresh from disk on every call, as the reference does)."""
        with np.load(self._filename, allow_pickle=False) as data:
            return data["val"]

    _read_accepts_slices = True

    def _read(self, row_index_or_none, col_index_or_none, order, dtype, force_python_only, view_ok, num_threads):
        self._run_once()
        val, _ = self._apply_sparray_or_slice_to_val(self._load_val(), row_index_or_none, col_index_or_none, order,
                                                     np.dtype(dtype), force_python_only, num_threads)
        return val

    @staticmethod
    def write(filename, distdata):
        """Write a DistData (ids as byte-string arrays, as the reference does) and return the DistNpz."""
        from pysnptools_amd.util import asnumpy

        np.savez(filename, row=np.array(distdata.row, dtype="S"), col=np.array(distdata.col, dtype="S"),
                 row_property=distdata.row_property, col_property=distdata.col_property, val=asnumpy(distdata.val))
        logging.debug("Done writing " + filename)
        return DistNpz(filename)
