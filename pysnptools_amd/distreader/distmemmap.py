"""DistData kept in a memory-mapped file (reference distreader/distmemmap.py).

The file is a PstMemMap with ``val_shape`` 3 (pstreader/pstmemmap.py describes the format and how
its header is read without unpickling); ``*.dist.memmap`` files written by the reference open as
they are.  ``DistMemMap.write`` copies any DistReader into one, block by block.
"""
import logging
import os
import shutil

import numpy as np

from pysnptools_amd.distreader.distdata import DistData
from pysnptools_amd.pstreader.pstmemmap import PstMemMap


class DistMemMap(PstMemMap, DistData):
    """A DistData whose ``val`` is an ``np.memmap`` of a ``*.dist.memmap`` file."""

    def __init__(self, *args, **kwargs):
        super(DistMemMap, self).__init__(*args, **kwargs)

    @property
    def val(self):
        self._run_once()
        return self._val

    @val.setter
    def val(self, new_value):
        self._run_once()
        if self._val is new_value:
            return
        raise Exception("DistMemMap val's cannot be set to a different array")

    @property
    def offset(self):
        self._run_once()
        return self._offset

    @property
    def filename(self):
        return self._filename

    def _empty_inner(self, *args, **kwargs):
        PstMemMap._empty_inner(self, *args, **kwargs)
        self._row = np.array(self._row, dtype="str")
        self._col = np.array(self._col, dtype="str")
        self._std_string_list = []
        self._assert_iid_sid_pos(check_val=True)

    @staticmethod
    def empty(iid, sid, filename, pos=None, order="F", dtype=np.float64):
        """Create an empty DistMemMap on disk (distmemmap.py:96-126); fill ``val`` and ``flush``."""
        self = DistMemMap(filename)
        self._empty_inner(row=iid, col=sid, filename=filename, row_property=None, col_property=pos, order=order,
                          dtype=dtype, val_shape=3)
        return self

    def flush(self):
        """Flush ``val`` to disk and close the file (reopened on the next access)."""
        if self._ran_once:
            self.val.flush()
            del self._val
            self._ran_once = False

    @staticmethod
    def write(filename, distreader, order="A", dtype=None, block_size=None, num_threads=None):
        """Write a DistReader to DistMemMap format (distmemmap.py:183-233): in-memory values whole,
        other readers in blocks of ``block_size`` SNPs (default ~100k triples per block)."""
        from pysnptools_amd.util import asnumpy

        block_size = block_size or max(100_000 // max(1, distreader.row_count), 1)
        if hasattr(distreader, "val"):
            order = PstMemMap._order(distreader) if order == "A" else order
            dtype = dtype or distreader.val.dtype
        else:
            order = "F" if order == "A" else order
            dtype = dtype or np.float64
        dtype = np.dtype(dtype)
        mm = DistMemMap.empty(iid=distreader.iid, sid=distreader.sid, filename=filename + ".temp", pos=distreader.pos,
                              order=order, dtype=dtype)
        if hasattr(distreader, "val"):
            mm.val[:, :, :] = asnumpy(distreader.val)
        else:
            start = 0
            while start < distreader.sid_count:
                distdata = distreader[:, start:start + block_size].read(order=order, dtype=dtype,
                                                                        num_threads=num_threads)
                mm.val[:, start:start + distdata.sid_count, :] = asnumpy(distdata.val)
                start += distdata.sid_count
        mm.flush()
        if os.path.exists(filename):
            os.remove(filename)
        shutil.move(filename + ".temp", filename)
        logging.debug("Done writing " + filename)
        return DistMemMap(filename)

    def _run_once(self):
        if self._ran_once:
            return
        row, col, val, row_property, col_property = self._run_once_inner()
        DistData.__init__(self, iid=np.array(row, dtype="str"), sid=np.array(col, dtype="str"), val=val,
                          pos=col_property, name="np.memmap('{0}')".format(self._filename))
