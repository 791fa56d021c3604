"""In-memory genotype distributions (reference distreader/distdata.py)."""
import numpy as np

from pysnptools_amd.distreader.distreader import DistReader
from pysnptools_amd.pstreader import PstData


class DistData(PstData, DistReader):
    """iid x sid x 3 probabilities in memory (``val``: NumPy, or an HbmArray resident in the GPU's
    HBM), with ``iid`` (N x 2 str), ``sid`` and ``pos`` (M x 3)."""

    def __init__(self, iid, sid, val, pos=None, name=None, copyinputs_function=None, xp=None):
        self._val = None
        self._row = PstData._fixup_input(iid, empty_creator=lambda ignore: np.empty([0, 2], dtype="str"), dtype="str")
        self._col = PstData._fixup_input(sid, empty_creator=lambda ignore: np.empty([0], dtype="str"), dtype="str")
        self._row_property = PstData._fixup_input(None, count=len(self._row),
                                                  empty_creator=lambda count: np.empty([count, 0], dtype="str"),
                                                  dtype="str")
        self._col_property = PstData._fixup_input(pos, count=len(self._col),
                                                  empty_creator=lambda count: np.full([count, 3], np.nan))
        self._xp = xp
        self._val = self._fixup_val(val)
        self._assert_iid_sid_pos(check_val=True)
        self._name = name or ""
        self._std_string_list = []

    def _fixup_val(self, val):
        if val is None:
            assert len(self._row) == 0 or len(self._col) == 0, "If val is None, either row_count or col_count must be 0"
            val = np.empty([len(self._row), len(self._col), 3], dtype=np.float64)
        return PstData._fixup_input_val(val, row_count=len(self._row), col_count=len(self._col), xp=self._xp)

    @property
    def val(self):
        return self._val

    @val.setter
    def val(self, new_value):
        self._val = self._fixup_val(new_value)
        self._assert_iid_sid_pos(check_val=True)

    def allclose(self, value, equal_nan=True):
        """True when ids, positions and values (within NumPy's allclose) agree; NaN equals NaN
        unless ``equal_nan`` is False."""
        return PstData.allclose(self, value, equal_nan=equal_nan)

    def __repr__(self):
        stds = ",".join(self._std_string_list)
        if self._name == "":
            return "{0}({1})".format(self.__class__.__name__, stds)
        return "{0}({1}{2})".format(self.__class__.__name__, self._name, "," + stds if stds else "")
