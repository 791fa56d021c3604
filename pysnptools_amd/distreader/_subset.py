from pysnptools_amd.distreader.distreader import DistReader
from pysnptools_amd.pstreader._subset import _PstSubset


class _DistSubset(_PstSubset, DistReader):
    def __init__(self, *args, **kwargs):
        super(_DistSubset, self).__init__(*args, **kwargs)
