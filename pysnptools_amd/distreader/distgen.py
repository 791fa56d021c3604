"""DistGen: deterministic synthetic genotype distributions, generated on the GPU (reference distreader/distgen.py).

``DistGen(seed, iid_count, sid_count)`` is a :class:`DistReader` whose values are a pure function of
``seed`` and ``block_size``: SNP ``s`` belongs to batch ``s // block_size``, and each batch -- always
``block_size`` SNPs, the reader's last one included -- is one MT19937 stream (numpy's legacy
``RandomState``) seeded with ``seed + batch * block_size``: ``random((iid_count, block_size, 3))``
normalised over its last axis, then ``rand(iid_count, block_size) < 0.218`` for the missing triples
(distgen.py:154-165).  The values are the reference's bit for bit, but the stream runs in HBM
(``snpmi_dev_distgen_*``, csrc/distgen.hip), one workgroup per batch, straight into the requested
dtype and order; ``as_snp()`` and its GRM read them there.  Only the metadata (iid, sid, pos) is
made on the host.
"""
import os

import numpy as np

from pysnptools_amd import _native as N
from pysnptools_amd.distreader.distreader import DistReader

_SEED_MAX = 2 ** 32 - 1
# approximate sizes of the human autosomes in base pairs (the proportions of `pos`)
_CHROM_MBP = (263, 255, 214, 203, 194, 183, 171, 155, 145, 144, 144, 143, 114, 109, 106, 98, 92, 85, 67, 72, 50, 56)


class DistGen(DistReader):
    """Generate deterministic "random" genotype distributions on the fly.

    :param seed: with *block_size*, determines the values
    :param iid_count, sid_count: the shape
    :param chrom_count: chromosomes in ``pos`` (at most 22)
    :param cache_file: optional ``.npz`` holding iid, sid and pos (created when missing)
    :param block_size: SNPs per batch; by default about 100,000 (iid, SNP) pairs per batch

    >>> from pysnptools_amd.distreader import DistGen
    >>> dist_gen = DistGen(seed=332, iid_count=1000, sid_count=1000*1000)
    >>> dist_data = dist_gen[:, 200*1000:201*1000].read()   # doctest: +SKIP
    """

    _chrom_size = np.array(_CHROM_MBP, dtype=np.int64) * int(1e6)

    def __init__(self, seed, iid_count, sid_count, chrom_count=22, cache_file=None, block_size=None):
        super(DistGen, self).__init__()
        self._ran_once = False
        self._cache_file = cache_file
        self._seed = seed
        self._iid_count = iid_count
        self._sid_count = sid_count
        self._chrom_count = chrom_count
        self._block_size = block_size or max(100000 // max(1, iid_count), 1)

        if cache_file is not None:
            if not os.path.exists(cache_file):
                directory = os.path.dirname(cache_file)
                if directory:
                    os.makedirs(directory, exist_ok=True)
                self._run_once()
                np.savez(cache_file, _row=self._row, _col=self._col, _col_property=self._col_property)
            else:
                with np.load(cache_file, allow_pickle=False) as data:
                    self._row = data["_row"]
                    assert len(self._row) == iid_count, "The iid in the cache file has a different length than iid_count"
                    self._col = data["_col"]
                    assert len(self._col) == sid_count, "The sid in the cache file has a different length than sid_count"
                    self._col_property = data["_col_property"]
                    assert len(self._col_property) == sid_count, \
                        "The pos in the cache file has a different length than sid_count"
                    self._ran_once = True

    def __repr__(self):
        return "{0}(seed={1},iid_count={2},sid_count={3},chrom_count={4},block_size={5},cache_file={6})".format(
            self.__class__.__name__, self._seed, self._iid_count, self._sid_count, self._chrom_count, self._block_size,
            self._cache_file)

    @property
    def row(self):
        self._run_once()
        return self._row

    @property
    def col(self):
        self._run_once()
        return self._col

    @property
    def col_property(self):
        self._run_once()
        return self._col_property

    def _run_once(self):
        """iid, sid and pos (distgen.py:84-103): as SnpGen's -- SNPs spread over the chromosomes in
        proportion to their sizes, evenly spaced from a per-chromosome random offset -- but with
        zeros, not NaN, in the genetic-distance column of ``pos`` (distgen.py:90)."""
        if self._ran_once:
            return
        self._ran_once = True
        self._row = np.array([("0", "iid_{0}".format(i)) for i in range(self._iid_count)])
        self._col = np.array(["sid_{0}".format(i) for i in range(self._sid_count)])
        pos = np.zeros((self._sid_count, 3))
        sizes = DistGen._chrom_size[:self._chrom_count]
        total = sizes.sum()
        step = total // self._sid_count
        ends = np.cumsum(sizes) * self._sid_count // total
        start = 0
        for chrom_index, stop in enumerate(int(e) for e in ends):
            offset = np.random.RandomState(chrom_index ^ 2292).randint(step)
            pos[start:stop, 0] = chrom_index + 1
            pos[start:stop, 2] = np.arange(0, stop - start) * step + offset + 1
            start = stop
        self._col_property = pos

    def copyinputs(self, copier):
        self._run_once()
        copier.input(self._cache_file)

    # ------------------------------------------------------------------ generation
    def _check_seeds(self, sid_index):
        """numpy's legacy seeding takes 0 .. 2**32-1: checked for every batch touched, before any launch."""
        if len(sid_index) == 0:
            return
        idx = np.asarray(sid_index)
        for sid in (int(idx.min()), int(idx.max())):
            batch_seed = self._seed + sid // self._block_size * self._block_size
            if batch_seed < 0 or batch_seed > _SEED_MAX:
                raise ValueError("Seed must be between 0 and 2**32 - 1")

    def _generate_into(self, out, sid_index):
        """The distributions of SNPs ``sid_index``, all iids, into the HbmArray ``out``
        (iid_count x len(sid_index) x 3, float32 / float64, C or F order)."""
        sid_index = np.asarray(sid_index)
        self._check_seeds(sid_index)
        idx = N.index_array(sid_index)
        assert tuple(out.shape) == (self._iid_count, len(idx), 3)
        if out.size:
            N.call("snpmi_dev_distgen_" + N.suffix(out.dtype), N.ptr(out), self._iid_count, int(self._seed),
                   int(self._block_size), N.ptr(idx), len(idx), 1 if out.order == "C" else 0)
        return out

    def _generate(self, sid_index, order, dtype):
        """A new HbmArray of the distributions of SNPs ``sid_index``, all iids."""
        from pysnptools_amd import hbm

        self._check_seeds(sid_index)  # before anything is allocated
        return self._generate_into(hbm.empty((self._iid_count, len(sid_index), 3), dtype=dtype, order=order),
                                   sid_index)

    def _read(self, row_index_or_none, col_index_or_none, order, dtype, force_python_only, view_ok, num_threads):
        from pysnptools_amd import hbm
        from pysnptools_amd.util import _on_device, sub_matrix

        dtype = np.dtype(dtype)
        if order == "A":
            order = "F"
        if dtype not in (np.float32, np.float64):
            raise ValueError("dtype '{0}' not supported; use float32 or float64".format(dtype))
        cols = np.arange(self._sid_count) if col_index_or_none is None else np.asarray(col_index_or_none)
        to_hbm = _on_device()
        rows = None if row_index_or_none is None else np.asarray(row_index_or_none)
        shape = (self._iid_count if rows is None else len(rows), len(cols), 3)
        if 0 in shape:
            self._check_seeds(cols)
            return (hbm.empty if to_hbm else np.empty)(shape, dtype=dtype, order=order)
        # every iid of the requested SNPs is generated; an iid subset is gathered from them in HBM
        val = self._generate(cols, order, dtype)
        if rows is not None:
            val = sub_matrix(val, rows, np.arange(len(cols)), order=order, dtype=dtype, num_threads=num_threads)
        return val if to_hbm else val.get()


def generated_range(distreader):
    """(DistGen, absolute SNP index array) when ``distreader`` is a DistGen, or a subset of one with
    every iid in order and any SNP selection; else None."""
    from pysnptools_amd.snpreader.snpreader import _resolve

    base, rows, cols = _resolve(distreader)
    if not isinstance(base, DistGen):
        return None
    if rows is not None and not np.array_equal(rows, np.arange(base.iid_count)):
        return None
    return base, (np.arange(base.sid_count) if cols is None else np.asarray(cols, dtype=np.int64))
