"""Pairs: one column per SNP pair, the elementwise product of two standardized SNP columns
(reference snpreader/pairs.py), served from the packed 2-bit codes in HBM.

The reference reads the inner SNPs into host floats, standardizes them and multiplies the columns
(pairs.py:135-152); its own use is the epistasis scan ``epi_reml`` (pairs.py:282-308).  Here a pair's
column is two code words and two 4-entry value tables: ``read`` writes any pair list at the store
rate (``snpmi_dev_pair_values``), and ``rmatmat`` -- the scan Zp.T V over ALL pairs -- never writes
a pair column at all (``snpmi_dev_pair_tdot``), so it works far beyond ``sid_materialize_limit``.

The pair <-> (i, j) maps below are closed forms; nothing goes through the list of sids (the
reference's ``index0_list`` / ``index1_list`` loops, pairs.py:51-57, 68-73).
"""
import numpy as np

from pysnptools_amd import _grm as G
from pysnptools_amd import _native as N
from pysnptools_amd import linop
from pysnptools_amd.snpreader._subset import _SnpSubset
from pysnptools_amd.snpreader.snpreader import SnpReader

PAIR_BLOCK = 4096  # SNPs per side of one snpmi_dev_pair_tdot rectangle of the scan
LOAD_CHUNK_BYTES = 1 << 30  # packed source codes per chunk while the inner SNPs are loaded
_SOURCES = (G.BED, G.SNPGEN, G.SNPGEN_IIDS)


# ---------------------------------------------------------------------- pair order, in closed form
# One reader of M SNPs: pairs (i, j) with j >= i + d, ordered by i then j; d = 0 with singles, else 1.
# Left SNP i owns the M - d - i consecutive pairs from _first(i) = i (M - d) - i (i - 1) / 2 on.
# Two readers of M0 and M1 SNPs: pair i M1 + j.
def pair_count(m0, m1=None, singles=False):
    if m1 is not None:
        return m0 * m1
    return (m0 * m0 + m0) // 2 if singles else (m0 * m0 - m0) // 2


def _first(i, m, d):
    return i * (m - d) - i * (i - 1) // 2


def ij_to_pair(i, j, m0, m1=None, singles=False):
    """Pair index of (i, j) (int64 arrays): the inverse of ``pair_to_ij``."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    if m1 is not None:
        return i * m1 + j
    d = 0 if singles else 1
    return _first(i, m0, d) + (j - i - d)


def pair_to_ij(index, m0, m1=None, singles=False):
    """(i, j) of pair ``index`` (int64 arrays): SNP i of the left reader and j of the right one (of
    the same reader when there is one)."""
    index = np.asarray(index, dtype=np.int64)
    if m1 is not None:
        return index // max(m1, 1), index % max(m1, 1)
    d = 0 if singles else 1
    # the largest i with _first(i) <= index: the root of i (2 (M - d) + 1 - i) / 2 = index in float64,
    # then corrected in integers (the root is off by at most a few near a row's first pair)
    b = 2.0 * (m0 - d) + 1.0
    i = np.floor((b - np.sqrt(np.maximum(b * b - 8.0 * index, 0.0))) / 2.0).astype(np.int64)
    i = np.clip(i, 0, max(m0 - 1, 0))
    for _ in range(4):
        i = i - (_first(i, m0, d) > index)
        i = i + (_first(i + 1, m0, d) <= index)
    return i, index - _first(i, m0, d) + i + d


def block_tables(a0, a1, b0, b1, m0, m1=None, singles=False):
    """(row_off int64 [a1 - a0], b_lo uint32 [a1 - a0]) of the rectangle of left SNPs [a0, a1) and
    right SNPs [b0, b1) for ``snpmi_dev_pair_tdot``: pair (a0 + a, b0 + b) is row ``row_off[a] + b`` of
    the reader's pair order, and exists for ``b >= b_lo[a]``."""
    a = np.arange(a0, a1, dtype=np.int64)
    if m1 is not None:
        return a * m1 + b0, np.zeros(len(a), dtype=np.uint32)
    d = 0 if singles else 1
    return _first(a, m0, d) - a - d + b0, np.clip(a + d - b0, 0, b1 - b0).astype(np.uint32)


class Pairs(SnpReader):
    """The SNP pairs of ``snpreader0`` (with itself), or of ``snpreader0`` x ``snpreader1``.

    :param snpreader0, snpreader1: each a :class:`Bed` or :class:`SnpGen`, or an iid / sid subset of
        one (what :class:`SnpOperator` takes).  Any other reader raises ``TypeError``: there is no
        dense route and no CPU fallback.
    :param do_standardize: True -- each inner SNP is Unit-standardized on the iids read, as
        ``snpreader0[iid_index, inner].read().standardize()`` is in the reference.  False -- the raw
        0 / 1 / 2 values (a Bed's ``count_A1`` honoured), NaN for a missing genotype.
    :param sid_materialize_limit: ``sid`` raises at this many pairs; ``sid_count``, ``read`` and
        ``rmatmat`` do not need the sids.  ``read_kernel`` does (its trained standardizer is over the
        pairs' sids), so it raises there too, as the reference's does.
    :param _include_single_times_single: also the squares (i, i).

    With one reader the pairs are (i, j), i < j, ordered by i then j; with two, i M1 + j.
    """

    def __init__(self, snpreader0, snpreader1=None, do_standardize=True, sid_materialize_limit=1000 * 1000,
                 _include_single_times_single=False):
        super(Pairs, self).__init__()
        self._ran_once = False
        self.snpreader0 = snpreader0
        self.snpreader1 = snpreader1
        self.do_standardize = do_standardize
        self.sid_materialize_limit = sid_materialize_limit
        self._include_single_times_single = _include_single_times_single
        for reader in (snpreader0,) + (() if snpreader1 is None else (snpreader1,)):
            _check_source(reader)
        self._sides = {}  # dtype -> the resident inner SNPs of the scan

    def __repr__(self):
        part2 = "" if self.snpreader1 is None else ",{0}".format(self.snpreader1)
        return "{0}({1}{2})".format(self.__class__.__name__, self.snpreader0, part2)

    # ------------------------------------------------------------------ metadata (pairs.py:31-98)
    def pair_to_ij(self, index):
        """(i, j) of pairs ``index``: SNP i of ``snpreader0`` and SNP j of ``snpreader1`` (of
        ``snpreader0`` when there is one reader), in closed form -- no sid is materialized."""
        return pair_to_ij(index, *self._counts)

    def ij_to_pair(self, i, j):
        """The pair index of SNPs (i, j): the inverse of ``pair_to_ij``."""
        return ij_to_pair(i, j, *self._counts)

    @property
    def _counts(self):
        """(M0, M1 or None, singles): the arguments of the closed-form maps."""
        m1 = None if self.snpreader1 is None else int(self.snpreader1.col_count)
        return int(self.snpreader0.col_count), m1, bool(self._include_single_times_single)

    @property
    def row(self):
        if not hasattr(self, "_row"):
            row = self.snpreader0.row
            if self.snpreader1 is not None and not np.array_equal(row, self.snpreader1.row):
                raise AssertionError("Expect snpreaders to have the same iids in the same order")
            self._row = row
        return self._row

    @property
    def col(self):
        if not hasattr(self, "_col"):
            if self.col_count >= self.sid_materialize_limit:
                raise AssertionError("{:,} is too many sids to materialize".format(self.col_count))
            col_0 = np.asarray(self.snpreader0.col)
            col_1 = col_0 if self.snpreader1 is None else np.asarray(self.snpreader1.col)
            if self.snpreader1 is not None and len(set(col_0) & set(col_1)) != 0:
                raise AssertionError("Pairs currently requires two snpreaders to have no sids in common")
            i, j = pair_to_ij(np.arange(self.col_count, dtype=np.int64), *self._counts)
            self._col = (np.char.add(np.char.add(col_0[i].astype(str), ","), col_1[j].astype(str))
                         if self.col_count else np.array([], dtype=str))
        return self._col

    @property
    def col_count(self):
        return pair_count(*self._counts)

    @property
    def row_count(self):
        return len(self.row)

    @property
    def col_property(self):
        if not hasattr(self, "_col_property"):
            self._col_property = np.zeros([self.sid_count, 3], dtype=np.int64)
        return self._col_property

    def copyinputs(self, copier):
        self.snpreader0.copyinputs(copier)
        if self.snpreader1 is not None:
            self.snpreader1.copyinputs(copier)

    def _run_once(self):
        if self._ran_once:
            return
        self._ran_once = True
        self.col

    def __getitem__(self, iid_indexer_and_snp_indexer):
        return _PairsSubset(self, *iid_indexer_and_snp_indexer)

    # ------------------------------------------------------------------ values (pairs.py:113-153)
    def _read(self, iid_index_or_none, sid_index_or_none, order, dtype, force_python_only, view_ok, num_threads):
        return self._values(iid_index_or_none, sid_index_or_none, order, dtype, num_threads=num_threads)

    def _values(self, iid_index, sid_index, order, dtype, to_hbm=False, num_threads=None):
        """The values of pairs ``sid_index`` at iids ``iid_index`` (None = all), on the host or in HBM.
        The unique inner SNPs the request names are loaded at the selected iids (so Unit trains on
        them) -- or, with all iids once the scan's resident SNPs exist, those are used -- and one
        ``snpmi_dev_pair_values`` writes the request."""
        from pysnptools_amd import hbm

        dtype = np.dtype(dtype)
        if dtype not in (np.float32, np.float64):
            raise ValueError("dtype '{0}' not supported; Pairs serves float32 and float64".format(dtype))
        if order not in ("F", "C", "A"):
            raise ValueError("order '{0}' not supported; use 'F', 'C' or 'A'".format(order))
        order = "F" if order == "A" else order
        n = self.iid_count if iid_index is None else len(iid_index)
        sids = np.arange(self.sid_count, dtype=np.int64) if sid_index is None else np.asarray(sid_index, dtype=np.int64)
        count = len(sids)
        if n == 0 or count == 0:
            return (hbm.empty if to_hbm else np.empty)((n, count), dtype=dtype, order=order)
        i, j = pair_to_ij(sids, *self._counts)
        if iid_index is None and dtype in self._sides:
            side0, side1 = self._sides[dtype]
        elif self.snpreader1 is None:
            inner = np.unique(np.r_[i, j])
            side0 = side1 = self._load(self.snpreader0, iid_index, inner, dtype, num_threads)
            i, j = np.searchsorted(inner, i), np.searchsorted(inner, j)
        else:
            inner0, inner1 = np.unique(i), np.unique(j)
            side0 = self._load(self.snpreader0, iid_index, inner0, dtype, num_threads)
            side1 = self._load(self.snpreader1, iid_index, inner1, dtype, num_threads)
            i, j = np.searchsorted(inner0, i), np.searchsorted(inner1, j)
        idx0 = hbm.asarray(np.ascontiguousarray(i, dtype=np.uint32))
        idx1 = hbm.asarray(np.ascontiguousarray(j, dtype=np.uint32))

        def write(out, order_c, ld):
            N.call("snpmi_dev_pair_values", N.ptr(side0[0]), side0[1], N.ptr(side0[2]), N.ptr(side1[0]), side1[1],
                   N.ptr(side1[2]), n, N.ptr(idx0), N.ptr(idx1), count, N.dt_code(dtype), order_c, N.ptr(out), ld)

        out = hbm.empty((n, count), dtype=dtype, order=order)
        if order == "C":
            write(out, 1, count)
        elif n % 16 == 0:
            write(out, 0, n)
        else:
            # F-order columns start 16-element aligned on the device; a device 2-D copy drops the pad rows
            ld = (n + 15) // 16 * 16
            padded = hbm.empty((ld, count), dtype=dtype, order="F")
            write(padded, 0, ld)
            N.call("snpmi_dev_memcpy_2d", N.ptr(out), n * dtype.itemsize, N.ptr(padded), ld * dtype.itemsize,
                   n * dtype.itemsize, count)
        N.call("snpmi_stream_sync")
        return out if to_hbm else out.get()

    def _load(self, reader, iid_index, sid_index, dtype, num_threads=None):
        """(packed codes, pitch, value table) in HBM of SNPs ``sid_index`` (None = all) of ``reader`` at
        iids ``iid_index`` (None = all): the loader SnpOperator uses, with Unit or Identity."""
        from pysnptools_amd.standardizer import Identity, Unit

        if iid_index is not None or sid_index is not None:
            reader = reader[slice(None) if iid_index is None else iid_index,
                            slice(None) if sid_index is None else sid_index]
        p = G.plan(reader, Unit() if self.do_standardize else Identity(), dtype)
        return G.load_packed(p, dtype, p.stats(), LOAD_CHUNK_BYTES, 1, num_threads)

    def _resident(self, dtype):
        """The two sides' inner SNPs, all iids: loaded once per dtype, kept for the life of the reader."""
        dtype = np.dtype(dtype)
        if dtype not in self._sides:
            side0 = self._load(self.snpreader0, None, None, dtype)
            side1 = side0 if self.snpreader1 is None else self._load(self.snpreader1, None, None, dtype)
            self._sides[dtype] = (side0, side1)
        return self._sides[dtype]

    # ------------------------------------------------------------------ the scan
    def rmatmat(self, V, dtype=None):
        """Zp.T V: the (``sid_count`` x k) scores of the k columns of V (``iid_count`` x k) against
        every pair, in the reader's pair order -- the per-pair statistic of an epistasis scan.  No pair
        column is written, so this works beyond ``sid_materialize_limit``.

        V is a NumPy array or an HbmArray of ``dtype`` (default: V's own; float32 or float64); a 1-D
        operand gives a 1-D result, and the result is an HbmArray when the operand was one
        (:class:`SnpOperator`'s conventions).  The inner SNPs are loaded once and stay in HBM for the
        life of the reader; the scan runs over block pairs of at most ``PAIR_BLOCK`` SNPs.

        Defined on the Pairs itself, not on ``pairs[:, idx]``: to restrict iids or SNPs build the Pairs
        from subsetted inner readers, as ``epi_reml`` does (``Pairs(part_i, part_j)``)."""
        from pysnptools_amd import hbm

        if dtype is None:
            dtype = V.dtype if hasattr(V, "dtype") else np.asarray(V).dtype
        dtype = np.dtype(dtype)
        if dtype not in (np.float32, np.float64):
            raise ValueError("rmatmat: dtype must be float32 or float64, not %s" % dtype)
        n, count = int(self.iid_count), int(self.sid_count)
        dev, one_d, to_hbm = linop.operand(V, n, "rmatmat", dtype)
        zero = linop.empty_product((n, count), count, dev, dtype)
        if zero is not None:
            return linop.as_result(zero, one_d, to_hbm)
        (pk_a, pitch_a, lut_a), (pk_b, pitch_b, lut_b) = self._resident(dtype)
        Vd = linop.as_device(dev)
        k, item, dt = Vd.shape[1], dtype.itemsize, N.dt_code(dtype)
        out = hbm.empty((count, k), dtype=dtype, order="F")
        m0, m1, singles = self._counts
        mb = m0 if m1 is None else m1
        keep = []  # the rectangles' tables, alive until the stream has drained
        for a0 in range(0, m0, PAIR_BLOCK):
            a1 = min(a0 + PAIR_BLOCK, m0)
            for b0 in range(a0 if m1 is None else 0, mb, PAIR_BLOCK):  # one reader: only the blocks I <= J
                b1 = min(b0 + PAIR_BLOCK, mb)
                row_off, b_lo = block_tables(a0, a1, b0, b1, m0, m1, singles)
                _check_tables(row_off, b_lo, b1 - b0, count)
                ro = hbm.asarray(row_off)
                lo = hbm.asarray(b_lo) if b_lo.any() else None  # (off-diagonal: every b)
                keep += [ro, lo]
                N.call("snpmi_dev_pair_tdot", G.at(pk_a, a0 * pitch_a), pitch_a, G.at(lut_a, 4 * a0 * item), a1 - a0,
                       G.at(pk_b, b0 * pitch_b), pitch_b, G.at(lut_b, 4 * b0 * item), b1 - b0, n, N.ptr(ro), N.ptr(lo),
                       dt, N.ptr(Vd), n, k, N.ptr(out), count)
        N.call("snpmi_stream_sync")
        return linop.as_result(out, one_d, to_hbm)


_Pairs = Pairs  # the reference's name


def _check_source(reader):
    from pysnptools_amd.snpreader.snpreader import _resolve

    kind = G.source_kind(*_resolve(reader)[:2]) if hasattr(reader, "iid_count") else None
    if kind not in _SOURCES:
        raise TypeError("Pairs takes a Bed or a SnpGen (or an iid / sid subset of one) as inner reader; got %s. "
                        "There is no dense or CPU route." % type(reader).__name__)


def _check_tables(row_off, b_lo, nb, count):
    """Every row a rectangle writes lies inside the result: row_off[a] + b for b_lo[a] <= b < nb."""
    on = b_lo < nb
    if on.any():
        first, last = row_off[on] + b_lo[on], row_off[on] + (nb - 1)
        if first.min() < 0 or last.max() >= count:
            raise ValueError("pair rectangle writes outside the %d pairs" % count)


class _PairsSubset(_SnpSubset):
    """``pairs[iids, idx]``: read through ``Pairs._read``; the scan is not defined on it."""

    def __getitem__(self, iid_indexer_and_snp_indexer):
        return _PairsSubset(self, *iid_indexer_and_snp_indexer)

    def rmatmat(self, V, dtype=None):
        raise TypeError("rmatmat is defined on the Pairs itself, not on a subset of it: build the Pairs from "
                        "subsetted inner readers instead, Pairs(snps[iids, part_i], snps[iids, part_j])")
