"""Standardized genotypes as a linear operator: ``Z.T @ V``, ``Z @ W`` and ``K @ V = Z @ (Z.T @ V)``
computed from the packed 2-bit codes in HBM (``snpmi_dev_packed_tdot`` / ``snpmi_dev_packed_dot``,
include/snpmi.h).  Neither Z nor K is ever formed: the per-SNP score of an association scan, a
polygenic score, and the one product a conjugate-gradient or randomized-eigen LMM solver needs from K.

The reference has no counterpart; its callers use NumPy on ``SnpData.val`` (``snps.val.T.dot(y)``).
"""
import numpy as np

from pysnptools_amd import _grm as G
from pysnptools_amd import _native as N

SEGMENT = 256  # SNPs per segment of the Z W kernel: streamed chunks are whole segments (include/snpmi.h)
MATVEC_CHUNK_BYTES = 1 << 30  # packed source codes streamed per chunk (resident=False, and while loading)
_SOURCES = (G.BED, G.SNPGEN, G.SNPGEN_IIDS)


# ---------------------------------------------------------------------- operands and results
# The conventions of every packed-SNP product (SnpOperator, Pairs.rmatmat): NumPy or HbmArray in, the
# same kind out, a 1-D operand a 1-D result, empty products without device work.
def operand(a, rows, what, dtype, xp=None):
    """(the operand as a NumPy array or HbmArray, 1-D?, result in HBM?), checked before any device
    work."""
    from pysnptools_amd import hbm
    from pysnptools_amd.util import array_module

    if not isinstance(a, hbm.HbmArray):
        a = np.asarray(a)
    if a.ndim not in (1, 2):
        raise ValueError("%s takes a vector or a matrix, not %d dimensions" % (what, a.ndim))
    if a.dtype != dtype:
        raise ValueError("%s: the operator is %s, the operand %s" % (what, dtype, a.dtype))
    if a.shape[0] != rows:
        raise ValueError("%s: the operand has %d rows, the operator needs %d" % (what, a.shape[0], rows))
    to_hbm = isinstance(a, hbm.HbmArray) or array_module(xp) is hbm
    return a, a.ndim == 1, to_hbm


def empty_product(shape, rows, a, dtype):
    """The all-zero product of an empty sum or an empty shape (no device work), else None."""
    k = 1 if a.ndim == 1 else a.shape[1]
    if shape[0] and shape[1] and k:
        return None
    return np.zeros((rows, k), dtype=dtype, order="F")


def as_device(a):
    """``a`` as a 2-D F-order HbmArray (no copy when it already is one)."""
    from pysnptools_amd import hbm

    if isinstance(a, hbm.HbmArray):
        if a.ndim == 1:
            return hbm.HbmArray((a.shape[0], 1), a.dtype, "F", _base=a, _ptr=a.ptr)
        return a if a.order == "F" or 1 in a.shape else a.astype(a.dtype, order="F")
    a = a.reshape(-1, 1) if a.ndim == 1 else a
    return hbm.asarray(np.asfortranarray(a), order="F")


def as_result(out, one_d, to_hbm):
    from pysnptools_amd import hbm

    if isinstance(out, hbm.HbmArray) and not to_hbm:
        out = out.get()
    elif to_hbm and not isinstance(out, hbm.HbmArray):
        out = hbm.asarray(out, order="F")
    if not one_d:
        return out
    if isinstance(out, hbm.HbmArray):
        return hbm.HbmArray((out.shape[0],), out.dtype, "C", _base=out, _ptr=out.ptr)
    return out[:, 0]


class SnpOperator(object):
    """The ``N x M`` matrix Z of ``snpreader``'s values standardized by ``standardizer``, as an operator.

    :param snpreader: a :class:`Bed` or :class:`SnpGen`, or any iid / sid subset of one.  Any other
        reader raises ``TypeError``: there is no CPU fallback and no dense route.
    :param standardizer: ``Unit``, ``Beta``, their trained forms or ``Identity``.  Untrained ones
        train on the selected iids.
    :param dtype: ``float32`` or ``float64``; inputs must have it.
    :param resident: True -- the codes and value tables of all selected SNPs are loaded once, at the
        first use, and stay in HBM for the life of the operator (a solver that applies it hundreds of
        times).  False -- every call streams the SNPs in chunks of at most ``MATVEC_CHUNK_BYTES``.
        Both give the same bits.
    :param num_threads: host threads of the .bed gather.
    :param xp: ``"hbm"`` returns HbmArrays for NumPy inputs too (default: ``ARRAY_MODULE``).

    ``rmatmat(V)`` = Z.T V (M x k), ``matmat(W)`` = Z W (N x k), ``kernel_matmat(V)`` =
    ``matmat(rmatmat(V))`` = K V.  Inputs are NumPy arrays or HbmArrays of any order; a 1-D vector is
    one column and gives a 1-D result.  The result is an HbmArray when the input was one.
    """

    def __init__(self, snpreader, standardizer, dtype="float32", resident=True, num_threads=None, xp=None):
        dtype = np.dtype(dtype)
        G.require_float(dtype)
        p = G.plan(snpreader, standardizer, dtype) if hasattr(snpreader, "iid_count") else None
        if p is None or p.source not in _SOURCES:
            raise TypeError("SnpOperator takes a Bed or a SnpGen (or an iid / sid subset of one) and a Unit, Beta, "
                            "trained or Identity standardizer; got %s with %s. There is no dense or CPU route."
                            % (type(snpreader).__name__, type(standardizer).__name__))
        self._p, self.dtype, self.resident, self._num_threads, self._xp = p, dtype, bool(resident), num_threads, xp
        self.shape = (int(p.n), int(p.m))
        self._stats = p.stats()  # given (trained standardizers) or filled by the first pass over the SNPs
        self._have_stats = bool(p.use_stats)
        self._loaded = None

    # ------------------------------------------------------------------ public products
    def rmatmat(self, V):
        """Z.T V: the (M x k) per-SNP scores of the k columns of V (N x k)."""
        dev, one_d, to_hbm = self._operand(V, self.shape[0], "rmatmat")
        zero = self._empty(self.shape[1], dev)
        return self._result(self._tdot(dev) if zero is None else zero, one_d, to_hbm)

    def matmat(self, W):
        """Z W: the (N x k) predictions from the k columns of SNP weights W (M x k)."""
        dev, one_d, to_hbm = self._operand(W, self.shape[1], "matmat")
        zero = self._empty(self.shape[0], dev)
        return self._result(self._dot(dev) if zero is None else zero, one_d, to_hbm)

    def kernel_matmat(self, V):
        """K V with K = Z Z.T never formed: exactly ``matmat(rmatmat(V))``."""
        dev, one_d, to_hbm = self._operand(V, self.shape[0], "kernel_matmat")
        zero = self._empty(self.shape[0], dev)
        return self._result(self._dot(self._tdot(dev)) if zero is None else zero, one_d, to_hbm)

    @property
    def trained(self):
        """The trained standardizer (UnitTrained / BetaTrained / Identity) that
        ``read_kernel(return_trained=True)`` gives."""
        if not self._have_stats:
            for _ in self._chunks():
                pass
        return self._p.trained(self._stats)

    # ------------------------------------------------------------------ operands and results
    def _operand(self, a, rows, what):
        return operand(a, rows, what, self.dtype, self._xp)

    def _empty(self, rows, a):
        return empty_product(self.shape, rows, a, self.dtype)

    _device = staticmethod(as_device)
    _result = staticmethod(as_result)

    # ------------------------------------------------------------------ the two kernels over the chunks
    def _tdot(self, V):
        from pysnptools_amd import hbm

        V = self._device(V)
        n, m = self.shape
        k, item, dt = V.shape[1], self.dtype.itemsize, N.dt_code(self.dtype)
        out = hbm.empty((m, k), dtype=self.dtype, order="F")
        for s0, cnt, packed, pitch, lut in self._chunks():  # each chunk writes its own rows
            N.call("snpmi_dev_packed_tdot", N.ptr(packed), pitch, n, cnt, N.ptr(lut), dt, N.ptr(V), n, k,
                   _at(out, s0 * item), m)
        N.call("snpmi_stream_sync")
        return out

    def _dot(self, W):
        from pysnptools_amd import hbm

        W = self._device(W)
        n, m = self.shape
        k, item, dt = W.shape[1], self.dtype.itemsize, N.dt_code(self.dtype)
        out = hbm.empty((n, k), dtype=self.dtype, order="F")
        for s0, cnt, packed, pitch, lut in self._chunks():  # the chunks continue one fold over the segments
            N.call("snpmi_dev_packed_dot", N.ptr(packed), pitch, n, cnt, N.ptr(lut), dt, _at(W, s0 * item), m, k,
                   N.ptr(out), n, int(s0 > 0))
        N.call("snpmi_stream_sync")
        return out

    # ------------------------------------------------------------------ the SNPs in HBM
    def _chunks(self):
        """(first SNP, count, packed codes, pitch, value table) of every chunk, in SNP order: the one
        resident chunk, or the streamed ones."""
        if not self.resident:
            return self._stream()
        if self._loaded is None:
            self._loaded = self._load()
        return [self._loaded]

    def _load(self):
        packed, pitch, lut = G.load_packed(self._p, self.dtype, self._stats, MATVEC_CHUNK_BYTES, SEGMENT,
                                           self._num_threads)
        self._have_stats = True
        return 0, self.shape[1], packed, pitch, lut

    def _stream(self):
        """Chunk by chunk, by the loader every packed-SNP consumer shares (``_grm.packed_chunks``)."""
        for chunk in G.packed_chunks(self._p, self.dtype, self._stats, MATVEC_CHUNK_BYTES, SEGMENT, self._num_threads):
            yield chunk
        self._have_stats = True


_at = G.at
