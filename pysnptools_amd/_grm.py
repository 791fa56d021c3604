"""What every Python GRM route shares: the plan (which native GRM entry serves a reader /
standardizer / dtype, and with what), the session (begin ... add ... end, whole K or K[rows, cols])
and the feeders (one loop per source kind that adds the source's SNPs to a session).

The routes themselves stay where they are -- ``snpreader._native_grm`` and the generic block loop,
``kernelreader.rect``, ``shard``, ``checkpoint`` -- and keep their own policy: which sources they
take, what they raise, where K lives.
"""
import contextlib
import ctypes

import numpy as np

from pysnptools_amd import _native as N
from pysnptools_amd.util import get_num_threads

# source kinds
BED, PIECES, SNPGEN, SNPGEN_IIDS, DIST, DISTGEN, BGEN, PAIRS, DENSE, NONE = (
    "bed", "pieces", "snpgen", "snpgen_iids", "dist", "distgen", "bgen", "pairs", "dense", None)
SNPGEN_CHUNK_BYTES = 1 << 30  # packed SNPs generated in HBM per add_packed
DISTGEN_CHUNK_BYTES = 1 << 30  # distributions generated in HBM per add_dist
BGEN_CHUNK_BYTES = 1 << 30  # inflated BGEN blocks staged, and triples decoded from them in HBM, per launch
PAIRS_CHUNK_BYTES = 1 << 30  # pair values written in HBM per add_dense


def order_c(val):
    """The ABI's order flag of a contiguous array: 1 = C.  One row or one column is both C- and
    F-contiguous (the same memory either way) and passed as F."""
    return 1 if (val.flags["C_CONTIGUOUS"] and not val.flags["F_CONTIGUOUS"]) else 0


def require_float(dtype):
    if np.dtype(dtype) not in (np.float32, np.float64):
        raise ValueError("GRM dtype must be float32 or float64")


def source_kind(base, rows=None):
    """The one ladder over reader types: which kind of GRM source the innermost reader ``base``
    (``_resolve``), read at iids ``rows``, is.  DISTGEN / BGEN is ``as_snp()`` of a DistGen / Bgen read
    at every iid, DIST any other ``dist.as_snp()``: see ``Plan.src``."""
    from pysnptools_amd.distreader.bgen import bgen_range
    from pysnptools_amd.distreader.distgen import generated_range
    from pysnptools_amd.snpreader._dist2snp import _Dist2Snp
    from pysnptools_amd.snpreader.bed import Bed
    from pysnptools_amd.snpreader.snpgen import SnpGen

    from pysnptools_amd.snpreader.pairs import Pairs

    if _bed_pieces(base) is not None:
        return PIECES
    if isinstance(base, Pairs):
        return PAIRS  # (an iid subset of a Pairs takes the generic block loop, through its _read)
    if isinstance(base, _Dist2Snp):
        # (an iid subset of a DistGen or Bgen is a DIST without stored values: the generic block loop)
        if bgen_range(base.distreader) is not None:
            return BGEN
        return DISTGEN if generated_range(base.distreader) is not None else DIST
    if isinstance(base, SnpGen):
        return SNPGEN if rows is None else SNPGEN_IIDS  # iid subsets take the generic block loop
    if isinstance(base, Bed):
        return BED
    return DENSE if hasattr(base, "val") and base.val.ndim == 2 else NONE


def _bed_pieces(base):
    """The _MergeSIDs behind a DistributedBed / _MergeSIDs whose pieces are all Beds, else None."""
    from pysnptools_amd.snpreader._mergesids import _MergeSIDs
    from pysnptools_amd.snpreader.bed import Bed
    from pysnptools_amd.snpreader.distributedbed import DistributedBed

    if isinstance(base, DistributedBed):
        base._run_once()
        base = base._merge
    if isinstance(base, _MergeSIDs) and all(isinstance(r, Bed) for r in base.reader_list):
        base._run_once()
        return base
    return None


def trained_from(standardizer, kind, a, b, sid, stats):
    from pysnptools_amd import standardizer as stdizer

    if kind == N.STD_NONE:
        return stdizer.Identity()
    if isinstance(standardizer, (stdizer.UnitTrained, stdizer.BetaTrained)):
        return standardizer
    if kind == N.STD_UNIT:
        return stdizer.UnitTrained(sid, stats)
    return stdizer.BetaTrained(standardizer.a, standardizer.b, sid, stats)


class Plan(object):
    """What every fused route derives from (reader, standardizer, dtype): ``base, rows, cols``
    (``_resolve``), ``kind, a, b, use_stats`` (``std``: as the ABI takes them; ``args``: all of
    ``_std_args``), ``sid, n, m``, the dtype and its suffix, ``source`` (a source kind above) and
    ``src``: the _MergeSIDs of PIECES; the (array, col0, cols) of DIST (``_stored_range``), None when
    the distributions are not stored ones -- then no fused route applies; the (DistGen, SNP index
    array) of DISTGEN (``generated_range``); the (Bgen, variant index array) of BGEN (``bgen_range``)."""

    def __init__(self, reader, standardizer, dtype, args):
        from pysnptools_amd.snpreader.snpreader import _resolve

        self.standardizer, self.dtype, self.sfx, self.args = standardizer, dtype, N.suffix(dtype), args
        self.kind, self.a, self.b, self.use_stats = args[:4]
        self.std = (self.kind, self.a, self.b, int(self.use_stats))
        self.base, self.rows, self.cols = _resolve(reader)
        self.sid, self.n = reader.sid, reader.iid_count
        self.m = len(self.sid)
        self.source, self._index = source_kind(self.base, self.rows), {}

    @property
    def src(self):
        """Looked up on first use: ``_stored_range`` may load a file."""
        if "_src" not in self.__dict__:
            from pysnptools_amd.distreader.bgen import bgen_range
            from pysnptools_amd.distreader.distgen import generated_range
            from pysnptools_amd.snpreader._dist2snp import _stored_range

            self._src = (_bed_pieces(self.base) if self.source == PIECES else
                         _stored_range(self.base.distreader, self.dtype) if self.source == DIST else
                         generated_range(self.base.distreader) if self.source == DISTGEN else
                         bgen_range(self.base.distreader) if self.source == BGEN else None)
        return self._src

    def stats(self, zeros=False):
        """The [m, 2] per-SNP stats the adds read (trained standardizers) or fill; ``zeros``: for
        callers that sum them over ranks."""
        if self.use_stats:
            return np.ascontiguousarray(self.standardizer.stats_for(self.sid), dtype=self.dtype)
        return (np.zeros if zeros else np.empty)((self.m, 2), dtype=self.dtype)

    def trained(self, stats):
        return trained_from(self.standardizer, self.kind, self.a, self.b, self.sid, stats)

    def col_index(self, dtype=None):
        """The plan's SNPs as absolute column numbers of the source (built once per dtype)."""
        if dtype not in self._index:
            count = self.src.col_count if self.source == PIECES else self.base.sid_count
            self._index[dtype] = (np.arange(count, dtype=dtype) if self.cols is None
                                  else np.asarray(self.cols, dtype=dtype))
        return self._index[dtype]

    def threads(self, num_threads):
        """``num_threads``, else the Bed's own setting, else the default."""
        return get_num_threads(num_threads if num_threads is not None else self.base._num_threads)


def plan(reader, standardizer, dtype):
    """The Plan, or None when no fused route applies: another dtype than float32 / float64, or a
    standardizer ``_std_args`` does not know."""
    from pysnptools_amd.standardizer.standardizer import _std_args

    dtype = np.dtype(dtype)
    args = _std_args(standardizer) if dtype in (np.float32, np.float64) else None
    return None if args is None else Plan(reader, standardizer, dtype, args)


class Session(object):
    """The add calls of an open GRM session over ``n`` iids; ``rect`` = (ri, ci), the rectangle's
    iid index arrays (None = all), makes them the rect session's."""

    def __init__(self, n, dtype, rect=None):
        self.n, self.sfx, self.rect = int(n), N.suffix(dtype), rect
        self._add = "snpmi_grm_add_" if rect is None else "snpmi_grm_rect_add_"
        self._tail = () if rect is None else (N.ptr(rect[0]), N.ptr(rect[1]))

    def add_bed(self, bed, rows, cols, std, stats, threads, shape=None):
        """SNPs ``cols`` of iids ``rows`` (absolute; None = all) of the file of ``bed``, which holds
        ``shape`` = (iids, SNPs) (default: the Bed's own counts)."""
        n_iid, n_sid = map(int, shape if shape is not None else (bed.iid_count, bed.sid_count))
        ri, ci = N.index_array(rows), N.index_array(cols)
        N.call(self._add + "bed_" + self.sfx, bed.filename.encode(), n_iid, n_sid, int(bool(bed.count_A1)),
               N.ptr(ri), self.n, N.ptr(ci), n_sid if ci is None else len(ci), *std, N.ptr(stats), threads, *self._tail)

    def add_packed(self, packed, pitch, m, count_a1, std, stats):
        N.call(self._add + "packed_" + self.sfx, N.ptr(packed), pitch, self.n, m, int(bool(count_a1)), *std,
               N.ptr(stats), *self._tail)

    def add_dist(self, val, col0, cols, max_weight, std, stats):
        assert self.rect is None, "the rect session takes Bed and packed SNPs only"
        N.call("snpmi_grm_add_dist_" + self.sfx, N.ptr(val), self.n, int(val.shape[1]), col0, cols, order_c(val),
               float(max_weight), *std, N.ptr(stats))

    def add_dense(self, val):
        assert self.rect is None, "the rect session takes Bed and packed SNPs only"
        N.call("snpmi_grm_add_dense_" + self.sfx, N.ptr(val), val.shape[0], val.shape[1], order_c(val))


@contextlib.contextmanager
def session(n, dtype, K, diag_k_to_n=False, factor=None, rect=None, order="C"):
    """An open GRM session, ended on the way out, error or not.  Whole K (``snpmi_grm_begin`` /
    ``snpmi_grm_end``): K is n x n; ``factor`` (one f64) receives DiagKtoN's when ``diag_k_to_n``.
    ``rect`` = (ri, ci) (``snpmi_grm_rect_begin`` / ``snpmi_grm_rect_end``): K is the rectangle in
    ``order``, and is not written after a failed add."""
    if rect is None:
        N.call("snpmi_grm_begin", n, N.dt_code(dtype))
    else:
        N.call("snpmi_grm_rect_begin", int(K.shape[0]), int(K.shape[1]), N.dt_code(dtype))
    ok = False
    try:
        yield Session(n, dtype, rect)
        ok = True
    finally:
        if rect is None:
            fptr = None if factor is None else factor.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            N.call("snpmi_grm_end", int(bool(diag_k_to_n)), fptr, N.ptr(K))
        else:
            N.call("snpmi_grm_rect_end", 1.0, 1 if order == "C" else 0, N.ptr(K) if ok else None)


# ---------------------------------------------------------------------- feeders
def _add_with_stats(p, stats, here, add):
    """``add(the stats rows of SNPs here)``; computed stats are written back."""
    st = np.ascontiguousarray(stats[here])
    add(st)
    if not p.use_stats:
        stats[here] = st


def feed_bed(s, p, stats, threads, here=None):
    """The plan's Bed: every SNP in one add, or the SNPs ``here`` (a slice of the plan's)."""
    p.base._run_once()
    if here is None:
        s.add_bed(p.base, p.rows, p.cols, p.std, stats, threads)
    else:
        cols = np.ascontiguousarray(p.col_index(np.uint64)[here])
        _add_with_stats(p, stats, here, lambda st: s.add_bed(p.base, p.rows, cols, p.std, st, threads))


def feed_pieces(s, p, stats, num_threads, only=None):
    """One add_bed for every piece holding requested SNPs (``only``: piece subset)."""
    merged, threads = p.src, get_num_threads(num_threads)
    for k, here, rel in merged._pieces(p.col_index()):
        if only is None or k in only:
            _add_with_stats(p, stats, here, lambda st: s.add_bed(
                merged.reader_list[k], p.rows, rel, p.std, st, threads, (merged.row_count, merged.col_count_list[k])))


def feed_snpgen(s, p, stats, chunk_bytes=SNPGEN_CHUNK_BYTES):
    """An all-iid SnpGen: packed batches are generated in HBM and added chunk by chunk -- the
    values never exist as floats.  Chunks are whole batches when the SNPs are a contiguous range;
    otherwise a batch whose SNPs fall into two chunks is generated once for each."""
    col_index = p.col_index()
    pitch = int(N.lib().snpmi_packed_pitch(p.n))
    bs = int(p.base._block_size)
    step = max(bs, chunk_bytes // pitch // bs * bs)
    for c0 in range(0, len(col_index), step):
        here = slice(c0, min(c0 + step, len(col_index)))
        packed, _ = p.base._packed(col_index[here])
        _add_with_stats(p, stats, here, lambda st: s.add_packed(packed, pitch, here.stop - here.start, 0, p.std, st))


def feed_dist(s, p, stats, block_size):
    """``dist.as_snp()`` over stored distributions: each block of ``block_size`` SNPs is converted
    to expected values straight into the SYRK's operand buffer and standardized there -- the values
    never exist on the host.  Whole / blocked as the reference's loop (snpreader.py:629)."""
    val, col0, cols = p.src
    whole = block_size is None or cols <= block_size or cols <= p.n
    step = max(cols if whole else int(block_size), 1)
    for c0 in range(0, cols, step):
        here = slice(c0, min(c0 + step, cols))
        _add_with_stats(p, stats, here, lambda st: s.add_dist(val, col0 + c0, here.stop - here.start,
                                                              p.base.max_weight, p.std, st))


def feed_distgen(s, p, stats, chunk_bytes=DISTGEN_CHUNK_BYTES):
    """``as_snp()`` of an all-iid DistGen: the distributions are generated chunk by chunk into one
    reused HBM buffer (C order, the stream's own) and each chunk is converted straight into the
    SYRK's operand buffer -- the triples never exist on the host.  Chunks are whole batches when the
    SNPs are a contiguous range; otherwise a batch whose SNPs fall into two chunks is generated
    once for each."""
    from pysnptools_amd import hbm

    gen, cols = p.src
    bs = int(gen._block_size)
    step = max(bs, chunk_bytes // (3 * max(p.n, 1) * p.dtype.itemsize) // bs * bs)
    buf = hbm.empty((p.n, min(step, max(len(cols), 1)), 3), dtype=p.dtype, order="C")
    for c0 in range(0, len(cols), step):
        here = slice(c0, min(c0 + step, len(cols)))
        count = here.stop - here.start
        # the chunk's n x count x 3 triples, tight, at the start of the buffer
        val = buf if count == buf.shape[1] else hbm.HbmArray((p.n, count, 3), p.dtype, "C", _base=buf, _ptr=buf.ptr)
        gen._generate_into(val, cols[here])
        _add_with_stats(p, stats, here, lambda st: s.add_dist(val, 0, count, p.base.max_weight, p.std, st))


def feed_bgen(s, p, stats, chunk_bytes=None):
    """``as_snp()`` of an all-iid Bgen: the variants' blocks are inflated, staged and decoded chunk by
    chunk into one reused HBM triple buffer (F order: the decode's 16-byte store form) and each chunk
    is converted straight into the SYRK's operand buffer -- the triples never exist on the host.  A
    chunk is bounded by its staged blocks and by its triples (``BGEN_CHUNK_BYTES`` each)."""
    from pysnptools_amd import hbm

    bgen, cols = p.src
    chunks = list(bgen._chunks(cols, p.n, p.dtype.itemsize, chunk_bytes or BGEN_CHUNK_BYTES))
    widest = max([c.stop - c.start for c in chunks] + [1])
    buf = hbm.empty((p.n, widest, 3), dtype=p.dtype, order="F")
    for here in chunks:
        count = here.stop - here.start
        # the chunk's n x count x 3 triples, tight, at the start of the buffer
        val = buf if count == widest else hbm.HbmArray((p.n, count, 3), p.dtype, "F", _base=buf, _ptr=buf.ptr)
        bgen._decode_into(val, count, 0, cols[here])
        _add_with_stats(p, stats, here, lambda st: s.add_dist(val, 0, count, p.base.max_weight, p.std, st))


def feed_pairs(s, p, stats, chunk_bytes=None):
    """An all-iid ``Pairs`` (any pair subset): chunks of at most ``PAIRS_CHUNK_BYTES`` of pair values
    are written in HBM from the resident packed inner SNPs (``snpmi_dev_pair_values``), standardized
    there by the plan's standardizer (the device-side dense standardize) and added -- the N x P values
    never exist on the host."""
    pairs, cols = p.base, p.col_index(np.int64)
    pairs._resident(p.dtype)  # every chunk reads the same inner SNPs: loaded once
    is_beta, st_fn = int(p.kind == N.STD_BETA), "snpmi_standardize_" + p.sfx
    step = max(1, (chunk_bytes or PAIRS_CHUNK_BYTES) // (max(p.n, 1) * p.dtype.itemsize))
    for c0 in range(0, len(cols), step):
        here = slice(c0, min(c0 + step, len(cols)))
        val = pairs._values(None, cols[here], "F", p.dtype, to_hbm=True)

        def add(st):
            if p.kind != N.STD_NONE:
                N.call(st_fn, N.ptr(val), val.shape[0], val.shape[1], 0, is_beta, float(p.a), float(p.b), 1,
                       int(p.use_stats), N.ptr(st), get_num_threads(None))
            s.add_dense(val)

        _add_with_stats(p, stats, here, add)


# ---------------------------------------------------------------------- packed SNPs in HBM
def at(a, offset):
    """Device address ``offset`` bytes into an HbmArray."""
    return ctypes.c_void_p(a.ptr + int(offset))


def packed_chunks(p, dtype, stats, chunk_bytes, multiple=1, num_threads=None):
    """The plan's SNPs (a Bed or SnpGen source) as packed codes in HBM, chunk by chunk: (first SNP,
    count, packed codes, pitch, value table) in SNP order.  Per chunk: the source's packed SNPs (the
    .bed gather and upload, or the generator), the iid repack of a subset, and the stats / value table
    of the chunk on the selected iids (``snpmi_dev_snp_stats`` with the plan's standardizer).  A chunk
    holds at most ``chunk_bytes`` of source codes and a multiple of ``multiple`` SNPs.  ``stats``
    ([m, 2] of dtype) is read when the plan's standardizer is trained, else filled on the way."""
    from pysnptools_amd import hbm

    dtype = np.dtype(dtype)
    n, m = int(p.n), int(p.m)
    base, rows = p.base, p.rows
    n_src = int(base.iid_count)
    pitch = int(N.lib().snpmi_packed_pitch(n))
    pitch_src = int(N.lib().snpmi_packed_pitch(n_src))
    col_index = p.col_index(np.uint64)
    is_bed = p.source == BED
    if is_bed:
        base._run_once()
    count_a1 = int(bool(base.count_A1)) if is_bed else 0
    idx = None if rows is None else hbm.asarray(N.index_array(rows))
    step = max(multiple, chunk_bytes // pitch_src // multiple * multiple)
    dt = N.dt_code(dtype)
    for s0 in range(0, m, step):
        here = slice(s0, min(s0 + step, m))
        cnt = here.stop - here.start
        cols = np.ascontiguousarray(col_index[here])
        if is_bed:
            host = np.empty((cnt, pitch_src), dtype=np.uint8)
            N.call("snpmi_bed_gather_packed", base.filename.encode(), n_src, int(base.sid_count), N.ptr(cols), cnt,
                   pitch_src, N.ptr(host), p.threads(num_threads))
            packed = hbm.asarray(host)
        else:
            packed, _ = base._packed(cols)
        if idx is not None:
            sub = hbm.empty((cnt, pitch), dtype=np.uint8)
            N.call("snpmi_dev_repack", N.ptr(packed), pitch_src, n_src, N.ptr(idx), n, cnt, N.ptr(sub), pitch)
            packed = sub
        lut = hbm.empty((cnt, 4), dtype=dtype)
        st = (hbm.asarray(np.ascontiguousarray(stats[here])) if p.use_stats
              else hbm.empty((cnt, 2), dtype=dtype))
        N.call("snpmi_dev_snp_stats", N.ptr(packed), pitch, n, cnt, count_a1, *p.std, dt, N.ptr(st), N.ptr(lut))
        if not p.use_stats:
            stats[here] = st.get()
        yield s0, cnt, packed, pitch, lut


def load_packed(p, dtype, stats, chunk_bytes, multiple=1, num_threads=None):
    """All of ``packed_chunks`` resident in HBM: (packed codes [m][pitch], pitch, value table [m][4])."""
    from pysnptools_amd import hbm

    dtype = np.dtype(dtype)
    n, m = int(p.n), int(p.m)
    pitch = int(N.lib().snpmi_packed_pitch(n))
    packed = hbm.empty((max(m, 1), pitch), dtype=np.uint8)
    lut = hbm.empty((max(m, 1), 4), dtype=dtype)
    for s0, cnt, pk, _, lt in packed_chunks(p, dtype, stats, chunk_bytes, multiple, num_threads):
        N.call("snpmi_dev_memcpy_d2d", at(packed, s0 * pitch), N.ptr(pk), cnt * pitch)
        N.call("snpmi_dev_memcpy_d2d", at(lut, s0 * 4 * dtype.itemsize), N.ptr(lt), cnt * 4 * dtype.itemsize)
        N.call("snpmi_stream_sync")  # the chunk's buffers are released on the way round
    return packed, pitch, lut
