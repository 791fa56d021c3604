"""Bgen: BGEN files decoded into genotype distributions on the GPU (reference distreader/bgen.py).

The reference reads through the ``bgen_reader`` / ``cbgen`` C library.  Here the variant index is
walked by ``snpmi_bgen_open`` / ``snpmi_bgen_index`` (csrc/bgen.hip, host side), the genotype blocks
are inflated by Python's ``zlib`` on a thread pool, checked, packed into one page-locked buffer and
uploaded, and ``snpmi_dev_bgen_decode_*`` unpacks the B-bit integers into the iid x sid x 3 array in
HBM, in the requested dtype and order; ``as_snp()`` and its GRM read the triples there.  Nothing is
written next to the input: there is no metadata cache file.  With ``inflate='device'`` the stored
bytes are uploaded as they are and ``snpmi_dev_inflate`` / ``snpmi_dev_bgen_check`` inflate and check
them in HBM; the host then only reads the file and the small check records.

Supported: layout 2, compression none or zlib, every variant read biallelic, unphased and diploid,
1 ... 32 bits.  Anything else raises ``ValueError`` naming what and where; every variant of a read
is checked on the host before its launch (the allele counts of all of them before the first).

``Bgen.write`` writes such files from any DistReader with NumPy alone (the reference shells out to
QCTool).
"""
import ctypes
import os
import struct
import threading
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from pysnptools_amd import _native as N
from pysnptools_amd.distreader.distreader import DistReader
from pysnptools_amd.util import get_num_threads


def default_iid_function(sample):
    """
    The default function for turning a Bgen sample into a two-part iid: split on a single comma,
    else ('0', sample).

    >>> default_iid_function('fam0,ind0')
    ('fam0', 'ind0')
    >>> default_iid_function('ind0')
    ('0', 'ind0')
    """
    fields = sample.split(",")
    if len(fields) == 2:
        return fields[0], fields[1]
    return ("0", sample)


def default_sid_function(id, rsid):
    """
    The default function for turning a Bgen (SNP) id and rsid into a sid: the id when the rsid is
    '' or '0', else 'ID,RSID'.

    >>> default_sid_function('SNP1','rs102343')
    'SNP1,rs102343'
    >>> default_sid_function('SNP1','0')
    'SNP1'
    """
    if rsid == "0" or rsid == "":
        return id
    return id + "," + rsid


def default_sample_function(famid, indid):
    """
    The default function for turning a two-part iid into a Bgen sample: the second part when the
    family id is '0' or '', else 'FAMID,INDID'.

    >>> default_sample_function('fam0','ind0')
    'fam0,ind0'
    >>> default_sample_function('0','ind0')
    'ind0'
    """
    if famid == "0" or famid == "":
        return indid
    return famid + "," + indid


def default_id_rsid_function(sid):
    """
    The default function for turning a sid into a Bgen (SNP) id and rsid: split on a single comma,
    else (sid, '0').

    >>> default_id_rsid_function('SNP1,rs102343')
    ('SNP1', 'rs102343')
    >>> default_id_rsid_function('SNP1')
    ('SNP1', '0')
    """
    fields = sid.split(",")
    if len(fields) == 2:
        return fields[0], fields[1]
    return sid, "0"


# the status words of snpmi_dev_inflate (csrc/inflate_core.hpp), as the reason of "does not inflate"
INFLATE_STATUS = {1: "bad zlib header", 2: "the stream is truncated", 3: "reserved block type",
                  4: "stored block length check failed", 5: "bad code-length set",
                  6: "invalid length or distance symbol", 7: "distance beyond the start of the output",
                  8: "more bytes than the header's length", 9: "fewer bytes than the header's length",
                  10: "Adler-32 mismatch"}
INFLATE_STATUS_OVERFLOW, INFLATE_STATUS_SHORT = 8, 9


def _round8(x):
    return (x + 7) // 8 * 8


def _strings(raw):
    """'S<width>' rows -> a fresh str array."""
    return np.char.decode(raw, "utf-8") if len(raw) else np.empty(0, dtype="U1")


class _Staging(object):
    """One page-locked host buffer and one HBM buffer of the same size (grow-only)."""

    def __init__(self):
        self.size, self.host, self.view, self.dev = 0, None, None, None

    def reserve(self, nbytes):
        from pysnptools_amd import hbm

        if nbytes <= self.size:
            return
        self.release()
        p = ctypes.c_void_p()
        N.call("snpmi_host_alloc", ctypes.byref(p), nbytes)
        self.host, self.size = p, nbytes
        self.view = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p.value))
        self.dev = hbm.empty((nbytes,), dtype=np.uint8)

    def release(self):
        self.view, self.dev = None, None
        if self.host is not None:
            try:
                N.call("snpmi_host_free", self.host)
            except Exception:
                pass
        self.host, self.size = None, 0


class Bgen(DistReader):
    """A :class:`DistReader` of a \\*.bgen file.

    :param filename: the BGEN file
    :param iid_function: turns a BGEN sample into an iid (default :func:`default_iid_function`)
    :param sid_function: turns a BGEN (SNP) id and rsid into a sid (default
        :func:`default_sid_function`), or the string 'id' or 'rsid'
    :param sample: optional GEN ``.sample`` file; overrides the samples in the \\*.bgen file
    :param num_threads: threads that inflate the genotype blocks (default: ``get_num_threads``)
    :param fresh_properties: accepted; iid, sid and pos are always fresh arrays
    :param inflate: where the zlib genotype blocks are inflated: 'host' (default: Python's ``zlib`` on
        the thread pool) or 'device' (the stored bytes are uploaded and inflated in HBM,
        ``snpmi_dev_inflate``, and checked there); the values read are the same

    >>> from pysnptools_amd.distreader import Bgen
    >>> data_on_disk = Bgen("tests/golden/data/example.bgen")
    >>> print((data_on_disk.iid_count, data_on_disk.sid_count))
    (500, 199)
    """

    def __init__(self, filename, iid_function=default_iid_function, sid_function=default_sid_function, sample=None,
                 num_threads=None, fresh_properties=True, inflate="host"):
        super(Bgen, self).__init__()
        if not isinstance(inflate, str) or inflate not in ("host", "device"):
            raise ValueError("inflate must be 'host' or 'device', not {0!r}".format(inflate))
        self._inflate_on = inflate
        self._inflated = None  # inflate='device': the HBM buffer the blocks are inflated into (grow-only)
        self._ran_once = False
        self.filename = filename
        self._iid_function = iid_function
        self._sid_function = sid_function
        self._sample = sample
        self._num_threads = num_threads
        self._fresh_properties = fresh_properties
        self._fd = None
        self._staging = None
        self._staging_lock = threading.Lock()  # one staging buffer per reader: one decode at a time

    def __repr__(self):
        return "{0}('{1}')".format(self.__class__.__name__, self.filename)

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

    def copyinputs(self, copier):
        # (only the original inputs: needs no _run_once)
        copier.input(self.filename)
        if self._sample is not None:
            copier.input(self._sample)

    def __del__(self):
        self.flush()

    def flush(self):
        """Close the \\*.bgen file (it is reopened when values or properties are used again)."""
        if getattr(self, "_ran_once", False):
            self._ran_once = False
            if self._fd is not None:
                os.close(self._fd)
                self._fd = None
            with self._staging_lock:
                if self._staging is not None:
                    self._staging.release()
                    self._staging = None
                self._inflated = None

    # ------------------------------------------------------------------ the index
    def _run_once(self):
        if self._ran_once:
            return
        assert os.path.exists(self.filename), "Expect file to exist ('{0}')".format(self.filename)
        path = os.fsencode(self.filename)
        info = (ctypes.c_uint64 * 11)()
        N.call("snpmi_bgen_open", path, info)
        m, n, flags, _, has_samples = (int(x) for x in info[:5])
        widths = [int(x) for x in info[5:10]]
        rec = np.zeros((m, 5), dtype=np.uint64)
        raw = [np.zeros(count, dtype="S{0}".format(max(w, 1))) for count, w in zip((n, m, m, m, m), widths)]
        args = []
        for a, w in zip(raw, widths):
            args += [N.ptr(a), w]
        N.call("snpmi_bgen_index", path, m, n, N.ptr(rec), *args)
        self._rec, self._flags, self._n = rec.astype(np.int64), flags, n
        self._ids, self._rsids, chroms = _strings(raw[1]), _strings(raw[2]), _strings(raw[3])
        self._chroms = chroms
        self._alleles = _strings(raw[4])

        if self._sample is not None:
            with open(self._sample) as f:
                lines = [line.split() for line in f.read().splitlines()[2:]]
            samples = np.array([fields[0] for fields in lines if fields], dtype="str")
            if len(samples) != n:
                raise ValueError("'{0}' lists {1} samples, '{2}' holds {3}".format(self._sample, len(samples),
                                                                                  self.filename, n))
        elif has_samples:
            samples = _strings(raw[0])
        else:
            samples = np.array(["sample_{0}".format(i) for i in range(n)], dtype="str")
        self._samples = samples
        if self._iid_function is default_iid_function and not np.any(np.char.count(samples, ",") == 1):
            row = np.empty((n, 2), dtype="<U{0}".format(max(samples.dtype.itemsize // 4, 1)))
            row[:, 0], row[:, 1] = "0", samples
        else:
            row = np.array([self._iid_function(s) for s in samples], dtype="str").reshape(-1, 2)
        self._row = row
        self._col = self._apply_sid_function(self._ids, self._rsids)

        pos = np.zeros((m, 3))
        pos[:, 2] = self._rec[:, 3]
        try:
            pos[:, 0] = chroms.astype(np.int64) if m else 0  # ("01" -> 1)
        except ValueError:
            for i, text in enumerate(chroms):
                try:
                    pos[i, 0] = int(text)
                except ValueError:
                    pos[i, 0] = 0
        self._col_property = pos
        self._assert_iid_sid_pos(check_val=False)
        self._fd = os.open(self.filename, os.O_RDONLY)
        self._ran_once = True

    def _apply_sid_function(self, ids, rsids):
        if isinstance(self._sid_function, str):
            if self._sid_function == "id":
                return ids.copy()
            if self._sid_function == "rsid":
                return rsids.copy()
            raise ValueError("sid_function must be a function, 'id' or 'rsid'")
        if self._sid_function is default_sid_function:
            # the reference's file-wide rule (bgen.py:281-302)
            if np.all(rsids == "0") or np.all(rsids == ""):
                return ids.copy()
            return np.char.add(np.char.add(ids, ","), rsids)
        return np.array([self._sid_function(i, r) for i, r in zip(ids, rsids)], dtype="str").reshape(-1)

    # ------------------------------------------------------------------ blocks -> HBM
    def _check(self, sid_index):
        """What the index alone tells about the variants ``sid_index``, before anything is inflated."""
        self._run_once()
        idx = np.asarray(sid_index, dtype=np.int64)
        bad = idx[self._rec[idx, 4] != 2] if len(idx) else idx
        if len(bad):
            v = int(bad[0])
            raise ValueError("variant {0} ('{1}') of '{2}' has {3} alleles ({4}); only biallelic variants are supported"
                             .format(v, self._ids[v], self.filename, int(self._rec[v, 4]), self._alleles[v]))

    def _inflate(self, v):
        """The checked, inflated genotype block of variant ``v`` and its bit depth."""
        at, stored, inflated = (int(x) for x in self._rec[v, :3])
        where = "variant {0} ('{1}') of '{2}'".format(v, self._ids[v], self.filename)
        data = os.pread(self._fd, stored, at)
        if len(data) != stored:
            raise ValueError("BGEN file is truncated: the genotype block of {0} at offset {1}".format(where, at))
        if self._flags & 3:
            try:
                data = zlib.decompress(data)
            except zlib.error as e:
                raise ValueError("the genotype block of {0} does not inflate: {1}".format(where, e))
        n = self._n
        if len(data) != inflated:
            raise ValueError("the genotype block of {0} inflates to {1} bytes, its header says {2}"
                             .format(where, len(data), inflated))
        if len(data) < 10 + n:
            self._check_block(where, len(data), None)
        n_here, k, pmin, pmax = struct.unpack_from("<IHBB", data, 0)
        ploidy = np.frombuffer(data, dtype=np.uint8, count=n, offset=8) & 0x3F
        bits = data[9 + n]
        self._check_block(where, len(data), (n_here, k, pmin, pmax, int(ploidy.min()) if n else pmin,
                                             int(ploidy.max()) if n else pmax, data[8 + n], bits))
        return data, bits

    def _check_block(self, where, length, fields):
        """Refuse an inflated block of ``length`` bytes that this reader cannot decode.  ``fields``:
        its N, K, header ploidy min and max, the samples' ploidy min and max, the phased byte and the
        bit depth, or None when it is too short to hold them."""
        n = self._n
        if fields is None:
            raise ValueError("the genotype block of {0} holds {1} bytes, too few for {2} samples"
                             .format(where, length, n))
        n_here, k, pmin, pmax, lo, hi, phased, bits = fields
        if n_here != n:
            raise ValueError("{0} holds {1} samples, the header {2}".format(where, n_here, n))
        if k != 2:
            raise ValueError("{0} has {1} alleles; only biallelic variants are supported".format(where, k))
        if pmin != 2 or pmax != 2 or lo != 2 or hi != 2:
            raise ValueError("{0} is not diploid throughout (ploidy {1} ... {2}); only ploidy 2 is supported"
                             .format(where, min(pmin, lo), max(pmax, hi)))
        if phased != 0:
            raise ValueError("{0} is phased; only unphased data is supported".format(where))
        if not 1 <= bits <= 32:
            raise ValueError("{0} stores {1} bits per probability; 1 ... 32 are supported".format(where, bits))
        want = 10 + n + (2 * bits * n + 7) // 8
        if length != want:
            raise ValueError("the genotype block of {0} holds {1} bytes, {2} samples at {3} bits need {4}"
                             .format(where, length, n, bits, want))

    def _chunks(self, sid_index, rows, itemsize, chunk_bytes):
        """Slices of ``sid_index`` whose blocks (each counted once per column) and whose triples both
        stay within ``chunk_bytes``; at least one column each."""
        cost = np.cumsum(_round8(self._rec[sid_index, 2])) if len(sid_index) else np.zeros(0, dtype=np.int64)
        per_out = max(chunk_bytes // max(3 * rows * itemsize, 1), 1)
        start, m = 0, len(sid_index)
        while start < m:
            base = int(cost[start - 1]) if start else 0
            stop = int(np.searchsorted(cost, base + chunk_bytes - 16, side="right"))
            stop = max(start + 1, min(stop, start + per_out, m))
            yield slice(start, stop)
            start = stop

    def _decode_into(self, out, cols_total, col0, sid_index, rows=None, num_threads=None):
        """Variants ``sid_index`` into the SNPs [col0, col0 + len(sid_index)) of the HbmArray ``out``
        (rows x cols_total x 3, tight); ``rows``: iid index array, None = every iid in order."""
        self._run_once()
        sid_index = np.asarray(sid_index, dtype=np.int64)
        n_rows = self._n if rows is None else len(rows)
        if len(sid_index) == 0 or n_rows == 0:
            return out
        with self._staging_lock:  # concurrent reads of one Bgen take turns at its staging buffer
            return self._decode_staged(out, cols_total, col0, sid_index, rows, n_rows, num_threads)

    def _decode_staged(self, out, cols_total, col0, sid_index, rows, n_rows, num_threads):
        uniq, inverse = np.unique(sid_index, return_inverse=True)
        lengths = self._rec[uniq, 2]
        offsets = np.concatenate(([0], np.cumsum(_round8(lengths))))
        total = int(offsets[-1]) + 16  # the kernel's two-word windows end inside the spare bytes
        if self._staging is None:
            self._staging = _Staging()
        threads = min(get_num_threads(self._num_threads if num_threads is None else num_threads), 64, len(uniq))
        if self._inflate_on == "device" and self._flags & 3:
            blocks, bits = self._stage_inflated(uniq, offsets, total, threads)
        else:
            blocks, bits = self._stage_on_host(uniq, offsets, total, threads)
        table = np.empty((len(sid_index), 3), dtype=np.uint64)
        table[:, 0], table[:, 1], table[:, 2] = offsets[:-1][inverse], bits[inverse], self._n
        idx = None if rows is None else N.index_array(rows)
        N.call("snpmi_dev_bgen_decode_" + N.suffix(out.dtype), N.ptr(blocks), total, N.ptr(table),
               len(sid_index), N.ptr(idx), n_rows, N.ptr(out), int(cols_total), int(col0),
               1 if out.order == "C" else 0)
        return out

    @staticmethod
    def _map(threads, fn, count):
        if threads > 1 and count > 1:
            with ThreadPoolExecutor(max_workers=threads) as pool:
                return list(pool.map(fn, range(count)))
        return [fn(k) for k in range(count)]

    def _stage_on_host(self, uniq, offsets, total, threads):
        """inflate='host': the variants ``uniq`` inflated and checked on the thread pool, packed at
        ``offsets`` of the page-locked buffer and uploaded.  Returns (HBM buffer, bit depths)."""
        self._staging.reserve(total)
        view = self._staging.view

        def one(k):
            data, bits = self._inflate(int(uniq[k]))
            view[offsets[k]:offsets[k] + len(data)] = np.frombuffer(data, dtype=np.uint8)
            return bits

        bits = np.fromiter(self._map(threads, one, len(uniq)), dtype=np.uint64, count=len(uniq))
        view[total - 16:total] = 0
        N.call("snpmi_memcpy_h2d", N.ptr(self._staging.dev), self._staging.host, total)
        return self._staging.dev, bits

    def _stage_inflated(self, uniq, offsets, total, threads):
        """inflate='device': the stored bytes of the variants ``uniq`` read into the page-locked
        buffer back to back, uploaded, inflated at ``offsets`` of a second HBM buffer (one wave per
        block) and checked there.  Returns (that buffer, bit depths)."""
        from pysnptools_amd import hbm

        at, stored, lengths = self._rec[uniq, 0], self._rec[uniq, 1], self._rec[uniq, 2]
        src = np.concatenate(([0], np.cumsum(stored)))
        src_total = int(src[-1])
        self._staging.reserve(max(src_total, 1))
        view = self._staging.view

        def one(k):
            a, b = int(src[k]), int(src[k + 1])
            if b > a and os.preadv(self._fd, [view[a:b]], int(at[k])) != b - a:
                raise ValueError("BGEN file is truncated: the genotype block of {0} at offset {1}"
                                 .format(self._where(int(uniq[k])), int(at[k])))

        self._map(threads, one, len(uniq))
        if self._inflated is None or self._inflated.nbytes < total:
            self._inflated = None
            self._inflated = hbm.empty((total,), dtype=np.uint8)
        blocks = self._inflated
        N.call("snpmi_dev_memset", ctypes.c_void_p(blocks.ptr + total - 16), 0, 16)  # the decode's spare bytes
        if src_total:
            N.call("snpmi_memcpy_h2d", N.ptr(self._staging.dev), self._staging.host, src_total)
        N.call("snpmi_stream_sync")
        table = np.empty((len(uniq), 4), dtype=np.uint64)
        table[:, 0], table[:, 1], table[:, 2], table[:, 3] = src[:-1], stored, offsets[:-1], lengths
        status = np.zeros(len(uniq), dtype=np.uint32)
        N.call("snpmi_dev_inflate", N.ptr(self._staging.dev), max(src_total, 1), N.ptr(blocks), total, N.ptr(table),
               len(uniq), N.ptr(status))
        rec = np.zeros((len(uniq), 10), dtype=np.uint64)
        where = np.ascontiguousarray(table[:, 2:])  # (offset, length) of each inflated block
        N.call("snpmi_dev_bgen_check", N.ptr(blocks), total, N.ptr(where), len(uniq), self._n, N.ptr(rec))
        bad = np.flatnonzero((status != 0) | (rec[:, 0] != 0) | (rec[:, 1] < 1) | (rec[:, 1] > 32)
                             | (rec[:, 9] != lengths.astype(np.uint64))
                             | np.any(rec[:, 2:9] != np.array([self._n, 2, 2, 2, 2, 2, 0], dtype=np.uint64), axis=1))
        if len(bad):  # the first variant in file order that the host route would have refused
            k = int(bad[0])
            self._refuse(int(uniq[k]), int(status[k]), bytes(view[int(src[k]):int(src[k + 1])]), int(lengths[k]),
                         [int(x) for x in rec[k]])
        return blocks, rec[:, 1].copy()

    def _where(self, v):
        return "variant {0} ('{1}') of '{2}'".format(v, self._ids[v], self.filename)

    def _refuse(self, v, status, stored, inflated, rec):
        """Raise for variant ``v``, whose device inflate ended with ``status`` or whose check record
        ``rec`` does not pass, in the words of ``_inflate``."""
        where = self._where(v)
        if status in (INFLATE_STATUS_OVERFLOW, INFLATE_STATUS_SHORT):
            # the stream disagrees with the header's length: inflate this one block here to name its own
            try:
                length = len(zlib.decompress(stored))
            except zlib.error as e:
                raise ValueError("the genotype block of {0} does not inflate: {1}".format(where, e))
            raise ValueError("the genotype block of {0} inflates to {1} bytes, its header says {2}"
                             .format(where, length, inflated))
        if status:
            raise ValueError("the genotype block of {0} does not inflate: {1}"
                             .format(where, INFLATE_STATUS.get(status, "status {0}".format(status))))
        self._check_block(where, inflated, None if rec[0] else (rec[2], rec[3], rec[4], rec[5],
                                                                 rec[6] if self._n else rec[4],
                                                                 rec[7] if self._n else rec[5], rec[8], rec[1]))
        raise AssertionError("the check record of {0} passes".format(where))

    def _generate_into(self, out, sid_index, rows=None, num_threads=None, chunk_bytes=None):
        """``_decode_into`` of all of ``out`` in chunks of bounded staging."""
        from pysnptools_amd import _grm

        n_rows = self._n if rows is None else len(rows)
        assert tuple(out.shape) == (n_rows, len(sid_index), 3)
        self._check(sid_index)
        for here in self._chunks(sid_index, n_rows, out.dtype.itemsize, chunk_bytes or _grm.BGEN_CHUNK_BYTES):
            self._decode_into(out, len(sid_index), here.start, sid_index[here], rows, num_threads)
        return out

    def _generate(self, sid_index, order, dtype):
        """A new HbmArray of the distributions of variants ``sid_index``, all iids."""
        from pysnptools_amd import hbm

        self._check(sid_index)  # before anything is allocated
        return self._generate_into(hbm.empty((self._n, len(sid_index), 3), dtype=dtype, order=order),
                                   np.asarray(sid_index, dtype=np.int64))

    def _read(self, iid_index_or_none, sid_index_or_none, order, dtype, force_python_only, view_ok, num_threads):
        from pysnptools_amd import hbm
        from pysnptools_amd.util import _on_device

        self._run_once()
        dtype = np.dtype(dtype)
        if order == "A":
            order = "F"
        if dtype not in (np.float32, np.float64):
            raise ValueError("dtype '{0}' not supported; use float32 or float64".format(dtype))
        cols = (np.arange(self.sid_count) if sid_index_or_none is None
                else np.asarray(sid_index_or_none, dtype=np.int64).reshape(-1))
        rows = None if iid_index_or_none is None else np.asarray(iid_index_or_none, dtype=np.int64).reshape(-1)
        to_hbm = _on_device()
        shape = (self._n if rows is None else len(rows), len(cols), 3)
        if 0 in shape:
            return (hbm.empty if to_hbm else np.empty)(shape, dtype=dtype, order=order)
        val = self._generate_into(hbm.empty(shape, dtype=dtype, order=order), cols, rows, num_threads)
        return val if to_hbm else val.get()

    # ------------------------------------------------------------------ writing
    @staticmethod
    def write(filename, distreader, bits=16, compression=None, sample_function=default_sample_function,
              id_rsid_function=default_id_rsid_function, iid_function=default_iid_function,
              sid_function=default_sid_function, block_size=None, qctool_path=None, cleanup_temp_files=True):
        """Write a :class:`DistReader` as a layout-2 BGEN file with a sample block, on the host, and
        return its :class:`Bgen` (the reference's ``write`` needs QCTool; ``qctool_path`` and
        ``cleanup_temp_files`` are accepted and ignored).

        :param bits: 1 ... 32 bits per probability
        :param compression: None or 'zlib'
        :param block_size: SNPs read from *distreader* at a time (default: about 100,000 values)

        A triple with a NaN, or summing to 0, is written as missing; a negative value, or a sum
        further than 1e-6 from 1, raises.  With D = 2**bits - 1 the triple p becomes the integers
        floor(p * D), and the D - sum of them components with the largest fractional parts (ties
        to the lower index) get one more; the first two are stored.  For a triple that sums to 1
        within float64 rounding that makes the three integers sum to D.  A sum up to 1e-6 off
        leaves them up to 1e-6 * D apart from D (thousands of units at 32 bits); the third value
        is not stored, so the file then reads back as (a, b, D - a - b) / D, each within one unit
        of p * D in the first two.
        """
        bits = int(bits)
        if not 1 <= bits <= 32:
            raise ValueError("bits must be between 1 and 32")
        if compression not in (None, "zlib"):
            raise ValueError("compression '{0}' is not supported; use None or 'zlib'".format(compression))
        n, m = distreader.iid_count, distreader.sid_count
        block_size = block_size or max((100 * 1000) // max(1, n), 1)
        flags = (1 if compression == "zlib" else 0) | (2 << 2) | (1 << 31)
        samples = [sample_function(f, i).encode("utf-8") for f, i in distreader.iid]
        sample_block = struct.pack("<I", n) + b"".join(struct.pack("<H", len(s)) + s for s in samples)
        sample_block = struct.pack("<I", len(sample_block) + 4) + sample_block
        header = struct.pack("<III4sI", 20, m, n, b"bgen", flags)
        D = float(2 ** bits - 1)
        with open(filename, "wb") as f:
            f.write(struct.pack("<I", len(header) + len(sample_block)) + header + sample_block)
            for start in range(0, m, block_size):
                val, sid, pos = _host_block(distreader, start, start + block_size)
                for j in range(len(sid)):
                    p = val[:, j, :]
                    total = p.sum(axis=1)
                    missing = np.isnan(total) | (total == 0)
                    ok = ~missing
                    if np.any(p[ok] < 0) or np.any(np.abs(total[ok] - 1) > 1e-6):
                        raise ValueError("the distributions of sid '{0}' are negative or do not sum to 1 (+/- 1e-6)"
                                         .format(sid[j]))
                    v = np.where(ok[:, None], p, 0.0) * D
                    x = np.floor(v)
                    short = (D - x.sum(axis=1)).astype(np.int64)  # 0, 1 or 2 when p sums to 1; any sign and size within 1e-6 D otherwise
                    # rank of each component by descending fractional part, ties to the lower index
                    f0, f1, f2 = (v - x).T
                    rank = np.stack([(f1 > f0).astype(np.int64) + (f2 > f0), (f0 >= f1).astype(np.int64) + (f2 > f1),
                                     (f0 >= f2).astype(np.int64) + (f1 >= f2)], axis=1)
                    x += rank < short[:, None]
                    x[missing] = 0
                    ab = np.clip(x[:, :2], 0, D).astype(np.uint64)
                    flag = np.where(missing, 0x82, 0x02).astype(np.uint8)  # ploidy 2, bit 7: missing
                    block = (struct.pack("<IHBB", n, 2, 2, 2) + flag.tobytes() + struct.pack("<BB", 0, bits)
                             + _pack_bits(ab.reshape(-1), bits))
                    ident, rsid = id_rsid_function(str(sid[j]))
                    assert ident.strip() != "", "id cannot be whitespace"
                    assert rsid.strip() != "", "rsid cannot be whitespace"
                    chrom = pos[j, 0]
                    chrom = str(int(chrom)) if chrom == chrom else "0"
                    position = pos[j, 2]
                    f.write(b"".join(struct.pack("<H", len(s)) + s
                                     for s in (ident.encode("utf-8"), rsid.encode("utf-8"), chrom.encode("utf-8"))))
                    f.write(struct.pack("<IH", int(position) if position == position else 0, 2))
                    f.write(struct.pack("<I", 1) + b"A" + struct.pack("<I", 1) + b"G")
                    if compression == "zlib":
                        packed = zlib.compress(block)
                        f.write(struct.pack("<II", len(packed) + 4, len(block)) + packed)
                    else:
                        f.write(struct.pack("<I", len(block)) + block)
        return Bgen(filename, iid_function=iid_function, sid_function=sid_function)


def _host_block(distreader, start, stop):
    """(float64 values, sid, pos) of the SNPs [start, stop) on the host: a slice of in-memory host
    values, else a read of the subset."""
    from pysnptools_amd.util import asnumpy

    val = getattr(distreader, "val", None)
    if isinstance(val, np.ndarray):
        return (np.asarray(val[:, start:stop, :], dtype=np.float64), distreader.sid[start:stop],
                distreader.pos[start:stop])
    data = distreader[:, start:stop].read(order="F", dtype=np.float64, view_ok=True)
    return asnumpy(data.val), data.sid, data.pos


def _pack_bits(values, bits):
    """``values`` (uint64, each below 2**bits) as consecutive little-endian ``bits``-bit fields."""
    if bits in (8, 16, 32):  # whole bytes: the fields are the little-endian integers themselves
        return values.astype("<u{0}".format(bits // 8)).tobytes()
    shifts = np.arange(bits, dtype=np.uint64)
    return np.packbits(((values[:, None] >> shifts) & np.uint64(1)).astype(np.uint8).reshape(-1),
                       bitorder="little").tobytes()


def bgen_range(distreader):
    """(Bgen, absolute variant index array) when ``distreader`` is a Bgen, or a subset of one with
    every iid in order and any SNP selection; else None."""
    from pysnptools_amd.snpreader.snpreader import _resolve

    base, rows, cols = _resolve(distreader)
    if not isinstance(base, Bgen):
        return None
    if rows is not None and not np.array_equal(rows, np.arange(base.iid_count)):
        return None
    return base, (np.arange(base.sid_count) if cols is None else np.asarray(cols, dtype=np.int64))
