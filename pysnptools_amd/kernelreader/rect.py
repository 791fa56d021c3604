"""K[rows, cols] of a SnpKernel computed directly (the rect GRM session, include/snpmi.h
``snpmi_grm_rect_*``), without the whole N x N K the reference builds and slices
(kernelreader/snpkernel.py:84-88).

``set_grm_rect`` / ``PST_GRM_RECT`` choose when ``SnpKernel._read`` takes this path; the decision
itself (``use_rect``) is a pure function of sizes and free memory.
"""
import ctypes
import os

import numpy as np

from pysnptools_amd import _grm as G
from pysnptools_amd import _native as N

_MODES = ("auto", "always", "never")
_mode = [os.environ.get("PST_GRM_RECT", "auto")]


def set_grm_rect(mode):
    """When ``SnpKernel(reader, std)[rows, cols].read()`` computes the rows x cols rectangle
    directly instead of the whole K followed by a slice: ``"never"`` -- the whole-K route;
    ``"always"`` -- whenever the direct path applies (a Bed or an all-iid SnpGen, a
    Unit/Beta/trained/Identity standardizer, float32/float64, no process group of > 1 rank);
    ``"auto"`` (default) -- only when the whole K cannot be held on the device (its tiles plus the
    extraction row blocks exceed 80% of the free HBM) and the rectangle's blocks do fit, so every
    call that works on the whole-K route keeps it, and its bits.  ``PST_GRM_RECT`` sets the default
    for new processes."""
    if mode not in _MODES:
        raise ValueError("set_grm_rect: mode must be one of %s" % (_MODES,))
    _mode[0] = mode


def grm_rect_mode():
    return _mode[0] if _mode[0] in _MODES else "auto"


def _tile_bytes(n, itemsize):
    t = (int(n) + 127) // 128
    return t * (t + 1) // 2 * 128 * 128 * itemsize  # snpmi_grm_tile_bytes


def _rect_bytes(n_r, n_c, itemsize):
    return ((int(n_r) + 255) // 256) * ((int(n_c) + 255) // 256) * 65536 * itemsize  # snpmi_grm_rect_bytes


def use_rect(n, n_r, n_c, dtype, world, free_bytes, mode=None):
    """Whether K[rows, cols] (n_r x n_c) of an n-iid SnpKernel is computed directly: see
    ``set_grm_rect``.  Pure: ``free_bytes`` is the device's free memory, ``world`` the process
    group's size (1 without a group)."""
    mode = grm_rect_mode() if mode is None else mode
    if mode == "never" or world > 1:
        return False
    if mode == "always":
        return True
    item = np.dtype(dtype).itemsize
    whole = _tile_bytes(n, item) + int(n) * int(n) * item // 8  # + the extraction row blocks
    rect = _rect_bytes(n_r, n_c, item)
    return whole > 0.8 * free_bytes and rect <= 0.8 * free_bytes


def _rect_plan(snpreader, standardizer, dtype):
    """The GRM plan when the direct path can serve this reader / standardizer / dtype -- a Bed (or
    subsets of one), or an all-iid SnpGen, with a standardizer the fused GPU path knows -- else None."""
    p = G.plan(snpreader, standardizer, dtype)
    return p if p is not None and p.source in (G.BED, G.SNPGEN) else None


def rect_source(snpreader, standardizer, dtype):
    """(base, rows, cols, std_args) of ``_rect_plan``, or None."""
    p = _rect_plan(snpreader, standardizer, dtype)
    return None if p is None else (p.base, p.rows, p.cols, p.args)


def diag_pairs(row_index, col_index, n_rows=None, n_cols=None):
    """The positions (r, c) with ``row_index[r] == col_index[c]`` -- the diagonal elements of K
    inside K[rows, cols] -- as an [npairs, 2] uint32 array (every combination of repeated entries;
    None = all iids in order, then the count is required).  Host only."""
    ri, ci = N.index_array(row_index), N.index_array(col_index)
    nr = len(ri) if ri is not None else int(n_rows)
    nc = len(ci) if ci is not None else int(n_cols)
    cnt = ctypes.c_uint64(0)
    N.call("snpmi_rect_diag_pairs", N.ptr(ri), nr, N.ptr(ci), nc, None, 0, ctypes.byref(cnt))
    out = np.empty((cnt.value, 2), dtype=np.uint32)
    if cnt.value:
        N.call("snpmi_rect_diag_pairs", N.ptr(ri), nr, N.ptr(ci), nc, N.ptr(out), cnt.value, ctypes.byref(cnt))
    return out


def _free_bytes():
    free, total = ctypes.c_uint64(), ctypes.c_uint64()
    N.call("snpmi_device_memory", ctypes.byref(free), ctypes.byref(total))
    return free.value


def read_rect(snpreader, standardizer, row_index, col_index, order, dtype, num_threads=None):
    """K[row_index, col_index] of SnpKernel(snpreader, standardizer) on the direct path, or None
    when the path does not apply or ``set_grm_rect`` routes the call to the whole K."""
    from pysnptools_amd import dist as dist_mod
    from pysnptools_amd import hbm
    from pysnptools_amd.util import _on_device, get_num_threads

    dtype = np.dtype(dtype)
    mode = grm_rect_mode()
    if mode == "never":
        return None
    group = dist_mod.current()
    world = group.world if group is not None else 1
    if world > 1:
        return None
    p = _rect_plan(snpreader, standardizer, dtype)
    if p is None:
        return None
    n = p.n
    ri = None if row_index is None else N.index_array(np.arange(n)[row_index])
    ci = None if col_index is None else N.index_array(np.arange(n)[col_index])
    n_r = n if ri is None else len(ri)
    n_c = n if ci is None else len(ci)
    if mode == "auto" and not use_rect(n, n_r, n_c, dtype, world, _free_bytes(), mode):
        return None
    stats = p.stats()
    order = "C" if order not in ("C", "F") else order
    K = (hbm.empty if _on_device() else np.empty)((n_r, n_c), dtype=dtype, order=order)
    with G.session(n, dtype, K, rect=(ri, ci), order=order) as s:
        if p.source == G.SNPGEN:
            p.base._check_seeds(p.col_index())
            G.feed_snpgen(s, p, stats)
        else:
            G.feed_bed(s, p, stats, get_num_threads(num_threads))
    return K
