"""Status code and snpmi_last_error text of the argument checks that several C ABI entry points share.

Every failing call below is an argument error the library rejects on the host: no call passes a bad
pointer or a size that reaches the device.  Shapes: 5 iids x 3 SNPs selected from toydata.bed, and
3 packed SNP columns of one 64-byte pitch in device memory.

Covered rules: no session / wrong dtype / wrong iid count (whole-K and rect sessions), bad
partition, bad pitch, NULL stats with a standardizer, and per family one call that breaks two rules
and pins which one is reported.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import DATA
from pysnptools_amd import _native as N

pytestmark = pytest.mark.gpu

BED = os.path.join(DATA, "toydata.bed").encode()
N_IID, N_SID = 500, 10000
IID = np.array([3, 0, 499, 7, 250], dtype=np.uint64)
SID = np.array([9999, 0, 17], dtype=np.uint64)
n, m = len(IID), len(SID)
PITCH = 64

NO_SESSION = "no GRM session (call snpmi_grm_begin)"
DTYPE = "dtype differs from snpmi_grm_begin"
IIDS = "iid count differs from snpmi_grm_begin"
NO_RECT = "no rect GRM session (call snpmi_grm_rect_begin)"
RECT_DTYPE = "dtype differs from snpmi_grm_rect_begin"
PITCH_MSG = "pitch must be snpmi_packed_pitch"
STATS = "stats is NULL"
PART = "bad partition"

FLT = {"f32": np.float32, "f64": np.float64}
DTV = {"f32": N.DT_F32, "f64": N.DT_F64}
OTHER = {"f32": "f64", "f64": "f32"}
BOTH = pytest.mark.parametrize("sfx", ["f32", "f64"])


def rejects(msg, name, *args, code=N.E_ARG):
    """The call returns `code`, leaves exactly `msg` in snpmi_last_error, and N.call raises on it."""
    rc = getattr(N.lib(), name)(*args)
    assert (rc, N.last_error()) == (code, msg), name
    with pytest.raises(ValueError if code == N.E_ARG else IndexError) as e:
        N.call(name, *args)
    assert str(e.value) == msg, name


@pytest.fixture(scope="module")
def packed():
    """3 x 64 bytes of zeroed codes in device memory."""
    p = ctypes.c_void_p()
    N.call("snpmi_dev_alloc", ctypes.byref(p), m * PITCH)
    N.call("snpmi_dev_memset", p, 0, m * PITCH)
    N.call("snpmi_stream_sync")
    yield p
    N.call("snpmi_dev_free", p)


def end_sessions():
    for name, args in (("snpmi_grm_end", (0, None, None)), ("snpmi_grm_rect_end", (1.0, 0, None))):
        try:
            N.call(name, *args)
        except ValueError:
            pass  # none was open


@pytest.fixture(autouse=True)
def no_session_left_open():
    end_sessions()
    yield
    end_sessions()


# host arrays the calls point at (kept alive here; no failing call reads or writes them)
STATS_ARR = {s: np.zeros((m, 2), dtype=t) for s, t in FLT.items()}
VAL = {s: np.zeros((n, m), dtype=t, order="F") for s, t in FLT.items()}
DIST = {s: np.zeros((n, m, 3), dtype=t, order="F") for s, t in FLT.items()}


def stats_of(sfx):
    return STATS_ARR[sfx]


def bed_sel():
    """path .. n_out_sid of a .bed entry point: 5 iids x 3 SNPs of toydata."""
    return (BED, N_IID, N_SID, 0, N.ptr(IID), n, N.ptr(SID), m)


def std(kind=N.STD_UNIT):
    return (kind, 0.0, 0.0, 0)


# ------------------------------------------------------------------ the whole-K session's adds
def add_calls(sfx, packed, *, pitch=PITCH, stats=True, parts=1):
    """One call per entry point that adds to the whole-K session: (name, args)."""
    st = N.ptr(stats_of(sfx)) if stats else None
    val, dist = VAL[sfx], DIST[sfx]
    pk = (packed, pitch, n, m, 0) + std() + (st,)
    bed = bed_sel() + std() + (st, 1)
    return {
        "bed": ("snpmi_grm_add_bed_" + sfx, bed),
        "bed_reduce": ("snpmi_grm_add_bed_reduce_" + sfx, bed + (0, 0, parts)),
        "packed": ("snpmi_grm_add_packed_" + sfx, pk),
        "packed_reduce": ("snpmi_grm_add_packed_reduce_" + sfx, pk + (0, 0, parts, None)),
        "dense": ("snpmi_grm_add_dense_" + sfx, (N.ptr(val), n, m, 0)),
        "dist": ("snpmi_grm_add_dist_" + sfx, (N.ptr(dist), n, m, 0, m, 0, 2.0) + std() + (st,)),
    }


ADDS = ["bed", "bed_reduce", "packed", "packed_reduce", "dense", "dist"]


@BOTH
@pytest.mark.parametrize("entry", ADDS)
def test_add_without_a_session(sfx, entry, packed):
    calls = add_calls(sfx, packed)
    rejects(NO_SESSION, *_flat(calls[entry]))


@BOTH
@pytest.mark.parametrize("entry", ADDS)
def test_add_with_the_other_dtype(sfx, entry, packed):
    N.call("snpmi_grm_begin", n, DTV[OTHER[sfx]])
    calls = add_calls(sfx, packed)
    rejects(DTYPE, *_flat(calls[entry]))


@BOTH
@pytest.mark.parametrize("entry", ADDS)
def test_add_with_another_iid_count(sfx, entry, packed):
    N.call("snpmi_grm_begin", n + 1, DTV[sfx])
    calls = add_calls(sfx, packed)
    rejects(IIDS, *_flat(calls[entry]))


@BOTH
@pytest.mark.parametrize("entry", ["bed", "bed_reduce", "packed", "packed_reduce", "dist"])
def test_add_with_a_standardizer_and_no_stats(sfx, entry, packed):
    N.call("snpmi_grm_begin", n, DTV[sfx])
    calls = add_calls(sfx, packed, stats=False)
    rejects(STATS, *_flat(calls[entry]))


@BOTH
@pytest.mark.parametrize("entry", ["packed", "packed_reduce"])
def test_add_packed_with_a_bad_pitch(sfx, entry, packed):
    N.call("snpmi_grm_begin", n, DTV[sfx])
    calls = add_calls(sfx, packed, pitch=32)
    rejects(PITCH_MSG, *_flat(calls[entry]))


@BOTH
def test_add_two_violations(sfx, packed):
    """The session's dtype is reported before its iid count, the iid count before the pitch and the
    NULL stats, the pitch before the NULL stats."""
    N.call("snpmi_grm_begin", n + 1, DTV[OTHER[sfx]])
    calls = add_calls(sfx, packed)
    for entry in ADDS:
        rejects(DTYPE, *_flat(calls[entry]))
    N.call("snpmi_grm_end", 0, None, None)
    N.call("snpmi_grm_begin", n + 1, DTV[sfx])
    calls = add_calls(sfx, packed, pitch=32, stats=False)
    for entry in ADDS:
        rejects(IIDS, *_flat(calls[entry]))
    N.call("snpmi_grm_end", 0, None, None)
    N.call("snpmi_grm_begin", n, DTV[sfx])
    for entry in ("packed", "packed_reduce"):
        rejects(PITCH_MSG, *_flat(calls[entry]))
    # dist: the SNP range is checked before the session
    name, args = calls["dist"]
    rejects("SNP range outside the dist array", name, *(args[:3] + (1,) + args[4:]), code=N.E_INDEX)


def test_reduce_arguments(packed):
    """collective and parts come after the session's dtype and before its iid count; the f64 forms
    take parts < 1 as 1 (the CRT path's own residue chunks are the groups)."""
    N.call("snpmi_grm_begin", n + 1, N.DT_F32)
    calls = add_calls("f32", packed, parts=0)
    for entry in ("bed_reduce", "packed_reduce"):
        rejects("parts must be >= 1", *_flat(calls[entry]))
        name, args = calls[entry]
        bad = list(args)
        bad[-3 if entry == "bed_reduce" else -4] = 3
        rejects("collective must be 0 (none), 1 (reduce), 2 (all-reduce)", name, *bad)
    N.call("snpmi_grm_end", 0, None, None)
    N.call("snpmi_grm_begin", n + 1, N.DT_F64)
    calls = add_calls("f64", packed, parts=0)
    for entry in ("bed_reduce", "packed_reduce"):
        rejects(IIDS, *_flat(calls[entry]))
    rejects("parts must be >= 1", "snpmi_grm_session_sum", 0, 0, 0)
    N.call("snpmi_grm_end", 0, None, None)
    rejects(NO_SESSION, "snpmi_grm_session_sum", 0, 0, 1)
    rejects(NO_SESSION, "snpmi_grm_session_tiles", None, None)
    rejects(NO_SESSION, "snpmi_grm_end", 0, None, None)


def _flat(call):
    return (call[0],) + tuple(call[1])


# ------------------------------------------------------------------ the rect session's adds
def rect_calls(sfx, packed, *, pitch=PITCH, stats=True):
    st = N.ptr(stats_of(sfx)) if stats else None
    return {
        "packed": ("snpmi_grm_rect_add_packed_" + sfx, (packed, pitch, n, m, 0) + std() + (st, None, None)),
        "bed": ("snpmi_grm_rect_add_bed_" + sfx, bed_sel() + std() + (st, 1, None, None)),
    }


@BOTH
@pytest.mark.parametrize("entry", ["packed", "bed"])
def test_rect_add_session_checks(sfx, entry, packed):
    name, args = rect_calls(sfx, packed)[entry]
    rejects(NO_RECT, name, *args)
    N.call("snpmi_grm_rect_begin", n, n, DTV[OTHER[sfx]])
    rejects(RECT_DTYPE, name, *args)
    N.call("snpmi_grm_rect_end", 1.0, 0, None)
    N.call("snpmi_grm_rect_begin", n + 1, n, DTV[sfx])
    rejects("row count differs from snpmi_grm_rect_begin", name, *args)
    N.call("snpmi_grm_rect_end", 1.0, 0, None)
    N.call("snpmi_grm_rect_begin", n, n + 2, DTV[sfx])
    rejects("col count differs from snpmi_grm_rect_begin", name, *args)
    N.call("snpmi_grm_rect_end", 1.0, 0, None)
    rejects(NO_RECT, "snpmi_grm_rect_end", 1.0, 0, None)


@BOTH
def test_rect_add_argument_checks(sfx, packed):
    N.call("snpmi_grm_rect_begin", n, n, DTV[sfx])
    rejects(PITCH_MSG, *_flat(rect_calls(sfx, packed, pitch=32)["packed"]))
    for entry in ("packed", "bed"):
        rejects(STATS, *_flat(rect_calls(sfx, packed, stats=False)[entry]))
    # two violations: the pitch before the NULL stats; the session's dtype before either
    rejects(PITCH_MSG, *_flat(rect_calls(sfx, packed, pitch=32, stats=False)["packed"]))
    N.call("snpmi_grm_rect_end", 1.0, 0, None)
    N.call("snpmi_grm_rect_begin", n + 1, n, DTV[OTHER[sfx]])
    for entry in ("packed", "bed"):
        rejects(RECT_DTYPE, *_flat(rect_calls(sfx, packed, pitch=32, stats=False)[entry]))
    # a whole-K session does not stand in for a rect session
    N.call("snpmi_grm_rect_end", 1.0, 0, None)
    N.call("snpmi_grm_begin", n, DTV[sfx])
    for entry in ("packed", "bed"):
        rejects(NO_RECT, *_flat(rect_calls(sfx, packed)[entry]))


# ------------------------------------------------------------------ partitioned K
BAD_PARTS = [(0, 0), (-1, 2), (2, 2), (3, 2)]


@pytest.mark.parametrize("rank,world", BAD_PARTS)
def test_bad_partition(rank, world, packed):
    assert N.lib().snpmi_grm_part_blocks(n, rank, world) == 0
    r0, c0 = ctypes.c_uint64(), ctypes.c_uint64()
    rejects(PART, "snpmi_grm_part_coords", n, rank, world, 0, ctypes.byref(r0), ctypes.byref(c0))
    coords = np.zeros((1, 2), dtype=np.uint64)
    rejects(PART, "snpmi_grm_part_coords_all", n, rank, world, N.ptr(coords))
    tr = ctypes.c_double()
    for sfx in ("f32", "f64"):
        blocks = np.zeros((1, 256, 256), dtype=FLT[sfx])
        out = np.zeros((n, n), dtype=FLT[sfx])
        st = stats_of(sfx)
        rejects("bad rank / world", "snpmi_grm_part_bed_" + sfx,
                *(bed_sel() + std() + (N.ptr(st), rank, world, N.ptr(blocks), 1)))
        # two violations: the partition before the NULL output / the NULL stats
        rejects("bad rank / world", "snpmi_grm_part_bed_" + sfx, *(bed_sel() + std() + (None, rank, world, None, 1)))
        rejects(PART, "snpmi_grm_part_extract_" + sfx, packed, n, rank, world, None, n, None, n, 1, 1.0, N.ptr(out))
        rejects(PART, "snpmi_grm_part_extract_" + sfx, packed, n, rank, world, None, n, None, n, 1, 1.0, None)
        rejects(PART, "snpmi_grm_part_trace_" + sfx, packed, n, rank, world, ctypes.byref(tr))
        rejects(PART, "snpmi_grm_part_trace_" + sfx, packed, n, rank, world, None)
    for name in ("snpmi_dev_syrk_packed_part", "snpmi_dev_syrk_packed_part_f64"):
        rejects(PART, name, packed, PITCH, n, m, packed, rank, world, packed, 0)
        rejects(PART, name, packed, 32, n, m, packed, rank, world, packed, 0)  # ... before the pitch


@BOTH
def test_part_argument_checks(sfx, packed):
    blocks = np.zeros((1, 256, 256), dtype=FLT[sfx])
    rejects("blocks_out is NULL", "snpmi_grm_part_bed_" + sfx, *(bed_sel() + std() + (None, 0, 1, None, 1)))
    rejects(STATS, "snpmi_grm_part_bed_" + sfx, *(bed_sel() + std() + (None, 0, 1, N.ptr(blocks), 1)))
    rejects("out is NULL", "snpmi_grm_part_extract_" + sfx, packed, n, 0, 1, None, n, None, n, 1, 1.0, None)
    rejects("trace is NULL", "snpmi_grm_part_trace_" + sfx, packed, n, 0, 1, None)


# ------------------------------------------------------------------ packed SNPs in HBM
def test_bad_pitch_of_the_device_entry_points(packed):
    for pitch in (32, 96, 0):
        rejects(PITCH_MSG, "snpmi_dev_syrk_packed", packed, pitch, n, m, packed, N.DT_F32, packed, 0)
        rejects(PITCH_MSG, "snpmi_dev_syrk_packed_part", packed, pitch, n, m, packed, 0, 1, packed, 0)
        rejects(PITCH_MSG, "snpmi_dev_syrk_packed_part_f64", packed, pitch, n, m, packed, 0, 1, packed, 0)
        rejects(PITCH_MSG, "snpmi_dev_snp_stats", packed, pitch, n, m, 0, N.STD_UNIT, 0.0, 0.0, 0, N.DT_F32, packed,
                packed)
        rejects(PITCH_MSG, "snpmi_dev_decode", packed, pitch, n, m, packed, N.DT_F32, 0, packed, 16)
        rejects(PITCH_MSG, "snpmi_dev_decode_standardize", packed, pitch, n, m, 0, N.STD_UNIT, 0.0, 0.0, 0, N.DT_F32,
                packed, packed, packed, 16)
        rejects("pitch must be a multiple of 64 >= ceil(n/4)", "snpmi_dev_encode", packed, N.DT_F32, 0, 16, n, m, 0,
                packed, pitch, None)
    # a pitch of 64 bytes holds 256 iids, not 257
    rejects(PITCH_MSG, "snpmi_dev_syrk_packed", packed, PITCH, 257, m, packed, N.DT_F32, packed, 0)
    # two violations: the dtype before the pitch
    rejects("GRM dtype must be f32/f64", "snpmi_dev_syrk_packed", packed, 32, n, m, packed, N.DT_I8, packed, 0)
    rejects("fused decode+standardize is f32 only", "snpmi_dev_decode_standardize", packed, 32, n, m, 0, N.STD_UNIT,
            0.0, 0.0, 0, N.DT_F64, packed, packed, packed, 16)


@BOTH
def test_bad_standardizer_kind_and_null_packed(sfx, packed):
    N.call("snpmi_grm_begin", n, DTV[sfx])
    st = stats_of(sfx)
    for name, tail in (("snpmi_grm_add_packed_" + sfx, ()), ("snpmi_grm_add_packed_reduce_" + sfx, (0, 0, 1, None))):
        rejects("bad standardizer kind", name, packed, PITCH, n, m, 0, 3, 0.0, 0.0, 0, N.ptr(st), *tail)
        rejects(PITCH_MSG, name, packed, 32, n, m, 0, 3, 0.0, 0.0, 0, N.ptr(st), *tail)
    rejects("packed is NULL", "snpmi_grm_add_packed_" + sfx, None, PITCH, n, m, 0, *std(), N.ptr(st))
    rejects("packed must be device memory of the current device", "snpmi_grm_add_packed_" + sfx, N.ptr(st), PITCH, n,
            m, 0, *std(), N.ptr(st))


# ------------------------------------------------------------------ whole-file entry points
@BOTH
def test_null_stats_of_the_one_call_entry_points(sfx):
    K = np.zeros((n, n), dtype=FLT[sfx])
    out = np.zeros((n, m), dtype=FLT[sfx], order="F")
    rejects(STATS, "snpmi_grm_bed_" + sfx, *(bed_sel() + std() + (None, 0, None, N.ptr(K), 1)))
    rejects(STATS, "snpmi_bed_read_standardize_" + sfx, *(bed_sel() + (0,) + std() + (None, N.ptr(out), 1)))
    rejects(STATS, "snpmi_standardize_" + sfx, N.ptr(out), n, m, 0, 0, 0.0, 0.0, 1, 0, None, 1)
    # two violations: grm_bed reports its NULL output first, bed_read_standardize the NULL stats
    rejects("K_out is NULL", "snpmi_grm_bed_" + sfx, *(bed_sel() + std() + (None, 0, None, None, 1)))
    rejects(STATS, "snpmi_bed_read_standardize_" + sfx, *(bed_sel() + (0,) + std() + (None, None, 1)))
