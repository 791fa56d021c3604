"""Genotype distributions on the GPU: the two conversions (csrc/dist.hip) pinned bit for bit against
NumPy, the reference's goldens (tests/golden/dist.npz, tools/make_golden_dist.py), and the GRM of
``dist.as_snp()`` through the session route (snpmi_grm_add_dist_*) against float64 NumPy.

Tolerances are the ones the dense-operand GRM already carries (tests/test_gpu_parity.py
test_grm_dense_snpdata_vs_reference: 1e-5 of max diag in float32, 1e-10 in float64) and the dense
standardizer's stats (tests/test_gpu_std_dense.py: rtol = atol = 1e-6)."""
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN
from oracle import oracle as O
from pysnptools_amd import _native as N
from pysnptools_amd import hbm
from pysnptools_amd.distreader import DistData, DistMemMap, DistNpz
from pysnptools_amd.distreader._snp2dist import snp_to_dist
from pysnptools_amd.kernelreader import SnpKernel
from pysnptools_amd.snpreader import Bed, SnpData
from pysnptools_amd.snpreader._dist2snp import dist_to_snp
from pysnptools_amd.standardizer import Beta, Unit
from test_gpu_parity import grm_close

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 4, 5, 63, 64, 65, 130)
COLS = (1, 2, 3, 5, 64, 65)
WEIGHTS = (2.0, 1.0, 0.7)
RANGES = ((7, 2, 3), (70, 1, 65), (70, 64, 6))  # (cols_total, col0, cols): misaligned planes and rows
_G = {}


def golden():
    if not _G:
        with np.load(os.path.join(GOLDEN, "dist.npz"), allow_pickle=False) as z:
            _G.update({k: z[k] for k in z.files})
    return _G


def same_bits(a, b):
    """Equal shape, dtype, NaN positions and bits everywhere else (+0 and -0 differ)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.ascontiguousarray(a).view(u)[~na],
                                                          np.ascontiguousarray(b).view(u)[~nb]))


def triples(rng, rows, cols, dtype, order):
    """Random distributions (each sums to 1) with whole-NaN triples, NaN in one component only, and
    one triple of negative zeros."""
    p = rng.random((rows, cols, 3))
    p /= p.sum(axis=-1, keepdims=True)
    p[rng.random((rows, cols)) < 0.1] = np.nan
    flat = p.reshape(-1, 3)
    pick = rng.permutation(len(flat))
    for k in range(3):  # NaN in only p0, only p1, only p2
        for t in pick[k::7][:max(1, len(flat) // 20)]:
            flat[t] = rng.dirichlet((1, 1, 1))
            flat[t, k] = np.nan
    flat[pick[-1]] = -0.0
    return np.array(p, dtype=dtype, order=order)


def numpy_dosage(val, max_weight, col0=0, cols=None):
    """_dist2snp.py:47-52 on the host, in val's dtype."""
    cols = val.shape[1] - col0 if cols is None else cols
    weights = np.array([0, .5, 1], dtype=val.dtype) * max_weight
    return (val[:, col0:col0 + cols] * weights).sum(axis=-1)


def snpval_to_distval(snpval, max_weight, order):
    """_snp2dist.py:41-54 restated on the host."""
    distval = np.zeros([snpval.shape[0], snpval.shape[1], 3], dtype=snpval.dtype, order=order)
    distval = distval.reshape(-1, 3, order=order)
    factor = 2.0 / max_weight
    for count in range(3):
        distval[snpval.reshape(-1, order=order) * factor == count, count] = 1
    distval[distval.sum(axis=-1) != 1, :] = np.nan
    return distval.reshape([snpval.shape[0], snpval.shape[1], 3], order=order)


# ---------------------------------------------------------------------------------- 1. dist -> snp
@pytest.mark.parametrize("out_order", ["F", "C"])
@pytest.mark.parametrize("src_order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dist_to_snp_bit_exact(dtype, src_order, out_order):
    rng = np.random.default_rng(5)
    shapes = [(r, c, 0, c) for r in ROWS for c in COLS] + [(r, t, c0, c) for r in ROWS for t, c0, c in RANGES]
    for rows, cols_total, col0, cols in shapes:
        val = triples(rng, rows, cols_total, dtype, src_order)
        dev = hbm.asarray(val, order=src_order)
        assert dev.order == src_order or val.flags[dev.order + "_CONTIGUOUS"]
        for mw in WEIGHTS:
            want = numpy_dosage(val, mw, col0, cols)
            where = (rows, cols_total, col0, cols, mw)
            got = dist_to_snp(val, col0, cols, mw, out_order)
            assert isinstance(got, np.ndarray) and got.flags[out_order + "_CONTIGUOUS"], where
            assert same_bits(got, want), where
            got_dev = dist_to_snp(dev, col0, cols, mw, out_order)
            assert isinstance(got_dev, hbm.HbmArray) and got_dev.order == out_order, where
            assert same_bits(got_dev.get(), want), where


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dist_to_snp_empty(dtype):
    for order in ("F", "C"):
        for shape in ((0, 5, 3), (4, 0, 3), (0, 0, 3)):
            val = np.zeros(shape, dtype=dtype, order=order)
            out = dist_to_snp(val, 0, shape[1], 2.0, order)
            assert out.shape == shape[:2] and out.dtype == dtype
        val = np.zeros((4, 5, 3), dtype=dtype, order=order)
        assert dist_to_snp(val, 2, 0, 2.0, order).shape == (4, 0)
        N.call("snpmi_dist_to_snp_" + N.suffix(dtype), N.ptr(val), 0, 5, 0, 5, 0, 2.0, None, 0)
        with pytest.raises(IndexError):
            N.call("snpmi_dist_to_snp_" + N.suffix(dtype), N.ptr(val), 4, 5, 3, 3, 0, 2.0, N.ptr(np.empty((4, 3), dtype)), 0)


# ---------------------------------------------------------------------------------- 2. snp -> dist
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_as_dist_matches_the_reference(dtype):
    G = golden()
    for mw in (2, 1):
        for order in ("F", "C"):
            data = SnpData(iid=[["f%d" % i, "i%d" % i] for i in range(3)], sid=["s%d" % j for j in range(4)],
                           val=np.array(G["as_dist_in"], dtype=dtype, order=order))
            got = data.as_dist(max_weight=mw).read(order=order, dtype=dtype).val
            assert got.flags[order + "_CONTIGUOUS"]
            assert same_bits(got, G["as_dist_w%d" % mw].astype(dtype))
            assert same_bits(got, snpval_to_distval(data.val, float(mw), order))
    # every value class, odd sizes (vector body + tails), a weight whose factor is inexact
    rng = np.random.default_rng(3)
    pool = np.array([0, 1, 2, np.nan, 0.5, 1.5, -0.0, 0.7, 1.4, 3, -1], dtype=dtype)
    for rows, cols in ((1, 1), (5, 3), (63, 5), (130, 65)):
        for order in ("F", "C"):
            val = np.array(pool[rng.integers(0, len(pool), size=(rows, cols))], order=order)
            for mw in (2.0, 1.0, 0.7):
                want = snpval_to_distval(val, mw, order)
                assert same_bits(snp_to_dist(val, mw, order), want), (rows, cols, order, mw)
                got = snp_to_dist(hbm.asarray(val, order=order), mw, order)
                assert isinstance(got, hbm.HbmArray) and same_bits(got.get(), want), (rows, cols, order, mw)


@pytest.mark.parametrize("name,n", [("n300", 300), ("gen4", 198)])
def test_as_dist_of_a_bed_is_one_hot(name, n):
    bed = Bed(os.path.join(DATA, name + ".bed"), count_A1=False)
    assert bed.iid_count == n
    val = bed.read().val
    got = bed.as_dist().read().val
    assert got.shape == val.shape + (3,) and got.flags["F_CONTIGUOUS"]
    want = np.stack([np.where(np.isnan(val), np.nan, (val == c).astype(np.float64)) for c in range(3)], axis=-1)
    assert same_bits(got, want)
    # in SNP blocks (more SNPs than the block and, for n300, than iids), and a subset pushed down
    sub = bed[::3, 5:40]
    blocked = sub.as_dist(block_size=9).read(order="C", dtype=np.float32).val
    assert blocked.flags["C_CONTIGUOUS"] and same_bits(blocked, want[::3, 5:40].astype(np.float32))
    if name == "n300":
        assert same_bits(bed.as_dist(block_size=400).read().val, want)


# ---------------------------------------------------------------------------------- 3. round trip
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bed_round_trip(dtype, order):
    for name in ("n300", "gen4"):
        bed = Bed(os.path.join(DATA, name + ".bed"), count_A1=False)
        back = bed.as_dist().as_snp().read(order=order, dtype=dtype).val
        assert back.flags[order + "_CONTIGUOUS"]
        assert same_bits(back, bed.read(order=order, dtype=dtype).val)


# ---------------------------------------------------------------------------------- 4. goldens
@pytest.mark.parametrize("name", ["toydata10", "distgen"])
def test_as_snp_matches_the_reference(name):
    G = golden()
    npz = DistNpz(os.path.join(DATA, name + ".dist.npz"))
    data = npz.read()
    for mw in (2, 1):
        for tag, block in (("", None), ("_b3", 3)):
            want = G["%s_snp_w%d%s" % (name, mw, tag)]
            for src in (npz, data, npz[:, :], data[np.arange(data.iid_count), :]):
                got = src.as_snp(max_weight=mw, block_size=block).read().val
                assert same_bits(got, want), (mw, block, src)
    # an iid subset and a SNP list take the gather path; a SNP range reads the base in place
    want = G[name + "_snp_w2"]
    assert same_bits(data[::2, [3, 0]].as_snp().read().val, want[::2][:, [3, 0]])
    assert same_bits(npz.as_snp()[:, 1:4].read(order="C").val, np.ascontiguousarray(want[:, 1:4]))
    got = data.as_snp().read(xp="hbm")
    assert isinstance(got.val, hbm.HbmArray) and same_bits(got.val.get(), want)
    if name == "toydata10":
        mm = DistMemMap(os.path.join(DATA, "tiny.dist.memmap"))
        assert same_bits(mm.as_snp().read().val, want)
        assert same_bits(mm.as_snp().read(dtype=np.float32).val, numpy_dosage(mm.val.astype(np.float32), 2.0))


# ---------------------------------------------------------------------------------- 5. GRM
_CASES = {}


def grm_case(n, m):
    """Seeded distributions with 5% NaN triples and their float64 dosage, shared by the GRM tests."""
    if (n, m) not in _CASES:
        rng = np.random.default_rng(n + m)
        p = rng.random((n, m, 3))
        p /= p.sum(axis=-1, keepdims=True)
        p[rng.random((n, m)) < 0.05] = np.nan
        iid = np.array([["f%d" % i, "i%d" % i] for i in range(n)])
        sid = np.array(["s%d" % j for j in range(m)])
        refs = {}
        for name, kw in (("unit", {}), ("beta", dict(is_beta=True, a=1, b=25))):
            Z = np.array(numpy_dosage(p, 2.0), order="F")
            stats = O.standardize_native(Z, **kw)
            refs[name] = (Z.dot(Z.T), stats)
        for v in refs.values():
            for a in v:
                a.setflags(write=False)
        p.setflags(write=False)
        _CASES[(n, m)] = (iid, sid, p, refs)
    return _CASES[(n, m)]


@pytest.mark.parametrize("src", ["F", "C", "hbm"])
@pytest.mark.parametrize("std_name", ["unit", "beta"])
@pytest.mark.parametrize("dtype,tol", [(np.float32, 1e-5), (np.float64, 1e-10)])
@pytest.mark.parametrize("n,m,block", [(300, 70, 32), (4097, 40, 16)])
def test_grm_of_as_snp(n, m, block, dtype, tol, std_name, src):
    iid, sid, p, refs = grm_case(n, m)
    Kref, stats_ref = refs[std_name]
    std = Unit() if std_name == "unit" else Beta(1, 25)
    val = np.array(p, dtype=dtype, order="C" if src == "C" else "F")
    dist = DistData(iid, sid, hbm.asarray(val) if src == "hbm" else val)
    snps = dist.as_snp()
    K, trained = snps._read_kernel(std, block_size=block, dtype=dtype, return_trained=True)
    assert isinstance(K, hbm.HbmArray) == (src == "hbm")
    K = np.asarray(K)
    assert K.dtype == dtype and np.array_equal(K, K.T)
    grm_close(K, Kref, tol)
    np.testing.assert_allclose(np.asarray(trained.stats, dtype=np.float64), stats_ref, rtol=1e-6, atol=1e-6)
    if src == "hbm":
        return
    # the same kernel on the same values: stats identical to standardizing the converted SnpData
    _, tr2 = SnpData(iid, sid, snps.read(dtype=dtype).val).standardize(std, return_trained=True)
    assert same_bits(np.asarray(trained.stats), np.asarray(tr2.stats))
    # the trained standardizer applied again, the public read_kernel and SnpKernel
    grm_close(snps._read_kernel(trained, block_size=block, dtype=dtype), Kref, tol)
    Kpub = snps.read_kernel(std, block_size=block, dtype=dtype).val
    assert np.array_equal(Kpub, K)
    assert np.array_equal(SnpKernel(snps, std, block_size=block).read(dtype=dtype).val, K)
    # a SNP range of the same array (misaligned planes), whole
    sub = snps[:, 3:m - 2]
    Z = np.array(numpy_dosage(p, 2.0)[:, 3:m - 2], order="F")
    O.standardize_native(Z, **({} if std_name == "unit" else dict(is_beta=True, a=1, b=25)))
    grm_close(sub.read_kernel(std, dtype=dtype).val, Z.dot(Z.T), tol)


def test_grm_of_toydata10_matches_the_reference():
    G = golden()
    npz = DistNpz(os.path.join(DATA, "toydata10.dist.npz"))
    mm = DistMemMap(os.path.join(DATA, "tiny.dist.memmap"))
    for src in (npz, mm):
        grm_close(src.as_snp().read_kernel(Unit()).val, G["toydata10_K_unit"], 1e-10)
        grm_close(src.as_snp().read_kernel(Beta(1, 25), block_size=3).val, G["toydata10_K_beta"], 1e-10)
    # a selection the native branch refuses takes the generic block loop
    K = npz[:, [0, 2, 1, 3, 4, 5, 6, 7, 8, 9]].as_snp().read_kernel(Unit()).val
    grm_close(K, G["toydata10_K_unit"], 1e-10)


def test_grm_add_dist_needs_a_session_and_skips_empty_blocks():
    val = np.zeros((4, 5, 3), dtype=np.float32, order="F")
    st = np.empty((5, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="no GRM session"):
        N.call("snpmi_grm_add_dist_f32", N.ptr(val), 4, 5, 0, 5, 0, 2.0, N.STD_UNIT, np.nan, np.nan, 0, N.ptr(st))
    K = np.empty((4, 4), dtype=np.float32)
    N.call("snpmi_grm_begin", 4, N.DT_F32)
    try:
        N.call("snpmi_grm_add_dist_f32", N.ptr(val), 4, 5, 2, 0, 0, 2.0, N.STD_UNIT, np.nan, np.nan, 0, N.ptr(st))
        with pytest.raises(ValueError, match="iid count differs"):
            N.call("snpmi_grm_add_dist_f32", N.ptr(val), 3, 5, 0, 5, 0, 2.0, N.STD_UNIT, np.nan, np.nan, 0, N.ptr(st))
    finally:
        N.call("snpmi_grm_end", 0, None, N.ptr(K))
    assert not K.any()


# ---------------------------------------------------------------------------------- 6. empty
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_snps(dtype):
    data = DistNpz(os.path.join(DATA, "toydata10.dist.npz")).read()
    for dist in (data, DistMemMap(os.path.join(DATA, "tiny.dist.memmap"))):
        sub = dist[:, []].as_snp()
        assert sub.sid_count == 0
        v = sub.read(dtype=dtype).val
        assert v.shape == (25, 0) and v.dtype == dtype
        K = sub.read_kernel(Unit(), dtype=dtype).val
        assert K.shape == (25, 25) and K.dtype == dtype and not K.any()
        K2 = SnpKernel(sub, Unit()).read(dtype=dtype).val
        assert K2.shape == (25, 25) and not K2.any()
