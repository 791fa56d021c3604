"""Z^T V, Z W and K V on packed SNPs (csrc/matvec.hip, include/snpmi.h snpmi_dev_packed_tdot /
snpmi_dev_packed_dot, pysnptools_amd.linop.SnpOperator).

Ground truth.  Z is rebuilt on the host from the codes and from the LUT that snpmi_dev_snp_stats wrote
for the same device buffer (Z[i, s] = lut[4 s + code(i, s)]), and the product is NumPy's in float64:
only the kernels' own summation is under test.

Bars (valid for any order of summation, FMA or not; t = number of terms; the factor 2 as in
test_gpu_dense_edges.within_bar):
  float64   |out - ref| <= 2 (t + 2) 2^-53 (|Z|^T |V|)            elementwise
  float32   |out - ref| <= 2 (min(t, 16384) + 2) 2^-24 (|Z|^T |V|)
and the same with |Z| |W| for Z W; `accumulate` counts the previous value as one more term.  A NaN
where the reference is finite fails, and so does the reverse.

Exact data: no standardization, no missing genotype, operand integers in [-8, 8].  Every partial sum is
an integer below 2^24, so the result equals the integer product bit for bit in both dtypes.

Every launch owns its leading dimensions: inputs are padded with NaN, outputs start as 0xFF bytes (a NaN
pattern) and their padding must keep those bytes.

Shapes.  The kernels' constants (matvec.hip): a lane holds 16 iids, a wave 1024 (kSpan), a tdot
workgroup 4096 (kChunk); tdot folds its waves every 64 SNPs (kTdotSub) and a workgroup takes 256 SNPs
(kTdotSnps); a dot segment is 256 SNPs (kSeg); 8 code words are in flight (kLoads); a panel is 8 (f32)
or 4 (f64) columns, narrower ones 4 / 2 / 1.  SHAPES holds every n, m and k the contract lists plus
n = 1024, 4095, 4096; m = 8, 9, 255, 256, 257, 513, 600 (above two segments); k = 12, 15 (8 + 4,
8 + 4 + 2 + 1).
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import DATA
from pysnptools_amd import _native as N

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DTYPES = [F32, F64]
IDS = ["f32", "f64"]
SEG = 256  # kSeg
SHAPES = [(1, 1, 1), (3, 2, 2), (4, 7, 3), (5, 64, 4), (15, 65, 5), (16, 300, 7), (17, 0, 8), (63, 1, 9), (64, 2, 16),
          (65, 7, 17), (255, 64, 33), (256, 65, 1), (257, 300, 2), (1023, 8, 3), (1024, 9, 15), (1025, 255, 4),
          (4095, 256, 5), (4096, 257, 12), (4097, 600, 8), (300, 513, 9)]
UNIT = (N.STD_UNIT, 0.0, 0.0, 0)
IDENTITY = (N.STD_NONE, 0.0, 0.0, 0)


def hbm():
    from pysnptools_amd import hbm as H

    return H


def pack(codes, pitch, poison):
    """codes [n][m] in 0 ... 3 -> [m][pitch] bytes, iid i in bits 2 (i % 4) of byte i / 4.  poison: the
    unused codes of the last byte are the missing code (1), the pad bytes up to pitch 0xFF."""
    n, m = codes.shape
    full = np.full((m, pitch * 4), 1 if poison else 0, dtype=np.uint8)
    full[:, :n] = codes.T
    q = full.reshape(m, pitch, 4)
    out = (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)
    if poison:
        out[:, (n + 3) // 4:] = 0xFF
    return np.ascontiguousarray(out)


class Snps(object):
    """Packed codes in HBM with the LUT snpmi_dev_snp_stats makes of them, and Z on the host."""

    def __init__(self, codes, dtype, std=UNIT, count_a1=0, poison=True, stats=None):
        H = hbm()
        self.n, self.m = codes.shape
        self.dtype, self.dt = np.dtype(dtype), N.dt_code(dtype)
        self.pitch = int(N.lib().snpmi_packed_pitch(self.n))
        self.packed = H.asarray(pack(codes, self.pitch, poison) if self.m else np.zeros((1, self.pitch), np.uint8))
        self.lut_dev = H.empty((max(self.m, 1), 4), dtype=self.dtype)
        st = H.empty((max(self.m, 1), 2), dtype=self.dtype) if stats is None else H.asarray(
            np.ascontiguousarray(stats, dtype=self.dtype))
        if self.m:
            N.call("snpmi_dev_snp_stats", self.packed.snpmi_ptr, self.pitch, self.n, self.m, count_a1, *std, self.dt,
                   st.snpmi_ptr, self.lut_dev.snpmi_ptr)
        self.stats = st.get()[:self.m]
        self.lut = self.lut_dev.get()[:self.m]
        self.Z = self.lut.astype(np.float64)[np.arange(self.m)[None, :], codes] if self.m else np.zeros((self.n, 0))

    def at(self, s):
        return (ctypes.c_void_p(self.packed.ptr + s * self.pitch),
                ctypes.c_void_p(self.lut_dev.ptr + 4 * s * self.dtype.itemsize))


def padded(a, ld):
    """[rows][k] host -> device [k][ld] with NaN between the rows and ld."""
    rows, k = a.shape
    buf = np.full((max(k, 1), ld), np.nan, dtype=a.dtype)
    buf[:k, :rows] = a.T
    return hbm().asarray(buf)


def poisoned_out(rows, k, ld, dtype, prev=None):
    buf = np.frombuffer(b"\xff" * (max(k, 1) * ld * dtype.itemsize), dtype=dtype).reshape(max(k, 1), ld).copy()
    if prev is not None:
        buf[:k, :rows] = prev.T
    return hbm().asarray(buf)


def unpadded(dev, rows, k, ld):
    """device [k][ld] -> host [rows][k]; the padding must still be 0xFF bytes."""
    buf = dev.get()
    assert (buf[:k, rows:].view(np.uint8) == 0xFF).all(), "output padding was written"
    return np.ascontiguousarray(buf[:k, :rows].T)


def tdot(S, V, pad=(3, 5), s0=0, cnt=None):
    cnt = S.m - s0 if cnt is None else cnt
    k, ldv, ldg = V.shape[1], S.n + pad[0], cnt + pad[1]
    Vd, Gd = padded(V, ldv), poisoned_out(cnt, k, ldg, S.dtype)
    packed, lut = S.at(s0)
    N.call("snpmi_dev_packed_tdot", packed, S.pitch, S.n, cnt, lut, S.dt, Vd.snpmi_ptr, ldv, k, Gd.snpmi_ptr, ldg)
    N.call("snpmi_stream_sync")
    return unpadded(Gd, cnt, k, ldg)


def dot(S, W, pad=(5, 7), s0=0, cnt=None, prev=None, Yd=None):
    """Z[:, s0 : s0 + cnt] W[s0 : s0 + cnt]; prev: Y beforehand (accumulate); Yd: accumulate into this
    device buffer (of this function) instead."""
    cnt = S.m - s0 if cnt is None else cnt
    k, ldw, ldy = W.shape[1], cnt + pad[0], S.n + pad[1]
    Wd = padded(W[s0:s0 + cnt], ldw)
    acc = int(prev is not None or Yd is not None)
    Yd = poisoned_out(S.n, k, ldy, S.dtype, prev) if Yd is None else Yd
    packed, lut = S.at(s0)
    N.call("snpmi_dev_packed_dot", packed, S.pitch, S.n, cnt, lut, S.dt, Wd.snpmi_ptr, ldw, k, Yd.snpmi_ptr, ldy, acc)
    N.call("snpmi_stream_sync")
    return unpadded(Yd, S.n, k, ldy), Yd


def check_bar(out, ref, absref, t, dtype, label):
    """The dtype's bar, elementwise; NaNs must match the reference's."""
    assert out.dtype == dtype and out.shape == ref.shape, label
    assert np.array_equal(np.isnan(out), np.isnan(ref)), (label, "NaN pattern differs")
    ok = ~np.isnan(ref)
    u, cap = (2.0 ** -24, min(t, 16384)) if dtype == F32 else (2.0 ** -53, t)
    bound = 2 * (cap + 2) * u * absref
    d = np.abs(out.astype(np.float64) - ref)
    worst = (d[ok] / np.where(bound[ok] > 0, bound[ok], 1)).max() if ok.any() else 0.0
    print(label, "error / bound %.3e" % worst)
    assert (d[ok] <= bound[ok]).all(), (label, worst)


def random_codes(rng, n, m, miss=0.03):
    codes = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=(n, m), p=[0.5, 0.35, 0.15])
    codes[rng.random((n, m)) < miss] = 1
    return codes


def operand(rng, rows, k, dtype):
    return rng.standard_normal((rows, k)).astype(dtype)


def tdot_refs(S, V):
    V64 = V.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return S.Z.T @ V64, np.abs(S.Z).T @ np.abs(V64)


def dot_refs(S, W):
    W64 = W.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return S.Z @ W64, np.abs(S.Z) @ np.abs(W64)


# ---------------------------------------------------------------------- the low-level entries
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shapes_within_bar(dtype):
    """Unit on codes with 3% missing, poisoned packed buffer, padded operands, both products; the dot
    also accumulating onto a previous Y."""
    rng = np.random.default_rng(1)
    for n, m, k in SHAPES:
        S = Snps(random_codes(rng, n, m), dtype)
        V, W = operand(rng, n, k, dtype), operand(rng, m, k, dtype)
        ref, aref = tdot_refs(S, V)
        check_bar(tdot(S, V), ref, aref, n, dtype, "tdot %s" % ((n, m, k),))
        ref, aref = dot_refs(S, W)
        if m == 0:
            assert (dot(S, W)[0] == 0).all()  # no SNPs: zeros written
        else:
            check_bar(dot(S, W)[0], ref, aref, m, dtype, "dot %s" % ((n, m, k),))
        prev = operand(rng, n, k, dtype)
        out = dot(S, W, prev=prev)[0]
        if m == 0:
            assert np.array_equal(out, prev)  # nothing launched
        else:
            check_bar(out, ref + prev, aref + np.abs(prev), m + 1, dtype, "dot+ %s" % ((n, m, k),))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_data_any_order(dtype):
    """Identity LUT, no missing genotype, integer operands: the integer product, bit for bit -- with
    the unused codes of the last byte set to the missing code (NaN under this LUT) and the pad bytes
    0xFF, so an iid >= n that is added, or multiplied by zero, shows as NaN."""
    rng = np.random.default_rng(2)
    for n, m, k in SHAPES:
        codes = random_codes(rng, n, m, miss=0.0)
        S = Snps(codes, dtype, std=IDENTITY, poison=True)
        assert np.isfinite(S.Z).all()
        V = rng.integers(-8, 9, size=(n, k)).astype(dtype)
        W = rng.integers(-8, 9, size=(m, k)).astype(dtype)
        assert np.array_equal(tdot(S, V), (S.Z.T @ V.astype(np.float64)).astype(dtype)), ("tdot", n, m, k)
        assert np.array_equal(dot(S, W)[0], (S.Z @ W.astype(np.float64)).astype(dtype)), ("dot", n, m, k)


def test_long_f32_chain():
    """n = 70,001 iids x 8 SNPs: the float32 tdot sums 70,001 terms per element, within the bar of a
    16384-term chain (the 4096-iid chunks are combined in float64)."""
    rng = np.random.default_rng(3)
    n, m, k = 70001, 8, 2
    codes = random_codes(rng, n, m)
    for dtype in DTYPES:
        S = Snps(codes, dtype)
        V = (rng.standard_normal((n, k)) + 0.5).astype(dtype)  # a mean: the sums grow with n
        ref, aref = tdot_refs(S, V)
        check_bar(tdot(S, V), ref, aref, n, dtype, "tdot long %s" % dtype)
        W = operand(rng, m, k, dtype)
        ref, aref = dot_refs(S, W)
        check_bar(dot(S, W)[0], ref, aref, m, dtype, "dot long %s" % dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_pattern_is_numpys(dtype):
    """Identity with missing genotypes: NaN in the tdot row of every SNP that has one and in the dot row
    of every iid that has one -- also where the operand is zero -- and finite values elsewhere."""
    rng = np.random.default_rng(4)
    n, m, k = 1100, 300, 3
    codes = random_codes(rng, n, m, miss=0.0)
    miss_snps = rng.choice(m, size=20, replace=False)
    for s in miss_snps:
        codes[rng.choice(n, size=2, replace=False), s] = 1
    S = Snps(codes, dtype, std=IDENTITY)
    V, W = operand(rng, n, k, dtype), operand(rng, m, k, dtype)
    V[:, 1] = 0  # NaN * 0 = NaN
    W[:, 1] = 0
    G, Y = tdot(S, V), dot(S, W)[0]
    has_s, has_i = (codes == 1).any(axis=0), (codes == 1).any(axis=1)
    assert has_s.sum() == 20 and 0 < has_i.sum() < n
    assert np.array_equal(np.isnan(G), np.repeat(has_s[:, None], k, axis=1))
    assert np.array_equal(np.isnan(Y), np.repeat(has_i[:, None], k, axis=1))
    ref, aref = tdot_refs(S, V)
    check_bar(G, ref, aref, n, dtype, "tdot nan")
    ref, aref = dot_refs(S, W)
    check_bar(Y, ref, aref, m, dtype, "dot nan")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_contract_bits(dtype):
    """The same call twice: equal bits.  tdot of SNPs [a, b) = rows [a, b) of tdot of all SNPs.  dot of
    all SNPs = dot accumulated over segment-multiple chunks."""
    rng = np.random.default_rng(5)
    n, m, k = 4097, 3 * SEG + 41, 9
    S = Snps(random_codes(rng, n, m), dtype)
    V, W = operand(rng, n, k, dtype), operand(rng, m, k, dtype)
    G, Y = tdot(S, V), dot(S, W)[0]
    assert np.array_equal(G, tdot(S, V)) and np.array_equal(Y, dot(S, W)[0])
    for a, b in ((0, 1), (100, 357), (SEG, m), (m - 1, m)):
        assert np.array_equal(tdot(S, V, s0=a, cnt=b - a), G[a:b]), (a, b)
    for cuts in ((0, SEG, 2 * SEG, m), (0, 2 * SEG, m), (0, SEG, m)):
        out, Yd = dot(S, W, s0=0, cnt=cuts[1])
        for a, b in zip(cuts[1:-1], cuts[2:]):
            out, Yd = dot(S, W, s0=a, cnt=b - a, Yd=Yd)
        assert np.array_equal(out, Y), cuts


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_standardizers(dtype):
    """Unit, Beta(1, 25), UnitTrained (given stats) and count_A1 = True, each with one all-missing and
    one constant SNP, whose LUT is what snp_stats makes of them."""
    rng = np.random.default_rng(6)
    n, m, k = 1025, 70, 5
    codes = random_codes(rng, n, m)
    codes[:, 3] = 1  # all missing
    codes[:, 9] = 2  # constant
    given = np.stack([rng.uniform(0.2, 1.5, m), rng.uniform(0.3, 1.0, m)], axis=1)
    V, W = operand(rng, n, k, dtype), operand(rng, m, k, dtype)
    for label, std, a1, stats in (("unit", UNIT, 0, None), ("beta", (N.STD_BETA, 1.0, 25.0, 0), 0, None),
                                  ("unit trained", (N.STD_UNIT, 0.0, 0.0, 1), 0, given), ("count_A1", UNIT, 1, None)):
        S = Snps(codes, dtype, std=std, count_a1=a1, stats=stats)
        assert np.isfinite(S.Z).all() and (S.Z[:, 3] == 0).all() and np.abs(S.Z).max() > 0, label
        ref, aref = tdot_refs(S, V)
        check_bar(tdot(S, V), ref, aref, n, dtype, "tdot " + label)
        ref, aref = dot_refs(S, W)
        check_bar(dot(S, W)[0], ref, aref, m, dtype, "dot " + label)


def test_argument_errors_before_any_launch():
    rng = np.random.default_rng(7)
    n, m, k = 70, 5, 2
    S = Snps(random_codes(rng, n, m), F32)
    Vd, Gd = padded(operand(rng, n, k, F32), n), poisoned_out(m, k, m, F32)
    Wd, Yd = padded(operand(rng, m, k, F32), m), poisoned_out(n, k, n, F32)
    p, l = S.at(0)
    for pitch, ldv, ldg in ((S.pitch, n - 1, m), (S.pitch, n, m - 1), (S.pitch + 4, n, m), (0, n, m)):
        with pytest.raises(ValueError):
            N.call("snpmi_dev_packed_tdot", p, pitch, n, m, l, S.dt, Vd.snpmi_ptr, ldv, k, Gd.snpmi_ptr, ldg)
    for pitch, ldw, ldy in ((S.pitch, m - 1, n), (S.pitch, m, n - 1), (S.pitch + 4, m, n), (0, m, n)):
        with pytest.raises(ValueError):
            N.call("snpmi_dev_packed_dot", p, pitch, n, m, l, S.dt, Wd.snpmi_ptr, ldw, k, Yd.snpmi_ptr, ldy, 0)
    with pytest.raises(ValueError):
        N.call("snpmi_dev_packed_tdot", p, S.pitch, n, m, l, N.DT_I8, Vd.snpmi_ptr, n, k, Gd.snpmi_ptr, m)
    N.call("snpmi_stream_sync")
    assert (Gd.get().view(np.uint8) == 0xFF).all() and (Yd.get().view(np.uint8) == 0xFF).all()
    # k == 0, n == 0 and (tdot) m == 0 launch nothing
    N.call("snpmi_dev_packed_tdot", p, S.pitch, n, m, l, S.dt, Vd.snpmi_ptr, n, 0, Gd.snpmi_ptr, m)
    N.call("snpmi_dev_packed_dot", p, S.pitch, 0, m, l, S.dt, Wd.snpmi_ptr, m, k, Yd.snpmi_ptr, n, 0)
    N.call("snpmi_dev_packed_tdot", p, S.pitch, 0, m, l, S.dt, Vd.snpmi_ptr, n, k, Gd.snpmi_ptr, m)
    N.call("snpmi_dev_packed_tdot", p, S.pitch, n, 0, l, S.dt, Vd.snpmi_ptr, n, k, Gd.snpmi_ptr, m)
    N.call("snpmi_stream_sync")
    assert (Gd.get().view(np.uint8) == 0xFF).all() and (Yd.get().view(np.uint8) == 0xFF).all()


# ---------------------------------------------------------------------- the public operator
def _readers():
    from pysnptools_amd.snpreader import Bed, SnpGen

    bed = Bed(os.path.join(DATA, "n300.bed"), count_A1=False)
    gen = SnpGen(seed=5, iid_count=500, sid_count=3000)
    return [("bed", bed), ("bed iids", bed[::3, :]), ("bed strided sids", bed[:, 5:900:7]),
            ("bed reordered", bed[[250, 3, 17, 100, 4], [900, 3, 500, 7, 8, 1014, 0]]),
            ("gen", gen), ("gen iids", gen[10:400:2, :]), ("gen reordered sids", gen[:, [2999, 5, 1200, 6, 0]])]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_operator_against_numpy_and_across_modes(dtype, monkeypatch):
    """rmatmat, matmat and kernel_matmat against Z = reader.read(dtype).standardize(Unit()).val in
    float64 NumPy; resident and streamed (chunks of two segments) give equal bits; kernel_matmat is
    matmat(rmatmat(V)) bit for bit."""
    from pysnptools_amd import linop
    from pysnptools_amd.standardizer import Unit

    rng = np.random.default_rng(8)
    for label, reader in _readers():
        n, m = reader.iid_count, reader.sid_count
        Z = reader.read(dtype=dtype).standardize(Unit()).val.astype(np.float64)
        aZ = np.abs(Z)
        V, W, v1 = operand(rng, n, 3, dtype), operand(rng, m, 9, dtype), operand(rng, n, 1, dtype)[:, 0]
        res = linop.SnpOperator(reader, Unit(), dtype=dtype, resident=True)
        assert res.shape == (n, m)
        G, Y, KV, g1 = res.rmatmat(V), res.matmat(W), res.kernel_matmat(V), res.rmatmat(v1)
        assert G.shape == (m, 3) and Y.shape == (n, 9) and KV.shape == (n, 3) and g1.shape == (m,)
        assert all(isinstance(x, np.ndarray) and x.dtype == dtype for x in (G, Y, KV, g1))
        check_bar(G, Z.T @ V.astype(np.float64), aZ.T @ np.abs(V.astype(np.float64)), n, dtype, label + " rmatmat")
        check_bar(Y, Z @ W.astype(np.float64), aZ @ np.abs(W.astype(np.float64)), m, dtype, label + " matmat")
        check_bar(g1[:, None], Z.T @ v1[:, None].astype(np.float64), aZ.T @ np.abs(v1[:, None].astype(np.float64)), n,
                  dtype, label + " rmatmat 1-D")
        # K V: the second stage's bar on its own input, the G the device computed
        check_bar(KV, Z @ G.astype(np.float64), aZ @ np.abs(G.astype(np.float64)), m, dtype, label + " kernel_matmat")
        assert np.array_equal(KV, res.matmat(G))
        assert np.array_equal(res.matmat(np.ascontiguousarray(W)), res.matmat(np.asfortranarray(W)))
        # streamed: the source's pitch decides the chunk
        base_n = 300 if label.startswith("bed") else 500
        monkeypatch.setattr(linop, "MATVEC_CHUNK_BYTES", 2 * linop.SEGMENT * int(N.lib().snpmi_packed_pitch(base_n)))
        stream = linop.SnpOperator(reader, Unit(), dtype=dtype, resident=False)
        if m > 2 * linop.SEGMENT:
            assert len(list(stream._chunks())) == -(-m // (2 * linop.SEGMENT)) > 1
        assert np.array_equal(stream.rmatmat(V), G), label
        assert np.array_equal(stream.matmat(W), Y), label
        assert np.array_equal(stream.kernel_matmat(V), KV), label
        assert np.array_equal(stream.trained.stats, res.trained.stats, equal_nan=True), label
        monkeypatch.undo()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_operator_hbm_and_trained(dtype):
    """HbmArray in, HbmArray out (any order, 1-D too), with the bits of the NumPy route; the trained
    standardizer is read_kernel's."""
    from pysnptools_amd import hbm as H
    from pysnptools_amd import SnpOperator
    from pysnptools_amd.snpreader import Bed
    from pysnptools_amd.standardizer import Beta, Unit, UnitTrained

    rng = np.random.default_rng(9)
    bed = Bed(os.path.join(DATA, "n300.bed"), count_A1=False)
    reader = bed[5:290, 10:700]
    n, m = reader.iid_count, reader.sid_count
    op = SnpOperator(reader, Unit(), dtype=dtype)
    V, v1 = operand(rng, n, 4, dtype), operand(rng, n, 1, dtype)[:, 0]
    G = op.rmatmat(V)
    for dev in (H.asarray(np.ascontiguousarray(V)), H.asarray(np.asfortranarray(V))):
        Gd = op.rmatmat(dev)
        assert isinstance(Gd, H.HbmArray) and Gd.shape == (m, 4) and np.array_equal(Gd.get(), G)
        Kd = op.kernel_matmat(dev)
        assert isinstance(Kd, H.HbmArray) and np.array_equal(Kd.get(), op.kernel_matmat(V))
    g1 = op.rmatmat(H.asarray(v1))
    assert isinstance(g1, H.HbmArray) and g1.shape == (m,) and np.array_equal(g1.get(), op.rmatmat(v1))
    out = SnpOperator(reader, Unit(), dtype=dtype, xp="hbm").matmat(G)
    assert isinstance(out, H.HbmArray) and np.array_equal(out.get(), op.matmat(G))
    _, trained = reader._read_kernel(Unit(), dtype=dtype, return_trained=True)
    assert isinstance(op.trained, UnitTrained) and np.array_equal(op.trained.stats, trained.stats)
    # a trained standardizer passes its stats: the operator of the trained form equals Z of those stats
    again = SnpOperator(reader, trained, dtype=dtype)
    assert again.trained is trained
    Z = reader.read(dtype=dtype).standardize(trained).val.astype(np.float64)
    check_bar(again.rmatmat(V), Z.T @ V.astype(np.float64), np.abs(Z).T @ np.abs(V.astype(np.float64)), n, dtype,
              "trained rmatmat")
    Zb = reader.read(dtype=dtype).standardize(Beta(1, 25)).val.astype(np.float64)
    check_bar(SnpOperator(reader, Beta(1, 25), dtype=dtype).rmatmat(V), Zb.T @ V.astype(np.float64),
              np.abs(Zb).T @ np.abs(V.astype(np.float64)), n, dtype, "beta rmatmat")
