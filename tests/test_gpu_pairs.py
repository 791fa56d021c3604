"""SNP-pair values and their scan from packed codes (csrc/pairs.hip, include/snpmi.h
snpmi_dev_pair_values / snpmi_dev_pair_tdot, pysnptools_amd.snpreader.Pairs).

Harness: that of test_gpu_matvec.py -- codes packed on the host with the unused codes of the last byte
set to the missing code and the pad bytes 0xFF, tables read back from snpmi_dev_snp_stats, outputs
pre-filled with 0xFF bytes whose padding must keep them.

Ground truth.  pair_values: the host product in dtype of the two table entries, bit for bit (integer
views equal, NaN positions equal).  pair_tdot: Zp rebuilt on the host (that product, widened) and
NumPy's float64 Zp^T V, within the bars of test_gpu_matvec.check_bar with t = n; exact data must match
bit for bit.

Codes: the first 64 iids of SNP s hold <v_s, i> over GF(4), i running over GF(4)^3 and v_s over the
21 points of its projective plane, so every two distinct SNPs show each of the 16 code combinations
(four times) in every column of n >= 64; the other iids are random with 3% missing.

Shapes.  The kernels' constants (pairs.hip): a lane holds 16 iids (kLaneIids), a wave 1024 (kSpan), a
tdot workgroup 4096 per chunk (kChunk); a tdot tile is kPairTA x kPairTB = 8 x 32 SNPs; a panel is 4
(f32) or 2 (f64) columns, narrower ones 2 / 1; the values kernel takes 4 (pair, span) items per wave.
"""
import os

import numpy as np
import pytest

from conftest import DATA
from pysnptools_amd import _native as N
from test_gpu_matvec import (F32, F64, IDENTITY, UNIT, Snps, check_bar, hbm, operand, padded, poisoned_out,
                             random_codes, unpadded)

pytestmark = pytest.mark.gpu

DTYPES = [F32, F64]
IDS = ["f32", "f64"]
TA, TB = 8, 32  # kPairTA, kPairTB
NS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]  # + each span +- 1
PAIR_COUNTS = [1, 2, 7, 64, 65, 300]
SIDES = [1, 2, 7, 8, 9, TA - 1, TA + 1, 2 * TA + 1, TB - 1, TB + 1, 2 * TB + 1]
KS = [1, 2, 3, 4, 5, 8, 9, 12, 15, 17]

_GF4_MUL = np.array([[0, 0, 0, 0], [0, 1, 2, 3], [0, 2, 3, 1], [0, 3, 1, 2]], dtype=np.uint8)
_POINTS = ([(1, a, b) for a in range(4) for b in range(4)] + [(0, 1, a) for a in range(4)] + [(0, 0, 1)])  # 21


def design_codes(rng, n, m, miss=0.03):
    """[n][m] codes, m <= 21: the GF(4) design on the first 64 iids (n >= 64), random elsewhere."""
    assert m <= len(_POINTS)
    codes = random_codes(rng, n, m, miss=miss)
    if n >= 64:
        i = np.arange(64)
        x = np.stack([i & 3, (i >> 2) & 3, i >> 4], axis=1)
        for s in range(m):
            v = _POINTS[s]
            codes[:64, s] = _GF4_MUL[v[0], x[:, 0]] ^ _GF4_MUL[v[1], x[:, 1]] ^ _GF4_MUL[v[2], x[:, 2]]
        for a in range(m):  # the design's claim, checked where it is made
            for b in range(a + 1, m):
                assert (np.bincount(4 * codes[:64, a].astype(int) + codes[:64, b], minlength=16) == 4).all(), (a, b)
    return codes


class Wide(Snps):
    """The same packed SNPs at a wider pitch (64 more pad bytes of 0xFF per column)."""

    def __init__(self, codes, dtype, std=UNIT, count_a1=0):
        Snps.__init__(self, codes, dtype, std=std, count_a1=count_a1)
        host = self.packed.get()
        self.pitch += 64
        wide = np.full((host.shape[0], self.pitch), 0xFF, dtype=np.uint8)
        wide[:, :host.shape[1]] = host
        self.packed = hbm().asarray(wide)


def table_values(S, idx):
    """[n][len(idx)] of S.dtype: the table entry of every genotype of SNPs idx."""
    return S.lut[idx[None, :], S.codes[:, idx]]


def make(codes, dtype, std, cls=Snps):
    S = cls(codes, dtype, std=std)
    S.codes = codes
    return S


def same_bits(out, ref, label):
    assert out.dtype == ref.dtype and out.shape == ref.shape, label
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan), (label, "NaN positions differ")
    view = np.uint32 if out.dtype == F32 else np.uint64
    assert np.array_equal(out.view(view)[~nan], ref.view(view)[~nan]), label


def dev_u32(a):
    return hbm().asarray(np.ascontiguousarray(a, dtype=np.uint32))


def pair_values(S0, S1, idx0, idx1, order_c):
    n, count, dtype = S0.n, len(idx0), S0.dtype
    i0, i1 = dev_u32(idx0), dev_u32(idx1)
    if order_c:
        rows, k, ld = count, n, count + 3  # [n][ld]: "column" = iid in the helpers' terms
    else:
        rows, k, ld = n, count, (n + 15) // 16 * 16 + 16
    out = poisoned_out(rows, k, ld, dtype)
    N.call("snpmi_dev_pair_values", S0.packed.snpmi_ptr, S0.pitch, S0.lut_dev.snpmi_ptr, S1.packed.snpmi_ptr, S1.pitch,
           S1.lut_dev.snpmi_ptr, n, i0.snpmi_ptr, i1.snpmi_ptr, count, S0.dt, int(order_c), out.snpmi_ptr, ld)
    N.call("snpmi_stream_sync")
    got = unpadded(out, rows, k, ld)  # [rows][k]; the padding is checked
    return got.T if order_c else got  # [n][count]


def pair_list(rng, count, m0, m1, kind):
    if kind == "descending":
        return (np.sort(rng.integers(0, m0, count))[::-1].copy(), np.sort(rng.integers(0, m1, count))[::-1].copy())
    idx0, idx1 = rng.integers(0, m0, count), rng.integers(0, m1, count)
    if kind == "squares":  # same buffers: every third pair a square, and repeats of the first pair
        idx1[::3] = idx0[::3]
        idx0[1::5], idx1[1::5] = idx0[0], idx1[0]
    return idx0, idx1


# ---------------------------------------------------------------------- pair_values
@pytest.mark.parametrize("std", [UNIT, IDENTITY], ids=["unit", "identity"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_values_bit_for_bit(dtype, std):
    rng = np.random.default_rng(11)
    for n in NS:
        A = make(design_codes(rng, n, 21), dtype, std)
        B = make(design_codes(rng, n, 21)[:, ::-1][:, :11].copy(), dtype, std, cls=Wide)
        assert B.pitch != A.pitch
        if n >= 64:  # missing genotypes in every column: zeros under Unit, NaN under Identity
            assert (A.codes == 1).any(axis=0).all() and np.isnan(A.lut).any() == (std is IDENTITY)
        for q, count in enumerate(PAIR_COUNTS):
            for order_c in (0, 1):
                kind = ("squares", "descending", "plain")[(q + order_c) % 3]
                two = (q + order_c) % 2 == 1
                S1 = B if two else A
                # (two buffers: B holds design points 20 ... 10, so side 0 keeps to points 0 ... 9)
                idx0, idx1 = pair_list(rng, count, 10 if two else A.m, S1.m,
                                       "plain" if two and kind == "squares" else kind)
                with np.errstate(invalid="ignore"):
                    ref = table_values(A, idx0) * table_values(S1, idx1)  # one multiply in dtype
                assert ref.dtype == dtype
                same_bits(pair_values(A, S1, idx0, idx1, order_c), ref, (n, count, order_c, kind, two))


def test_pair_values_argument_errors_before_any_launch():
    rng = np.random.default_rng(12)
    n, count = 300, 5
    A = make(design_codes(rng, n, 6), F32, UNIT)
    idx = dev_u32(np.arange(count))
    ld_f = 304
    out = poisoned_out(n, count, ld_f, F32)

    def call(pitch0=A.pitch, pitch1=A.pitch, dt=A.dt, order_c=0, ld=ld_f, nn=n, cnt=count):
        N.call("snpmi_dev_pair_values", A.packed.snpmi_ptr, pitch0, A.lut_dev.snpmi_ptr, A.packed.snpmi_ptr, pitch1,
               A.lut_dev.snpmi_ptr, nn, idx.snpmi_ptr, idx.snpmi_ptr, cnt, dt, order_c, out.snpmi_ptr, ld)

    for bad in (dict(ld=n - 12), dict(ld=288), dict(ld=n), dict(ld=n + 1), dict(order_c=1, ld=count - 1),
                dict(pitch0=A.pitch + 4), dict(pitch1=A.pitch + 32), dict(pitch0=64), dict(pitch1=0),
                dict(dt=N.DT_I8), dict(dt=7)):
        with pytest.raises(ValueError):
            call(**bad)
    call(nn=0)  # nothing launched
    call(cnt=0)
    N.call("snpmi_stream_sync")
    assert (out.get().view(np.uint8) == 0xFF).all()
    call()
    N.call("snpmi_stream_sync")
    assert not np.isnan(unpadded(out, n, count, ld_f)).any()


# ---------------------------------------------------------------------- pair_tdot
def zp_of(A, B, a_idx, b_idx):
    """Zp [n][len(a_idx) * len(b_idx)] in float64: the product rounded in dtype, then widened."""
    with np.errstate(invalid="ignore"):
        za, zb = table_values(A, a_idx), table_values(B, b_idx)
        return (za[:, :, None] * zb[:, None, :]).reshape(A.n, -1).astype(np.float64)


def pair_tdot(A, a0, na, B, b0, nb, V, rows=None, row_off=None, b_lo=None, pad=(3, 5)):
    """The rectangle A[a0 : a0 + na] x B[b0 : b0 + nb]; G has ``rows`` rows (default na nb)."""
    rows = na * nb if rows is None else rows
    k, ldv, ldg = V.shape[1], A.n + pad[0], rows + pad[1]
    Vd, Gd = padded(V, ldv), poisoned_out(rows, k, ldg, A.dtype)
    ro = None if row_off is None else hbm().asarray(np.ascontiguousarray(row_off, dtype=np.int64))
    lo = None if b_lo is None else dev_u32(b_lo)
    pa, la = A.at(a0)
    pb, lb = B.at(b0)
    N.call("snpmi_dev_pair_tdot", pa, A.pitch, la, na, pb, B.pitch, lb, nb, A.n, N.ptr(ro), N.ptr(lo), A.dt,
           Vd.snpmi_ptr, ldv, k, Gd.snpmi_ptr, ldg)
    N.call("snpmi_stream_sync")
    buf = Gd.get()
    assert (buf[:k, rows:].view(np.uint8) == 0xFF).all(), "output padding was written"
    return np.ascontiguousarray(buf[:k, :rows].T)


def tdot_shapes():
    shapes = []
    for q, n in enumerate(NS):
        na, nb = SIDES[q % len(SIDES)], SIDES[(3 * q + 4) % len(SIDES)]
        shapes.append((n, na, nb, KS[q % len(KS)]))
    # every side length on either side, every k
    shapes += [(300, s, SIDES[-1 - q], KS[(q + 5) % len(KS)]) for q, s in enumerate(SIDES)]
    return shapes


def wide_codes(rng, n, m, miss):
    return random_codes(rng, n, m, miss=miss)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_tdot_shapes_within_bar(dtype):
    """Unit tables on codes with 3% missing, two buffers of different pitch, padded V and G."""
    rng = np.random.default_rng(13)
    seen_a, seen_b, seen_k = set(), set(), set()
    for n, na, nb, k in tdot_shapes():
        A = make(wide_codes(rng, n, na, 0.03), dtype, UNIT)
        B = make(wide_codes(rng, n, nb, 0.03), dtype, UNIT, cls=Wide)
        V = operand(rng, n, k, dtype)
        Zp = zp_of(A, B, np.arange(na), np.arange(nb))
        V64 = V.astype(np.float64)
        check_bar(pair_tdot(A, 0, na, B, 0, nb, V), Zp.T @ V64, np.abs(Zp).T @ np.abs(V64), n, dtype,
                  "pair_tdot %s" % ((n, na, nb, k),))
        seen_a.add(na), seen_b.add(nb), seen_k.add(k)
    assert seen_a == seen_b == set(SIDES) and seen_k == set(KS)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_tdot_exact_data(dtype):
    """Identity tables, no missing genotype, V integer in [-8, 8], n <= 4097: every partial sum is an
    integer below 2^24 (4097 x 4 x 8), so the result is the integer product bit for bit -- with the unused
    codes of the last byte and the pad bytes poisoned, so an iid >= n that is added shows as NaN."""
    rng = np.random.default_rng(14)
    for n, na, nb, k in tdot_shapes():
        A = make(wide_codes(rng, n, na, 0.0), dtype, IDENTITY)
        B = make(wide_codes(rng, n, nb, 0.0), dtype, IDENTITY, cls=Wide)
        V = rng.integers(-8, 9, size=(n, k)).astype(dtype)
        Zp = zp_of(A, B, np.arange(na), np.arange(nb))
        assert np.isfinite(Zp).all()
        assert np.array_equal(pair_tdot(A, 0, na, B, 0, nb, V), (Zp.T @ V.astype(np.float64)).astype(dtype)), (n, na, nb, k)


@pytest.mark.parametrize("singles", [False, True], ids=["pairs", "singles"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_tdot_triangular_tables(dtype, singles):
    """One buffer on both sides with the reader's row_off / b_lo: the whole triangle in pair order, and
    one rectangle of it -- every row no pair maps to keeps its 0xFF bytes."""
    from pysnptools_amd.snpreader.pairs import block_tables, pair_count, pair_to_ij

    rng = np.random.default_rng(15)
    n, m, k = 1030, 2 * TB + 5, 3
    S = make(wide_codes(rng, n, m, 0.03), dtype, UNIT)
    V = operand(rng, n, k, dtype)
    V64 = V.astype(np.float64)
    count = pair_count(m, None, singles)
    i, j = pair_to_ij(np.arange(count), m, None, singles)
    with np.errstate(invalid="ignore"):
        Zp = (table_values(S, i) * table_values(S, j)).astype(np.float64)
    ref, aref = Zp.T @ V64, np.abs(Zp).T @ np.abs(V64)
    row_off, b_lo = block_tables(0, m, 0, m, m, None, singles)
    whole = pair_tdot(S, 0, m, S, 0, m, V, rows=count, row_off=row_off, b_lo=b_lo)
    check_bar(whole, ref, aref, n, dtype, "triangle")
    for a0, a1, b0, b1 in ((0, 20, 10, m), (TB, TB + 9, TB, TB + 9), (3, 12, 0, 7)):
        row_off, b_lo = block_tables(a0, a1, b0, b1, m, None, singles)
        got = pair_tdot(S, a0, a1 - a0, S, b0, b1 - b0, V, rows=count, row_off=row_off, b_lo=b_lo)
        mine = (i >= a0) & (i < a1) & (j >= b0) & (j < b1)
        assert (got[~mine].view(np.uint8) == 0xFF).all(), "a row no pair of the rectangle maps to was written"
        assert mine.any() and np.array_equal(got[mine], whole[mine]), "a pair's row depends on its rectangle"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_tdot_independence_and_determinism(dtype):
    """One pair as part of different rectangles, at different places of the tile: identical bits; the
    same call twice: identical bits."""
    rng = np.random.default_rng(16)
    n, k = 4097 + 70, 5
    A = make(wide_codes(rng, n, 20, 0.03), dtype, UNIT)
    B = make(wide_codes(rng, n, 70, 0.03), dtype, UNIT, cls=Wide)
    V = operand(rng, n, k, dtype)
    big = pair_tdot(A, 0, 20, B, 0, 70, V)
    assert np.array_equal(big, pair_tdot(A, 0, 20, B, 0, 70, V))
    for a0, na, b0, nb in ((5, 1, 40, 1), (3, 9, 33, 37), (0, 6, 39, 2), (5, 15, 0, 41)):
        part = pair_tdot(A, a0, na, B, b0, nb, V)
        rows = (np.arange(a0, a0 + na)[:, None] * 70 + np.arange(b0, b0 + nb)[None, :]).ravel()
        assert np.array_equal(part, big[rows]), (a0, na, b0, nb)
    # k in panels: column c does not depend on its panel
    assert np.array_equal(pair_tdot(A, 0, 20, B, 0, 70, V[:, 1:2])[:, 0], big[:, 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_tdot_nan_rows(dtype):
    """Identity tables: a missing genotype makes exactly the rows of that SNP's pairs NaN, also where V
    is zero."""
    rng = np.random.default_rng(17)
    n, na, nb, k = 1100, 12, 40, 3
    ca, cb = wide_codes(rng, n, na, 0.0), wide_codes(rng, n, nb, 0.0)
    ca[rng.choice(n, 2, replace=False), 4] = 1
    cb[rng.choice(n, 2, replace=False), 33] = 1
    cb[n - 1, 7] = 1
    A, B = make(ca, dtype, IDENTITY), make(cb, dtype, IDENTITY, cls=Wide)
    V = operand(rng, n, k, dtype)
    V[:, 1] = 0  # NaN * 0 = NaN
    G = pair_tdot(A, 0, na, B, 0, nb, V)
    bad = np.zeros((na, nb), dtype=bool)
    bad[4, :] = True
    bad[:, [7, 33]] = True
    assert np.array_equal(np.isnan(G), np.repeat(bad.ravel()[:, None], k, axis=1))
    Zp = zp_of(A, B, np.arange(na), np.arange(nb))
    V64 = V.astype(np.float64)
    with np.errstate(invalid="ignore"):
        check_bar(G, Zp.T @ V64, np.abs(Zp).T @ np.abs(V64), n, dtype, "pair_tdot nan")


def test_pair_tdot_argument_errors_and_empty_shapes():
    rng = np.random.default_rng(18)
    n, na, nb, k = 70, 3, 5, 2
    A = make(wide_codes(rng, n, na, 0.03), F32, UNIT)
    B = make(wide_codes(rng, n, nb, 0.03), F32, UNIT)
    Vd, Gd = padded(operand(rng, n, k, F32), n), poisoned_out(na * nb, k, na * nb, F32)

    def call(pitch_a=A.pitch, pitch_b=B.pitch, dt=A.dt, ldv=n, ldg=na * nb, nn=n, a=na, b=nb, kk=k):
        N.call("snpmi_dev_pair_tdot", A.packed.snpmi_ptr, pitch_a, A.lut_dev.snpmi_ptr, a, B.packed.snpmi_ptr, pitch_b,
               B.lut_dev.snpmi_ptr, b, nn, None, None, dt, Vd.snpmi_ptr, ldv, kk, Gd.snpmi_ptr, ldg)

    for bad in (dict(ldv=n - 1), dict(ldg=na * nb - 1), dict(pitch_a=A.pitch + 4), dict(pitch_b=0), dict(dt=N.DT_I8)):
        with pytest.raises(ValueError):
            call(**bad)
    call(a=0)
    call(b=0)
    call(kk=0)
    N.call("snpmi_stream_sync")
    assert (Gd.get().view(np.uint8) == 0xFF).all()
    call(nn=0)  # an empty sum: zeros in the rows the call owns
    N.call("snpmi_stream_sync")
    assert not Gd.get().any()


# ---------------------------------------------------------------------- the reader
def _bed(count_a1=False):
    from pysnptools_amd.snpreader import Bed

    return Bed(os.path.join(DATA, "n300.bed"), count_A1=count_a1)


def _gen():
    from pysnptools_amd.snpreader import SnpGen

    return SnpGen(seed=332, iid_count=257, sid_count=40)


def _products(Z, pairs, idx=None):
    """The columns of Z multiplied in the order of the pairs' sids."""
    from pysnptools_amd.snpreader.pairs import pair_to_ij

    idx = np.arange(pairs.sid_count) if idx is None else np.asarray(idx)
    i, j = pair_to_ij(idx, *pairs._counts)
    with np.errstate(invalid="ignore"):
        return Z[0][:, i] * Z[1][:, j]


def _unit(reader, dtype):
    from pysnptools_amd.standardizer import Unit

    return reader.read(dtype=dtype).standardize(Unit()).val


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reader_values_bit_for_bit(dtype):
    from pysnptools_amd import hbm as H
    from pysnptools_amd.snpreader import Pairs

    for source in (_bed(), _gen()):
        inner = source[:, :12]
        Z = _unit(inner, dtype)
        pairs = Pairs(inner)
        assert pairs.sid_count == 66 and pairs.sid[13] == "%s,%s" % (inner.sid[1], inner.sid[4])
        for order in "FCA":
            val = pairs.read(dtype=dtype, order=order).val
            assert val.flags["C_CONTIGUOUS" if order == "C" else "F_CONTIGUOUS"]
            same_bits(np.ascontiguousarray(val), np.ascontiguousarray(_products((Z, Z), pairs)), ("whole", order))
        dev = pairs.read(dtype=dtype, xp="hbm").val
        assert isinstance(dev, H.HbmArray) and dev.order == "F"
        same_bits(np.ascontiguousarray(dev.get()), np.ascontiguousarray(_products((Z, Z), pairs)), "hbm")
        # a subset: Unit trains on the selected iids
        n = source.iid_count
        for rows in (slice(None, None, -3), np.arange(n) % 3 == 1):
            sub = pairs[rows, [5, 2, 2, 40]]
            Zs = _unit(inner[rows, :], dtype)
            same_bits(np.ascontiguousarray(sub.read(dtype=dtype).val),
                      np.ascontiguousarray(_products((Zs, Zs), pairs, [5, 2, 2, 40])), "subset")
            same_bits(np.ascontiguousarray(sub.read(dtype=dtype, xp="hbm", order="C").val.get()),
                      np.ascontiguousarray(_products((Zs, Zs), pairs, [5, 2, 2, 40])), "subset hbm")
        # singles
        both = Pairs(inner, _include_single_times_single=True)
        assert both.sid_count == 78
        same_bits(np.ascontiguousarray(both.read(dtype=dtype).val), np.ascontiguousarray(_products((Z, Z), both)),
                  "singles")
        # two readers
        r0, r1 = source[:, :5], source[:, 20:27]
        two = Pairs(r0, r1)
        assert two.sid_count == 35 and two.sid[8] == "%s,%s" % (r0.sid[1], r1.sid[1])
        Z0, Z1 = _unit(r0, dtype), _unit(r1, dtype)
        same_bits(np.ascontiguousarray(two.read(dtype=dtype).val), np.ascontiguousarray(_products((Z0, Z1), two)), "two")
        same_bits(np.ascontiguousarray(two[::2, ::-4].read(dtype=dtype, order="C").val),
                  np.ascontiguousarray(_products((_unit(r0[::2, :], dtype), _unit(r1[::2, :], dtype)), two,
                                                 np.arange(35)[::-4])), "two subset")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reader_without_standardization(dtype):
    """do_standardize=False: the raw values with NaN for a missing genotype, a Bed's count_A1 honoured.
    n300.bed has no missing genotype, so this runs on dist_x.bed (100 x 100, 2182 missing) as well."""
    from pysnptools_amd.snpreader import Bed, Pairs

    for name, want_nan in (("dist_x.bed", True), ("n300.bed", False)):
        vals = []
        for count_a1 in (True, False):
            bed = Bed(os.path.join(DATA, name), count_A1=count_a1)
            Z = bed[:, :9].read(dtype=dtype).val
            assert np.isnan(Z).any() == want_nan
            pairs = Pairs(bed[:, :9], do_standardize=False)
            val = pairs.read(dtype=dtype).val
            assert np.isnan(val).any() == want_nan
            same_bits(np.ascontiguousarray(val), np.ascontiguousarray(_products((Z, Z), pairs)), (name, count_a1))
            sub = pairs[5:90:2, [30, 1, 1]].read(dtype=dtype, order="C").val
            same_bits(np.ascontiguousarray(sub), np.ascontiguousarray(_products((Z[5:90:2], Z[5:90:2]), pairs, [30, 1, 1])),
                      (name, count_a1, "subset"))
            vals.append(val)
        assert not np.array_equal(vals[0], vals[1], equal_nan=True)


def _scan_ref(pairs, V, dtype):
    Zp = pairs.read(dtype=dtype).val.astype(np.float64)
    V64 = np.asarray(V, dtype=np.float64).reshape(len(Zp), -1)
    return Zp.T @ V64, np.abs(Zp).T @ np.abs(V64)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reader_rmatmat(dtype, monkeypatch):
    from pysnptools_amd import hbm as H
    from pysnptools_amd.snpreader import Pairs
    from pysnptools_amd.snpreader import pairs as module

    rng = np.random.default_rng(19)
    for source in (_bed(), _gen()):
        n = source.iid_count
        V, v1 = operand(rng, n, 5, dtype), operand(rng, n, 1, dtype)[:, 0]
        for label, build in (("one", lambda: Pairs(source[:, :12])),
                             ("singles", lambda: Pairs(source[:, :12], _include_single_times_single=True)),
                             ("two", lambda: Pairs(source[:, :12], source[:, 20:27]))):
            pairs = build()
            ref, aref = _scan_ref(pairs, V, dtype)
            G = pairs.rmatmat(V)
            assert isinstance(G, np.ndarray) and G.shape == (pairs.sid_count, 5) and G.dtype == dtype
            check_bar(G, ref, aref, n, dtype, label + " rmatmat")
            g1 = pairs.rmatmat(v1)
            assert g1.shape == (pairs.sid_count,)
            ref1, aref1 = _scan_ref(pairs, v1, dtype)
            check_bar(g1[:, None], ref1, aref1, n, dtype, label + " rmatmat 1-D")
            for dev in (H.asarray(np.ascontiguousarray(V)), H.asarray(np.asfortranarray(V))):
                Gd = pairs.rmatmat(dev)
                assert isinstance(Gd, H.HbmArray) and Gd.shape == G.shape and np.array_equal(Gd.get(), G)
            gd = pairs.rmatmat(H.asarray(v1))
            assert isinstance(gd, H.HbmArray) and gd.shape == g1.shape and np.array_equal(gd.get(), g1)
            # blocks of 5 SNPs: diagonal, off-diagonal and ragged last blocks at M = 12 -- the same bits
            monkeypatch.setattr(module, "PAIR_BLOCK", 5)
            assert np.array_equal(build().rmatmat(V), G), label
            monkeypatch.undo()
            # beyond the limit the scan still works
            small = build()
            small.sid_materialize_limit = 10
            assert np.array_equal(small.rmatmat(V), G)
            with pytest.raises(AssertionError, match="too many sids"):
                small.sid
        limited = Pairs(source[:, :12], sid_materialize_limit=10)
        assert limited.rmatmat(v1).shape == (66,)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reader_read_kernel(dtype, monkeypatch):
    """The GRM of the pairs against the dense route on the same values; bars of test_gpu_snpgen.py:
    1e-5 (f32) / 1e-10 (f64) of max diag."""
    from pysnptools_amd import _grm as G
    from pysnptools_amd.kernelreader import SnpKernel
    from pysnptools_amd.snpreader import Pairs, SnpData
    from pysnptools_amd.standardizer import Unit

    tol = 1e-5 if dtype == F32 else 1e-10
    inner = _bed()[:, :12]
    pairs = Pairs(inner)
    dense = SnpData(iid=pairs.iid, sid=pairs.sid, val=pairs.read(dtype=dtype).val)
    K_ref, trained_ref = dense._read_kernel(Unit(), dtype=dtype, return_trained=True)
    bar = tol * np.abs(np.diag(K_ref)).max()
    fed = []
    real = G.Session.add_dense
    monkeypatch.setattr(G.Session, "add_dense", lambda self, val: (fed.append(val.shape), real(self, val))[1])
    K = pairs.read_kernel(Unit(), dtype=dtype).val
    assert fed == [(300, 66)] and K.dtype == dtype and K.shape == (300, 300)
    print("read_kernel max error / bar %.3e" % (np.abs(K - K_ref).max() / bar))
    assert np.abs(K - K_ref).max() <= bar
    del fed[:]
    monkeypatch.setattr(G, "PAIRS_CHUNK_BYTES", 17 * 300 * dtype.itemsize)
    K4, trained = Pairs(inner)._read_kernel(Unit(), dtype=dtype, return_trained=True)
    assert fed == [(300, 17)] * 3 + [(300, 15)]
    assert np.abs(K4 - K_ref).max() <= bar
    assert np.array_equal(trained.stats, trained_ref.stats, equal_nan=True)
    assert np.array_equal(trained.sid, pairs.sid)
    rows, cols = [3, 299, 17], [0, 5, 250, 251]
    rect = SnpKernel(pairs, Unit())[rows, cols].read(dtype=dtype).val
    assert np.abs(rect - K_ref[np.ix_(rows, cols)]).max() <= bar
    # a pair subset takes the same feeder, an iid subset the generic block loop
    sub = pairs[:, 5:40].read_kernel(Unit(), dtype=dtype).val
    sub_ref = SnpData(iid=pairs.iid, sid=pairs.sid[5:40], val=dense.val[:, 5:40].copy()).read_kernel(Unit(), dtype=dtype).val
    assert np.abs(sub - sub_ref).max() <= bar
    half = pairs[::2, :]
    half_ref = SnpData(iid=half.iid, sid=half.sid, val=half.read(dtype=dtype).val).read_kernel(Unit(), dtype=dtype).val
    assert np.abs(half.read_kernel(Unit(), dtype=dtype).val - half_ref).max() <= tol * np.abs(np.diag(half_ref)).max()
