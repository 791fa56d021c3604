"""The dense-operand GRM kernels, K = Z Z^T of a float matrix already in HBM, at the block, stage and
range edges that the one shape of test_gpu_parity.test_grm_dense_h2_range (4200 x 45) does not reach:

  k_split_h2<false> -> k_image_h2 -> k_syrk_h2<false, 6, true>   f32, n >= 4096, every column's
                                                                 max |z| in [2^-2, 2^15) ("fp16x2")
  k_syrk256d                  its fallback on the range flag, and all of hook syrk = 20 ("fallback")
  f32k::k_syrk<false>         f32, n < 4096
  f64k::k_syrk_glds           f64

Every launch goes through the C-ABI entry snpmi_dev_syrk_dense (_dense below): the test owns the
operand's leading dimension, its pad rows, `accumulate` and what the tiles hold beforehand (0xFF
bytes = NaN, so an element a kernel leaves unwritten fails every comparison).

Data and bars.  Reference everywhere: Z.astype(f64) @ Z.astype(f64).T (NumPy), per (kind, n, m, seed).
  exact   every value k / 8, |k| <= 32, 5% zeros, a 2.0 in each column.  Exact in fp16 (the second
          fp16 plane is 0); every product is a multiple of 2^-6 and every partial sum over m <= 1024
          SNPs stays below 2^14, so each is exact in f32 and f64 in any order.  Bar: the bits of the
          reference, for every kernel.  A dropped, doubled or misplaced term of any size fails.
  normal  seeded standard normal, 1% zeros (f32 values for f32, f64 values for f64).  f32 bar: max
          |K - ref| / max diag(ref) <= 2e-6, the bar of test_grm_dense_h2_range (without the second
          fp16 plane the error is ~5e-4).  f64 bar, elementwise: |K - ref|_ij <= 2 (m + 1) 2^-53
          (|Z| |Z|^T)_ij -- K and NumPy's product each lie within gamma_m = m u / (1 - m u) of the
          exact sum, whatever their order of summation.
Scaling the data by 2^-10 is exact and puts every column's max below 2^-2: the range flag is raised
and the fallback computes the same K times 2^-20.

Path witness.  Hook syrk = 20 runs k_syrk256d alone, with the same segmentation.  A launch that must
fall back gives its bits; a launch that must stay on fp16x2 differs from it somewhere on normal data
(and meets the bar).

A  block edges of the n >= 4096 tier, m = 33: n = 4096 (no pad), 4097 (a one-row last block), 4351,
   4352 (17 blocks: the second supertile column starts), 4353 (18 blocks); both paths, both data.
B  SNP counts around the 16-SNP step and the 32-SNP stage, 1 ... 65: n = 4097 on both paths, n = 257
   on the small f32 kernel and the f64 kernel; m = 0 with and without `accumulate`.
C  stage-image chunks of 32 SNPs (hook dense_chunk) and two accumulating calls, the second one on
   the other path.
D  the range flag's bounds, to the ulp; an all-zero column; one NaN value.
E  leading dimensions beyond round_up(n, 256) (the block-order table once followed ldz, not n) and
   pad rows of NaN / 1e30, through the entry and through the scratch of snpmi_grm_dense_f32.
F  64-SNP accumulation segments (hook seg): SegFlush inside k_syrk_h2 MODE 6, for_segments around
   k_syrk256d.
G  a C-order device operand through the session (k_transpose).
"""
import functools
import time

import numpy as np
import pytest

from conftest import DATA  # noqa: F401  (sys.path)
import bench
from pysnptools_amd import _native as N
from test_gpu_rect_edges import hooks as hooked

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BAR32 = 2e-6
DOWN = np.float32(2.0 ** -10)  # exact; 4 * 2^-10 and 6 sigma * 2^-10 are far below 2^-2
WORST = {}  # (group, what) -> the largest error seen, printed when the module is done
T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (group, what), e in sorted(WORST.items()):
        print("worst error, group %s, %s: %.3e" % (group, what, e))
    print("test_gpu_dense_edges: %.1f s since import" % (time.perf_counter() - T0))


def round_up(x, q):
    return -(-x // q) * q


# ------------------------------------------------------------------- data and references
def exact_data(n, m, seed, dtype=F32):
    rng = np.random.default_rng(seed)
    k = rng.integers(-32, 33, size=(n, m))
    k[rng.random((n, m)) < 0.05] = 0
    k[rng.integers(0, n, size=m), np.arange(m)] = 16  # max |z| >= 2^-2 in every column
    return (k / 8.0).astype(dtype)


def normal_data(n, m, seed, dtype=F32):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, m)).astype(dtype)
    v[rng.random((n, m)) < 0.01] = 0
    return v


def product(Z):
    z = Z.astype(np.float64)
    return z @ z.T


@functools.lru_cache(maxsize=4)
def reference(kind, n, m, seed, dtype=F32):
    """(Z [n, m], its f64 product), computed once and left unchanged.  The cache is small: a
    4353^2 product is 150 MB, and the tests that share one run next to each other."""
    Z = (exact_data if kind == "exact" else normal_data)(n, m, seed, np.dtype(dtype))
    ref = product(Z)
    if kind == "exact" and m:
        # what the bit-equality bar rests on: not a genotype-valued operand (k_dense_codes would
        # divert it to the packed kernels), the range, and a product that f32 holds exactly
        assert min(len(np.unique(Z[:, s])) for s in range(m)) > 4
        assert np.abs(Z).max(axis=0).min() >= 0.25 and np.abs(Z).max() <= 4
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    Z.flags.writeable = False
    ref.flags.writeable = False
    return Z, ref


# ------------------------------------------------------------------- the launch
def _dense(Z, n, dtype, *, ldz=None, pad=None, accumulate=0, poison=True, hooks={}, tiles=None):
    """K of one snpmi_dev_syrk_dense: Z [n, m] goes to the device as [m][ldz] (F order, ldz =
    round_up(n, 256) unless given), rows n .. ldz - 1 of every column hold `pad` (None = 0); the
    tiles (a fresh buffer unless given) hold 0xFF bytes first when `poison`; the whole K comes back
    through snpmi_dev_grm_extract.  Hooks are set around the launch and restored."""
    dtype = np.dtype(dtype)
    m = Z.shape[1]
    assert Z.shape[0] == n and Z.dtype == dtype
    ldz = round_up(n, 256) if ldz is None else ldz
    host = np.full((m, ldz), 0 if pad is None else pad, dtype=dtype)
    host[:, :n] = Z.T
    code = N.dt_code(dtype)
    tile_bytes = int(N.lib().snpmi_grm_tile_bytes(n, code))
    dz = bench.Dev(N, max(host.nbytes, 256))
    own = bench.Dev(N, tile_bytes) if tiles is None else None
    out = bench.Dev(N, n * n * dtype.itemsize)
    K = np.empty((n, n), dtype=dtype)
    try:
        t = own if tiles is None else tiles
        if m:
            N.call("snpmi_memcpy_h2d", dz.p, N.ptr(host), host.nbytes)
        if poison:
            N.call("snpmi_dev_memset", t.p, 0xFF, tile_bytes)
        with hooked(**hooks):
            N.call("snpmi_dev_syrk_dense", dz.p, ldz, n, m, code, t.p, accumulate)
        N.call("snpmi_dev_grm_extract", t.p, n, code, None, n, None, n, 1, 1.0, out.p)
        N.call("snpmi_memcpy_d2h", N.ptr(K), out.p, K.nbytes)
    finally:
        for d in (dz, own, out):
            if d is not None:
                d.free()
    return K


def _k20(Z, n, **kw):
    """the witness: the same call on k_syrk256d alone"""
    hooks = dict(kw.pop("hooks", {}), syrk=20)
    return _dense(Z, n, F32, hooks=hooks, **kw)


def note(group, what, e):
    if np.isfinite(e):
        WORST[group, what] = max(WORST.get((group, what), 0.0), float(e))


def same_bits(K, ref, label, group=None):
    """K is the reference, bit for bit (exact data: the reference is exact in K's dtype)"""
    assert K.shape == ref.shape
    expect = ref.astype(K.dtype)
    if not np.array_equal(K, expect):
        bad = np.argwhere(~(K == expect))
        raise AssertionError("%s: %d elements differ, first at %s: %r vs %r"
                             % (label, len(bad), bad[0], K[tuple(bad[0])], expect[tuple(bad[0])]))
    if group:
        note(group, "exact data, differing elements", 0.0)


def within_bar(group, K, ref, Z, label, skip=None):
    """the dtype's bar on normal data; a NaN (an unwritten element) fails it.  skip: a row / column
    left out (D's NaN case)."""
    m = Z.shape[1]
    assert K.shape == ref.shape and K.dtype == Z.dtype
    d = np.abs(K - ref)  # f32 - f64 -> f64
    if skip is not None:
        keep = np.ones(len(K), dtype=bool)
        keep[skip] = False
        d, ref = d[np.ix_(keep, keep)], ref[np.ix_(keep, keep)]
    if K.dtype == F32:
        e = d.max() / np.abs(np.diag(ref)).max()
        print(group, label, "f32 error / max diag %.3e" % e)
        note(group, "f32 / max diag", e)
        assert e <= BAR32, (label, e, "largest at", np.unravel_index(d.argmax(), d.shape))
    else:
        assert skip is None
        z = np.abs(Z.astype(np.float64))
        bound = 2 * (m + 1) * 2.0 ** -53 * (z @ z.T)
        e = (d / np.where(bound > 0, bound, 1)).max()
        print(group, label, "f64 error / bound %.3e, / max diag %.3e" % (e, d.max() / np.abs(np.diag(ref)).max()))
        note(group, "f64 / elementwise bound", e)
        note(group, "f64 / max diag", d.max() / np.abs(np.diag(ref)).max())
        assert (d <= bound).all(), (label, e)


def check(group, kind, K, ref, Z, label):
    if kind == "exact":
        same_bits(K, ref, label, group)
    else:
        within_bar(group, K, ref, Z, label)


def stays_fp16x2(K, K20, label):
    assert (K != K20).any(), label + ": the bits of k_syrk256d -- the launch fell back"


def falls_back(K, K20, label):
    assert np.array_equal(K, K20), label + ": not the bits of k_syrk256d -- the launch did not fall back"


def scaled(Z, ref):
    """the data times 2^-10 (exact) and its reference"""
    return Z * DOWN, ref * 2.0 ** -20


# ------------------------------------------------------------------- A. block edges of the n >= 4096 tier
@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("n", [4096, 4097, 4351, 4352, 4353])
def test_block_edges(n, kind):
    """16, 17 and 18 blocks of 256 iids with a full, a one-row and a 255-row last block, m = 33 (one
    stage and one SNP), on fp16x2 and on the fallback.  Catches: a last block whose rows past n are
    read as data or whose tiles past n_tiles are written, a supertile table that is no permutation
    of the triangle (a block computed twice, another never: it stays NaN), the stage-image block
    stride taken from another count than the kernel's, the 128-tile a 256-block's wave owns."""
    Z, ref = reference(kind, n, 33, 1000 + n)
    K, K20 = _dense(Z, n, F32), _k20(Z, n)
    check("A", kind, K, ref, Z, "n %d fp16x2" % n)
    check("A", kind, K20, ref, Z, "n %d syrk 20" % n)
    if kind == "normal":
        stays_fp16x2(K, K20, "n %d" % n)
    Zs, refs = scaled(Z, ref)
    Ks = _dense(Zs, n, F32)
    falls_back(Ks, _k20(Zs, n), "n %d scaled" % n)
    check("A", kind, Ks, refs, Zs, "n %d fallback" % n)


# ------------------------------------------------------------------- B. SNP counts (k-tail)
M_EDGES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65]


@pytest.mark.parametrize("m", M_EDGES)
def test_snp_count_edges_wide(m):
    """n = 4097, exact data, SNP counts around one 16-SNP step and one and two 32-SNP stages, on
    fp16x2 (k_image_h2 zero-fills the SNPs past m of the last stage) and on the fallback (k_syrk256d
    zero-fills its 16-SNP stage in LDS).  Catches: the last SNP dropped or a SNP past m read, a
    half-filled stage taken from stale images / LDS, a stage count rounded the wrong way."""
    Z, ref = reference("exact", 4097, m, 2000 + m)
    same_bits(_dense(Z, 4097, F32), ref, "m %d fp16x2" % m, "B")
    Zs, refs = scaled(Z, ref)
    Ks = _dense(Zs, 4097, F32)
    same_bits(Ks, refs, "m %d fallback" % m, "B")
    falls_back(Ks, _k20(Zs, 4097), "m %d scaled" % m)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["exact", "normal"])
def test_snp_count_edges_small(kind, dtype):
    """The same SNP counts at n = 257 (three 128-tiles a side, a one-row last tile) on the small
    f32 kernel (clamped loads of the last stage, zeroed in registers) and on k_syrk_glds (f64, LDS
    zero-fill).  Catches: the clamp without the zeroing, or the tail stage skipped."""
    for m in M_EDGES:
        Z, ref = reference(kind, 257, m, 2100 + m, dtype)
        check("B", kind, _dense(Z, 257, dtype), ref, Z, "n 257 m %d %s" % (m, dtype.name))


@pytest.mark.parametrize("n,dtype", [(4097, F32), (257, F32), (257, F64)], ids=["wide", "small", "f64"])
def test_no_snps(n, dtype):
    """m = 0: K = nothing turns poisoned tiles into an all-zero K, K += nothing leaves a K that was
    there bit-identical.  Catches: an early return before the memset, a memset when accumulating."""
    empty = np.empty((n, 0), dtype=dtype)
    K = _dense(empty, n, dtype)
    assert K.shape == (n, n) and not K.any()
    Z, ref = reference("exact", n, 17, 2200 + n, dtype)
    tiles = bench.Dev(N, int(N.lib().snpmi_grm_tile_bytes(n, N.dt_code(dtype))))
    try:
        K1 = _dense(Z, n, dtype, tiles=tiles)
        same_bits(_dense(empty, n, dtype, tiles=tiles, accumulate=1, poison=False), ref, "K += nothing")
        same_bits(K1, ref, "K")
    finally:
        tiles.free()


# ------------------------------------------------------------------- C. chunks and accumulation
@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("m", [32, 33, 64, 65, 97])
def test_stage_image_chunks(m, kind):
    """n = 4097, stage images in chunks of 32 SNPs: one, one and a SNP, two, two and a SNP, three and
    a SNP.  Every chunk after the first must add to the tiles even though the call does not
    accumulate, and its images start at column c0 of Z.  Catches: a later chunk overwriting K, the
    chunk's column offset or SNP count wrong, a short last chunk reading the images of the one
    before.  Exact data: the bits of the unchunked K."""
    Z, ref = reference(kind, 4097, m, 3000 + m)
    K = _dense(Z, 4097, F32, hooks={"dense_chunk": 32})
    check("C", kind, K, ref, Z, "chunk 32, m %d" % m)
    if kind == "exact":
        assert np.array_equal(K, _dense(Z, 4097, F32)), "chunked != unchunked"
    else:
        stays_fp16x2(K, _k20(Z, 4097), "chunk 32, m %d" % m)


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("second", ["fp16x2", "fallback"])
def test_two_accumulating_calls(second, kind):
    """n = 4097: 33 SNPs into poisoned tiles (accumulate = 0), then 40 more (accumulate = 1); the
    second call on fp16x2, or scaled by 2^-10 so that the fallback adds to what fp16x2 wrote.
    Catches: accumulate ignored by either epilogue (the first K lost, or NaN kept from the poison),
    the gated kernel of the path not taken touching the tiles.  Exact data, same path: the bits of
    one call over all 73 SNPs.  Exact data, scaled second call: each call's own sum is exact and
    the add rounds once, as the cast of the (exact) f64 reference does, so the bits agree."""
    n = 4097
    Z, _ = reference(kind, n, 73, 3100)
    Z = Z.copy()
    if second == "fallback":
        Z[:, 33:] *= DOWN
    ref = product(Z)
    tiles = bench.Dev(N, int(N.lib().snpmi_grm_tile_bytes(n, N.DT_F32)))
    try:
        _dense(Z[:, :33], n, F32, tiles=tiles)
        K = _dense(Z[:, 33:], n, F32, tiles=tiles, accumulate=1, poison=False)
        if second == "fallback":  # the witness of the second call alone
            falls_back(_dense(Z[:, 33:], n, F32), _k20(Z[:, 33:], n), "second call")
    finally:
        tiles.free()
    if kind == "exact":
        assert np.array_equal(K, ref.astype(np.float32)), "two calls != the reference"
        if second == "fp16x2":
            assert np.array_equal(K, _dense(Z, n, F32)), "two calls != one call"
    else:
        within_bar("C", K, ref, Z, "33 + 40, second on " + second)


# ------------------------------------------------------------------- D. range flag bounds
def with_column_max(Z, s, target):
    """column s rescaled by a power of two so that its max |z| lies in [target / 2, target), then
    its largest element set to exactly `target` (sign kept)"""
    Z = Z.copy()
    col = Z[:, s]
    i = np.abs(col).argmax()
    col *= np.float32(2.0 ** (np.ceil(np.log2(float(target))) - 1 - np.floor(np.log2(float(np.abs(col[i]))))))
    assert target / 2 <= np.abs(col[i]) < target
    col[i] = np.copysign(np.float32(target), col[i])
    assert np.abs(Z[:, s]).max() == np.float32(target)
    return Z


QUARTER, TOP = np.float32(0.25), np.float32(32768)
BOUNDS = {
    "quarter": (QUARTER, True),
    "below_quarter": (np.nextafter(QUARTER, np.float32(0)), False),
    "below_2p15": (np.nextafter(TOP, np.float32(0)), True),
    "2p15": (TOP, False),
}


@pytest.mark.parametrize("case", list(BOUNDS))
def test_range_flag_bounds(case):
    """n = 4096, m = 33, normal data with column 7's max |z| exactly 2^-2, one ulp below, one ulp
    below 2^15, 2^15: fp16x2, fallback, fp16x2, fallback.  Catches: either comparison of the range
    check off by its equality (>= / <), a column max that skips an element or a thread's share."""
    target, h2 = BOUNDS[case]
    base, _ = reference("normal", 4096, 33, 4000)
    Z = with_column_max(base, 7, target)
    ref = product(Z)
    K, K20 = _dense(Z, 4096, F32), _k20(Z, 4096)
    within_bar("D", K, ref, Z, case)
    (stays_fp16x2 if h2 else falls_back)(K, K20, case)


def test_zero_column_keeps_fp16x2():
    """An all-zero column (max 0 < 2^-2) must not raise the flag.  Catches: the m != 0 exemption of
    the range check dropped."""
    base, _ = reference("normal", 4096, 33, 4000)
    Z = base.copy()
    Z[:, 11] = 0
    K = _dense(Z, 4096, F32)
    within_bar("D", K, product(Z), Z, "zero column")
    stays_fp16x2(K, _k20(Z, 4096), "zero column")


def test_one_nan_value():
    """One NaN at (i, s): row and column i of K are NaN, nothing else is, the rest meets the bar and
    the path stays fp16x2 (the column max ignores NaN, as k_lut_h2's does).  Catches: a NaN that
    spreads through a shared accumulator, or that raises the flag."""
    base, _ = reference("normal", 4096, 33, 4000)
    i, s = 1234, 5
    Z = base.copy()
    Z[i, s] = np.nan
    K, K20 = _dense(Z, 4096, F32), _k20(Z, 4096)
    for name, k in (("fp16x2", K), ("syrk 20", K20)):
        nan = np.isnan(k)
        assert nan[i].all() and nan[:, i].all() and nan.sum() == 2 * 4096 - 1, name
    Zf = np.nan_to_num(Z, nan=0.0)
    within_bar("D", K, product(Zf), Zf, "one NaN", skip=i)
    keep = np.arange(4096) != i
    stays_fp16x2(K[np.ix_(keep, keep)], K20[np.ix_(keep, keep)], "one NaN")


# ------------------------------------------------------------------- E. leading dimension and pad rows
@pytest.mark.parametrize("path", ["fp16x2", "fallback"])
def test_pad_rows_wide(path):
    """n = 4200, m = 45, normal data: pad rows 4200 .. 4351 of NaN and of 1e30 give the bits of zero
    pads, and 1e30 does not raise the range flag.  (In production the pads are whatever the scratch
    held.)  Catches: the column max taken over ldz rows, a pad row reaching K through a panel load
    that ignores n, a tile past the triangle written."""
    n = 4200
    Z, ref = reference("normal", n, 45, 5000)
    if path == "fallback":
        Z, ref = scaled(Z, ref)
    K0, K20 = _dense(Z, n, F32, pad=0), _k20(Z, n, pad=0)
    within_bar("E", K0, ref, Z, "pad 0, " + path)
    (stays_fp16x2 if path == "fp16x2" else falls_back)(K0, K20, "pad 0")
    for pad in (np.nan, 1e30):
        assert np.array_equal(_dense(Z, n, F32, pad=pad), K0), "pad %r changes K on %s" % (pad, path)
    assert np.array_equal(_k20(Z, n, pad=np.nan), K20)


@pytest.mark.parametrize("kind", ["exact", "normal"])
def test_longer_leading_dimension_wide(kind):
    """n = 4200 with ldz = 4352 + 256 stays on fp16x2 and gives the bits of ldz = 4352: the
    block-order table is the one of ceil(n / 256) = 17 blocks, not of ldz / 256 = 18 (whose first
    153 entries name a block (0, 17) outside the tiles and never (16, 16)).  ldz = 4352 + 4 is no
    multiple of 256 and goes to k_syrk256d: the witness's bits, the reference's on exact data.
    NaN pads throughout.  Catches: any count taken from ldz instead of n, a 16-byte load that
    assumes ldz % 256 == 0."""
    n, ld = 4200, 4352
    Z, ref = reference(kind, n, 45, 5000)
    K = _dense(Z, n, F32)
    check("E", kind, K, ref, Z, "ldz 4352")
    assert np.array_equal(_dense(Z, n, F32, ldz=ld + 256, pad=np.nan), K), "ldz + 256"
    K4 = _dense(Z, n, F32, ldz=ld + 4, pad=np.nan)
    if kind == "exact":
        assert np.array_equal(K4, K), "ldz + 4"
    else:
        falls_back(K4, _k20(Z, n), "ldz + 4")
        stays_fp16x2(K, K4, "ldz 4352")
        within_bar("E", K4, ref, Z, "ldz + 4")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["exact", "normal"])
def test_pad_rows_and_ldz_small(kind, dtype):
    """n = 300 on the small f32 kernel and on k_syrk_glds: ldz = 384 (round_up(n, 128)) and 388
    (% 4 only), pads 0 / NaN / 1e30, all the bits of the first.  Catches: a panel row stride other
    than ldz, pads reaching K, an aligned-load assumption beyond ldz % 4 == 0."""
    n = 300
    Z, ref = reference(kind, n, 45, 5100, dtype)
    K0 = _dense(Z, n, dtype, ldz=384, pad=0)
    check("E", kind, K0, ref, Z, "n 300 %s" % dtype.name)
    for ldz in (384, 388):
        for pad in (0, np.nan, 1e30):
            assert np.array_equal(_dense(Z, n, dtype, ldz=ldz, pad=pad), K0), (ldz, pad)


def test_stale_pads_of_the_upload_scratch():
    """End to end through snpmi_grm_dense_f32: a 4352 x 45 matrix of 1e30, then 4097 x 45 normal
    values.  Both uploads have ldz = 4352 and the same size, the second copies 4097 rows of each
    column and leaves 1e30 in the 255 below.  Catches: what test_pad_rows_wide catches, on the
    path production takes; the K is also the bits of the entry's with zero pads."""
    n, m = 4097, 45
    big = np.full((4352, m), 1e30, dtype=np.float32, order="F")
    Kbig = np.empty((4352, 4352), dtype=np.float32)
    N.call("snpmi_grm_dense_f32", N.ptr(big), 4352, m, 0, N.STD_NONE, 0.0, 0.0, 0, None, 0, None, N.ptr(Kbig))
    del Kbig
    Z, ref = reference("normal", n, m, 5200)
    Zf, K = np.asfortranarray(Z), np.empty((n, n), dtype=np.float32)
    N.call("snpmi_grm_dense_f32", N.ptr(Zf), n, m, 0, N.STD_NONE, 0.0, 0.0, 0, None, 0, None, N.ptr(K))
    within_bar("E", K, ref, Z, "stale 1e30 pads")
    assert np.array_equal(K, _dense(Z, n, F32, pad=0))


# ------------------------------------------------------------------- F. segments
@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("m", [63, 64, 65, 129, 193])
def test_segments(m, kind):
    """n = 4097, 64-SNP accumulation segments: fp16x2 flushes its accumulators every two 32-SNP
    stages into a scratch slot (SegFlush in MODE 6: a first flush that stores, later ones that add,
    a phase that differs per workgroup, no flush after the last stage); the fallback runs one
    launch per 64 SNPs (for_segments).  m = one SNP short of, exactly and one past a segment, two
    and three segments and a SNP.  Catches: a segment lost or added twice when m ends on a flush,
    a slot read back before its adds landed, the later launches of the fallback overwriting K.
    Exact data: the bits of seg = 0."""
    n = 4097
    Z, ref = reference(kind, n, m, 6000 + m)
    Zs, refs = scaled(Z, ref)
    with hooked(seg=64):
        K, Ks = _dense(Z, n, F32), _dense(Zs, n, F32)
        K20, Ks20 = _k20(Z, n), _k20(Zs, n)
    check("F", kind, K, ref, Z, "seg 64, m %d fp16x2" % m)
    check("F", kind, Ks, refs, Zs, "seg 64, m %d fallback" % m)
    falls_back(Ks, Ks20, "seg 64, m %d scaled" % m)
    if kind == "exact":
        with hooked(seg=0):
            assert np.array_equal(K, _dense(Z, n, F32)) and np.array_equal(Ks, _dense(Zs, n, F32))
    else:
        stays_fp16x2(K, K20, "seg 64, m %d" % m)


# ------------------------------------------------------------------- G. C-order device operand
def session_k(val, n, m, dtype, order_c):
    K = np.empty((n, n), dtype=dtype)
    sfx = "f32" if dtype == F32 else "f64"
    N.call("snpmi_grm_begin", n, N.dt_code(dtype))
    try:
        N.call("snpmi_grm_add_dense_" + sfx, val, n, m, order_c)
    finally:
        N.call("snpmi_grm_end", 0, None, N.ptr(K))
    return K


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,m", [(300, 65), (4097, 33)])
def test_c_order_device_operand(n, m, dtype):
    """snpmi_grm_add_dense with a device pointer to a C-order [n][m] block (k_transpose into the
    padded F-order scratch), neither side a multiple of the 64 x 64 transpose tile.  Exact data:
    the bits of the same call on the F-order host array, and of the reference.  Catches: a partial
    transpose tile dropped or written past ld, rows and columns swapped, the wrong element size."""
    Z, ref = reference("exact", n, m, 7000 + n, dtype)
    Zc = np.ascontiguousarray(Z)
    dev = bench.Dev(N, Zc.nbytes)
    try:
        N.call("snpmi_memcpy_h2d", dev.p, N.ptr(Zc), Zc.nbytes)
        Kc = session_k(dev.p, n, m, dtype, 1)
    finally:
        dev.free()
    same_bits(Kc, ref, "C-order device operand", "G")
    Zf = np.asfortranarray(Z)
    assert np.array_equal(Kc, session_k(N.ptr(Zf), n, m, dtype, 0))
