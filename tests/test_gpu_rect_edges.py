"""The two-operand ("rect") GRM kernels, K[rows, cols] computed directly, at the block, stage and
moduli edges that test_gpu_rect.py's one synthetic shape (300 x 700, homogeneous genotypes) does
not reach.  Reference everywhere: the f64 oracle O.decode_standardize -> Z[rows] @ Z[cols].T;
measure: test_gpu_rect._err (max |dK| / max_i (Z Z^T)_ii over all iids of the source); bars: f32
1e-5, f64 1e-12 (test_gpu_rect.TOL).  Where the arithmetic allows a stronger statement (exact
integer sums on the CRT path, one f64 sum rounded once on the f32 diagonal, a pure copy in the
extraction) the bits, or one ulp, are asserted.  Every launch that does not accumulate starts from
blocks filled with 0xFF bytes, so an element a kernel leaves unwritten reads as NaN and fails.

Shapes, each the smallest that reaches its edge (source: 1101 iids, n % 4 = 1, 5% missing):

A  block edges, m = 200 SNPs (6 1/4 f32 stages of 32; one int8 stage of 128 and a partial one):
   (1, 1), (1, 257), (257, 1): one row / column, nba = 1 / nbb = 1 beside two blocks;
   (255, 256), (256, 255), (256, 256): one short of, and exactly, one 256-block per side;
   (257, 513), (513, 257): one past a block, 2 x 3 and 3 x 2 blocks;
   (all, 1), (3, all): the in-place operand (5 blocks, no repack) beside a one-block other side.
   Forms: f32 default (fp16x2 + gated bf16x3), bf16x3 alone (hook syrk = 36), f64 CRT per block
   and launch-wide (crt_block = 1 / 0), the two-operand f64 MFMA (hook f64 = 1).
B  SNP counts on a 257 x 513 rectangle (2 x 3 blocks, odd row count): around the 64-SNP SegFlush
   trip and whole 256-SNP segments (f32, seg = 256), one SNP / one past a stage under the shipped
   seg, around the 128-SNP int8 stage (f64).
C  unequal panel bounds: two iids carry every SNP, so a light row panel beside a heavy column panel
   needs more moduli than the row panel alone would choose (pins the second bound table and the
   two-sum scan of the launch-wide R); 257 rows, so B's sums start behind A's odd-count padding.
D  the exact f32 diagonal inside a rectangle: 300 x 700 with repeats on both sides, pairs off the
   block diagonal, two accumulating adds, the hook off, identity sides.
E  snpmi_dev_rect_extract, both orders, a scale != 1, host and device outputs (257 x 513).
F  residue chunks of a rectangle: 4370 blocks (2 x 2185), one more than a 4 GiB residue chunk
   holds; the cut falls inside the last block column.  Sized by that constant of the library.
"""
import contextlib
import ctypes
import time

import numpy as np
import pytest

from conftest import DATA  # noqa: F401  (sys.path)
import bench
from oracle import oracle as O
from pysnptools_amd import _native as N
from test_gpu_rect import TOL, _err, _operand, _session, _stateless, data, m, m2, n  # noqa: F401  (data: fixture)

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
# kernel form -> (dtype, hooks set around the launch)
FORMS = {
    "f32": (F32, {}),
    "bf3": (F32, {"syrk": 36}),
    "crt": (F64, {"crt_block": 1}),
    "crt_wide": (F64, {"crt_block": 0}),
    "f64mfma": (F64, {"f64": 1}),
}
WORST = {}  # (section, form) -> the largest error seen, printed when the module is done


@contextlib.contextmanager
def hooks(**values):
    """snpmi_set_kernel_variant around a block, the former values restored on the way out."""
    old = {k: N.kernel_variant(k) for k in values}
    try:
        for k, v in values.items():
            N.call("snpmi_set_kernel_variant", k.encode(), v)
        yield
    finally:
        for k, v in old.items():
            N.call("snpmi_set_kernel_variant", k.encode(), v)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (section, form), e in sorted(WORST.items()):
        print("worst error, section %s, form %s: %.3e" % (section, form, e))


def draw(count, seed):
    """count iids of the source, seeded, unsorted, one repeated whenever count > 2 (None = all in place)."""
    if count is None:
        return None
    idx = np.random.RandomState(seed).permutation(n)[:count].astype(np.uint64)
    if count > 2:
        idx[count // 2] = idx[0]
    return idx


def take(K, rows, cols):
    r = np.arange(n) if rows is None else rows.astype(np.intp)
    c = np.arange(n) if cols is None else cols.astype(np.intp)
    return K[np.ix_(r, c)]


def run(packed, pitch, rows, cols, form, cnt, **kw):
    dtype, hk = FORMS[form]
    with hooks(**hk):
        return _stateless(packed, pitch, rows, cols, dtype, cnt=cnt, poison=True, **kw)


def check(section, form, K, Z, rows, cols, label):
    """the dtype's bar against the oracle; a NaN (an unwritten element) fails it"""
    dtype = FORMS[form][0]
    ref = (Z if rows is None else Z[rows.astype(np.intp)]) @ (Z if cols is None else Z[cols.astype(np.intp)]).T
    assert K.shape == ref.shape and K.dtype == dtype
    e = _err(K, ref, Z)
    print(section, form, label, e)
    if np.isfinite(e):
        WORST[section, form] = max(WORST.get((section, form), 0.0), e)
    assert e <= TOL[dtype], (label, e)
    return e


def whole_k(packed, pitch, cnt):
    """K of all n iids over the first cnt SNPs on the whole-K f64 path: one snpmi_dev_syrk_packed
    and one snpmi_dev_grm_extract."""
    lut, stats = bench.Dev(N, cnt * 32), bench.Dev(N, cnt * 16)
    tiles, out = bench.Dev(N, int(N.lib().snpmi_grm_tile_bytes(n, N.DT_F64))), bench.Dev(N, n * n * 8)
    K = np.empty((n, n), dtype=np.float64)
    try:
        N.call("snpmi_dev_snp_stats", packed.p, pitch, n, cnt, 0, N.STD_UNIT, 0.0, 0.0, 0, N.DT_F64, stats.p, lut.p)
        N.call("snpmi_dev_syrk_packed", packed.p, pitch, n, cnt, lut.p, N.DT_F64, tiles.p, 0)
        N.call("snpmi_dev_grm_extract", tiles.p, n, N.DT_F64, None, n, None, n, 1, 1.0, out.p)
        N.call("snpmi_memcpy_d2h", N.ptr(K), out.p, K.nbytes)
    finally:
        for d in (lut, stats, tiles, out):
            d.free()
    K.flags.writeable = False
    return K


@pytest.fixture(scope="module")
def whole(data):
    """cnt -> the whole K over the first cnt SNPs of the module's source, computed once per cnt
    (under the shipped hooks) and left unchanged."""
    packed, pitch, _ = data
    cache = {}

    def get(cnt):
        assert N.kernel_variant("f64") == 0 and N.kernel_variant("syrk") == 0 and N.kernel_variant("crt_block") == 1
        if cnt not in cache:
            cache[cnt] = whole_k(packed, pitch, cnt)
        return cache[cnt]

    return get


def crt_pair(section, packed, pitch, Z, rows, cols, cnt, Kwhole, label):
    """both CRT forms: the f64 bar, the bits of the whole K's entries, the bits of each other"""
    Ks = {}
    for form in ("crt", "crt_wide"):
        Ks[form] = run(packed, pitch, rows, cols, form, cnt)
        check(section, form, Ks[form], Z, rows, cols, label)
        # exact integer sums and one launch either way: the same bits as the whole-K path
        assert np.array_equal(Ks[form], take(Kwhole, rows, cols)), (form, label)
    assert np.array_equal(Ks["crt"], Ks["crt_wide"]), label


# ------------------------------------------------------------------- A. block-edge shapes x kernel forms
MA = 200
SHAPES = [(1, 1), (1, 257), (257, 1), (255, 256), (256, 255), (256, 256), (257, 513), (513, 257), (None, 1),
          (3, None)]


@pytest.mark.parametrize("form", ["f32", "bf3", "crt", "f64mfma"])
@pytest.mark.parametrize("nr,nc", SHAPES, ids=lambda v: "all" if v is None else str(v))
def test_block_edge_shapes(data, whole, nr, nc, form):
    """Row / column counts of 1 and around one and two 256-blocks, and the in-place operand beside a
    one-block side, on every kernel form.  Catches: a block index split with nba = 1 or nbb = 1
    that is wrong (wg % nba, wg / nba), rows or columns of a partial block dropped or written past,
    an epilogue that skips part of a dense block, the bf16x3 / f64 MFMA two-operand forms reading
    the A operand for both panels; for the CRT forms any difference from the whole-K path's bits."""
    packed, pitch, Zall = data
    Z = Zall[:, :MA]
    rows, cols = draw(nr, 100 + (nr or 0)), draw(nc, 200 + (nc or 0))
    label = "%s x %s" % (nr, nc)
    if form == "crt":
        crt_pair("A", packed, pitch, Z, rows, cols, MA, whole(MA), label)
    else:
        check("A", form, run(packed, pitch, rows, cols, form, MA), Z, rows, cols, label)


# ------------------------------------------------------------------- B. SNP-count edges
B_ROWS, B_COLS = draw(257, 31), draw(513, 32)


@pytest.mark.parametrize("cnt", [1, 63, 64, 65, 255, 256, 257, 512, 513])
def test_snp_count_edges_f32_seg256(data, cnt):
    """f32 default form with 256-SNP segments: SNP counts around the 64-SNP SegFlush trip of
    k_syrk_h2s and at whole numbers of segments (256, 512).  Catches: a flush that is skipped or
    doubled when the last trip ends exactly on a segment, a tail stage read past m."""
    packed, pitch, Zall = data
    with hooks(seg=256):
        K = run(packed, pitch, B_ROWS, B_COLS, "f32", cnt)
    check("B", "f32", K, Zall[:, :cnt], B_ROWS, B_COLS, "seg 256, m %d" % cnt)


@pytest.mark.parametrize("cnt", [1, 33])
def test_snp_count_edges_f32_shipped_seg(data, cnt):
    """The shipped segment length (one chain at these counts): one SNP, and one past a 32-SNP stage.
    Catches: a partial first / second stage that is not zero-padded through the LUT."""
    packed, pitch, Zall = data
    seg = N.kernel_variant("seg")
    assert seg == 0 or seg > cnt, seg  # no test left a short segment behind
    check("B", "f32", run(packed, pitch, B_ROWS, B_COLS, "f32", cnt), Zall[:, :cnt], B_ROWS, B_COLS,
          "shipped seg, m %d" % cnt)


@pytest.mark.parametrize("form", ["crt", "f64mfma"])
@pytest.mark.parametrize("cnt", [1, 127, 128, 129, 255, 256, 257])
def test_snp_count_edges_f64(data, whole, cnt, form):
    """f64 with SNP counts around one and two int8 stages of 128 SNPs.  Catches: a partial stage
    whose padding SNPs are not zero in the second operand's panel, a stage count rounded the wrong
    way (the last SNP dropped, or a stage of stale LDS added)."""
    packed, pitch, Zall = data
    Z = Zall[:, :cnt]
    if form == "crt":
        crt_pair("B", packed, pitch, Z, B_ROWS, B_COLS, cnt, whole(cnt), "m %d" % cnt)
    else:
        check("B", form, run(packed, pitch, B_ROWS, B_COLS, form, cnt), Z, B_ROWS, B_COLS, "m %d" % cnt)


# ------------------------------------------------------------------- C. unequal panel bounds
H1, H2 = 700, 901


def skew_genotypes():
    """[n, m]: SNPs 0..499 carried only by iid H1 (value 2), 500..999 only by H2 (value 1), every
    other entry 0 with 2% missing among the non-carriers."""
    rng = np.random.default_rng(5)
    v = np.zeros((n, m), dtype=np.float64)
    miss = rng.random((n, m)) < 0.02
    v[H1, :m // 2] = 2.0
    v[H2, m // 2:] = 1.0
    miss[H1, :m // 2] = False
    miss[H2, m // 2:] = False
    v[miss] = np.nan
    return v


def skew_indices():
    rng = np.random.RandomState(9)
    light = rng.permutation(np.setdiff1d(np.arange(n), [H1, H2]))
    rows = light[:257].copy()
    rows[200] = rows[5]  # one repeat
    other = np.concatenate([rows[:150], light[257:257 + 548]])  # 150 shared with the rows
    rng.shuffle(other)
    cols = np.concatenate([other[:10], [H1], other[10:599], [H2], other[599:]])
    assert len(cols) == 700 and cols[10] == H1 and cols[600] == H2
    return rows.astype(np.uint64), cols.astype(np.uint64)


C_ROWS, C_COLS = skew_indices()
C_REQUESTS = {"rows x cols": (C_ROWS, C_COLS), "cols x rows": (C_COLS, C_ROWS), "all x cols": (None, C_COLS)}


@pytest.fixture(scope="module")
def skew():
    """the skewed codes on the device at snpmi_packed_pitch(n), and the oracle's Z in f64"""
    body = O.encode(skew_genotypes())
    pitch = int(N.lib().snpmi_packed_pitch(n))
    host = np.zeros((m, pitch), dtype=np.uint8)
    host[:, :body.shape[1]] = body
    packed = bench.Dev(N, host.nbytes)
    N.call("snpmi_memcpy_h2d", packed.p, N.ptr(host), host.nbytes)
    Z, _ = O.decode_standardize(np.ascontiguousarray(body).reshape(-1), n, m, dtype=np.float64)
    yield packed, pitch, np.ascontiguousarray(Z)
    packed.free()


def crt_counts():
    """(sum of launch-wide R, launches, sum of R_b, blocks) since the last call; resets them"""
    v = [ctypes.c_uint64() for _ in range(4)]
    N.call("snpmi_crt_moduli_stats", ctypes.byref(v[0]), ctypes.byref(v[1]), 1)
    N.call("snpmi_crt_block_moduli_stats", ctypes.byref(v[2]), ctypes.byref(v[3]), 1)
    return tuple(x.value for x in v)


@pytest.fixture(scope="module")
def skew_runs(skew):
    """crt_block -> {request: (K, moduli counts of its launch)}, computed once per value"""
    packed, pitch, _ = skew
    cache = {}

    def get(per_block):
        if per_block not in cache:
            out = {}
            for name, (rows, cols) in C_REQUESTS.items():
                crt_counts()
                K = run(packed, pitch, rows, cols, "crt" if per_block else "crt_wide", m)
                out[name] = (K, crt_counts())
            cache[per_block] = out
        return cache[per_block]

    return get


def test_skew_precondition(skew):
    """The data has teeth: over the light rows, the smallest |K[l, H1]| is at least 1.5 x 256 x the
    largest sum_s z_ls^2.  No modulus exceeds 256, so the smallest R a light row panel alone would
    choose has P_R <= 256 * 2 M, while a correct digit needs |K_int| < P_R / 2 <= 256 M: a block of
    light rows x the heavy column sized from the row panel alone must wrap (1.5: room for the
    quantisation of q at F >= 50 bits).  Catches: a change of the data that would let such a
    kernel pass the tests below.  (This seed: heavy sum z^2 5.39e5, light <= 0.92, ratio 2.04.)"""
    _, _, Z = skew
    S = np.einsum("ij,ij->i", Z, Z)
    rows = C_ROWS.astype(np.intp)
    print("sum z^2: heavy", S[H1], S[H2], "light max", np.delete(S, [H1, H2]).max(),
          "min |K[l, H1]|", np.abs(Z[rows] @ Z[H1]).min())
    assert np.abs(Z[rows] @ Z[H1]).min() >= 1.5 * 256 * S[rows].max()


@pytest.mark.parametrize("per_block", [1, 0])
def test_unequal_panel_bounds_f64(skew, skew_runs, per_block):
    """f64 CRT on light rows x cols that hold the two heavy iids (in different column blocks), the
    transposed request and the in-place rows.  Catches: block_moduli taking both bounds from A's
    table or indexing B's with bi (the light x heavy blocks then wrap); with crt_block = 0 a
    launch-wide R that scans A's sums only, or misses B's behind the padding of A's odd count."""
    _, _, Z = skew
    runs = skew_runs(per_block)
    form = "crt" if per_block else "crt_wide"
    for name, (rows, cols) in C_REQUESTS.items():
        check("C", form, runs[name][0], Z, rows, cols, name)
    # exact integer sums: the same bits either way round, and under either choice of moduli
    assert np.array_equal(runs["rows x cols"][0], runs["cols x rows"][0].T)
    first = skew_runs(1)
    for name in C_REQUESTS:
        assert np.array_equal(runs[name][0], first[name][0]), name
    if per_block:
        for name, (rows, cols) in C_REQUESTS.items():
            sum_r, launches, sum_rb, blocks = runs[name][1]
            nr, nc = (n if rows is None else len(rows)), len(cols)
            assert launches == 1 and blocks == -(-nr // 256) * -(-nc // 256), (name, launches, blocks)
        sum_r, launches, sum_rb, blocks = runs["rows x cols"][1]
        print("rows x cols: launch-wide R", sum_r, "mean R_b", sum_rb / blocks)
        assert sum_rb / blocks < sum_r / launches  # the light x light blocks run fewer moduli


def test_panel_bound_probes(skew):
    """One-block launches: 256 light rows x 256 cols that hold H1 run more moduli than the same rows
    x 256 light cols.  Catches: R_b taken from the row panel alone (both probes would agree)."""
    packed, pitch, Z = skew
    rb = {}
    for name, cols in (("light", C_COLS[256:512]), ("heavy", C_COLS[:256])):
        assert (H1 in cols) == (name == "heavy") and H2 not in cols
        crt_counts()
        K = run(packed, pitch, C_ROWS[:256], cols, "crt", m)
        _, launches, sum_rb, blocks = crt_counts()
        assert launches == 1 and blocks == 1
        check("C", "crt", K, Z, C_ROWS[:256], cols, "probe " + name)
        rb[name] = sum_rb
    print("R_b: light x light", rb["light"], "light x heavy", rb["heavy"])
    assert rb["heavy"] > rb["light"]


def test_unequal_panel_bounds_f32(skew):
    """The same requests on the f32 default form: the heavy values are |z| ~ 33, inside fp16's range.
    Catches: a panel's LUT scaling shared between the two operands' loaders."""
    packed, pitch, Z = skew
    for name, (rows, cols) in C_REQUESTS.items():
        check("C", "f32", run(packed, pitch, rows, cols, "f32", m), Z, rows, cols, name)


# ------------------------------------------------------------------- D. the exact f32 diagonal
def diag_indices():
    rng = np.random.RandomState(13)
    perm = rng.permutation(n)
    rows = perm[:300].copy()
    rows[200], rows[280] = rows[3], rows[40]  # two repeats, of iids that are among the shared
    cols = np.concatenate([rows[:150], perm[300:850]])  # 150 shared with the rows
    rng.shuffle(cols)
    other = np.flatnonzero(~np.isin(cols, rows))
    cols[other[0]] = rows[3]  # a repeat that is also a (repeated) row: 2 x 2 pairs
    cols[other[1]] = cols[other[7]]  # a repeat that is no row
    return rows.astype(np.uint64), cols.astype(np.uint64)


D_ROWS, D_COLS = diag_indices()


@pytest.fixture(scope="module")
def sq32(data):
    """(d1, d2): per iid, sum_s float64(z32_is)^2 over the first m SNPs and over the m2 after them,
    z32 the oracle's f32 standardization (bit-equal to the device LUT).  Each square is exact in
    f64; the order of summation moves the sum by ~m 2^-53 relative, so float32(d) is the device
    value up to one ulp of f32."""
    packed, pitch, _ = data
    host = np.empty((m + m2, pitch), dtype=np.uint8)
    N.call("snpmi_memcpy_d2h", N.ptr(host), packed.p, host.nbytes)
    body = np.ascontiguousarray(host[:, :(n + 3) // 4]).reshape(-1)
    z32, _ = O.decode_standardize(body, n, m + m2, dtype=np.float32)
    z = z32.astype(np.float64)
    return np.einsum("ij,ij->i", z[:, :m], z[:, :m]), np.einsum("ij,ij->i", z[:, m:], z[:, m:])


def pairs_of(rows, cols):
    from pysnptools_amd.kernelreader.rect import diag_pairs

    nr, nc = (n if rows is None else len(rows)), (n if cols is None else len(cols))
    p = diag_pairs(rows, cols, nr, nc).astype(np.intp)
    r = np.arange(n) if rows is None else rows.astype(np.intp)
    c = np.arange(n) if cols is None else cols.astype(np.intp)
    # the brute-force list, repeats giving every combination
    rr, cc = np.nonzero(r[:, None] == c[None, :])
    assert len(p) == len(rr) and len(p) > 0
    assert np.array_equal(p[np.lexsort((p[:, 1], p[:, 0]))], np.stack([rr, cc], axis=1))
    return p[:, 0], p[:, 1], r[p[:, 0]]


def within_one_ulp(got, expect32):
    assert got.dtype == F32 and expect32.dtype == F32
    return np.abs(got.astype(np.float64) - expect32.astype(np.float64)) <= np.spacing(expect32)


def test_diag_index_lists():
    """The lists reach what the section is about: repeats on both sides, one of the repeated cols
    also a row, 150 shared iids, a shared iid whose row block and column block differ.  Catches:
    a change of the seeds or sizes that leaves the tests below without those cases."""
    assert len(D_ROWS) == 300 and len(np.unique(D_ROWS)) == 298
    assert len(D_COLS) == 700 and len(np.unique(D_COLS)) == 698
    assert len(np.intersect1d(D_ROWS, D_COLS)) == 150
    vals, counts = np.unique(D_COLS, return_counts=True)
    assert np.isin(vals[counts > 1], D_ROWS).any() and not np.isin(vals[counts > 1], D_ROWS).all()
    pr, pc = np.nonzero(D_ROWS[:, None] == D_COLS[None, :])
    assert (pr // 256 != pc // 256).any() and (pr // 256 == pc // 256).any()


def test_diag_stateless_pairs(data, sq32):
    """One launch with the pair list.  Catches: a pair patched at the wrong offset (pairs off the
    block diagonal, repeated indices), the square sums indexed by the column instead of the row,
    a patch that touches a position that is no pair, a pair that is left to the MFMA chain."""
    packed, pitch, Zall = data
    d1, _ = sq32
    pr, pc, iid = pairs_of(D_ROWS, D_COLS)
    K = _stateless(packed, pitch, D_ROWS, D_COLS, np.float32, poison=True)
    K0 = _stateless(packed, pitch, D_ROWS, D_COLS, np.float32, exact_diag=False, poison=True)
    check("D", "f32", K, Zall[:, :m], D_ROWS, D_COLS, "stateless, pairs")
    ok = within_one_ulp(K[pr, pc], d1[iid].astype(np.float32))
    assert ok.all(), (np.flatnonzero(~ok), K[pr, pc][~ok], d1[iid][~ok])
    other = np.ones(K.shape, dtype=bool)
    other[pr, pc] = False
    assert np.array_equal(K[other], K0[other])
    print("pairs", len(pr), "of them differing from the chain's own diagonal", int((K[pr, pc] != K0[pr, pc]).sum()))


def test_diag_session_two_adds(data, sq32):
    """Two accumulating adds (1000 + 37 SNPs).  Catches: the second add dropping the first add's
    diagonal (saved[p] not read when accumulating), or rounding the sum twice."""
    packed, pitch, Zall = data
    d1, d2 = sq32
    pr, pc, iid = pairs_of(D_ROWS, D_COLS)
    K = _session(packed, pitch, np.float32, [(0, m), (m, m2)], D_ROWS, D_COLS)
    expect = (d1[iid].astype(np.float32).astype(np.float64) + d2[iid]).astype(np.float32)
    ok = within_one_ulp(K[pr, pc], expect)
    assert ok.all(), (np.flatnonzero(~ok), K[pr, pc][~ok], expect[~ok])
    check("D", "f32", K, Zall, D_ROWS, D_COLS, "session 1000 + 37")


def test_diag_hook_off_session(data):
    """Hook diag = 0: the session gives the bits of the stateless launch without pairs, so the hook
    is the only difference between the two.  Catches: a session that patches regardless of the hook."""
    packed, pitch, _ = data
    K0 = _stateless(packed, pitch, D_ROWS, D_COLS, np.float32, exact_diag=False, poison=True)
    with hooks(diag=0):
        K = _session(packed, pitch, np.float32, [(0, m)], D_ROWS, D_COLS)
    assert np.array_equal(K, K0)


@pytest.mark.parametrize("side", ["all x cols", "rows x all"])
def test_diag_identity_sides(data, sq32, side):
    """An in-place side: (all, cols) and (rows, all), the latter through the branch of
    rect_diag_pairs for an identity column list.  Catches: pairs built as (r, r) instead of
    (r, rows[r]) / (cols[c], c), or none at all for an identity side."""
    packed, pitch, Zall = data
    d1, _ = sq32
    rows, cols = (None, D_COLS) if side == "all x cols" else (D_ROWS, None)
    pr, pc, iid = pairs_of(rows, cols)
    assert len(pr) == (len(D_COLS) if rows is None else len(D_ROWS))
    K = _session(packed, pitch, np.float32, [(0, m)], rows, cols)
    ok = within_one_ulp(K[pr, pc], d1[iid].astype(np.float32))
    assert ok.all(), (np.flatnonzero(~ok), K[pr, pc][~ok], d1[iid][~ok])
    check("D", "f32", K, Zall[:, :m], rows, cols, side)


# ------------------------------------------------------------------- E. snpmi_dev_rect_extract
@pytest.fixture(scope="module")
def raw_blocks(data):
    """dtype -> the raw blocks of one 257 x 513 launch on the host, [nbb, nba, 256, 256], and the
    same blocks still on the device"""
    packed, pitch, _ = data
    nr, nc = len(B_ROWS), len(B_COLS)
    out, held = {}, []
    for dtype in (F32, F64):
        lut, stats = bench.Dev(N, m * 4 * dtype.itemsize), bench.Dev(N, m * 2 * dtype.itemsize)
        N.call("snpmi_dev_snp_stats", packed.p, pitch, n, m, 0, N.STD_UNIT, 0.0, 0.0, 0, N.dt_code(dtype), stats.p, lut.p)
        a, pa, pitch_a = _operand(packed, pitch, B_ROWS, m)
        b, pb, pitch_b = _operand(packed, pitch, B_COLS, m)
        nbytes = int(N.lib().snpmi_grm_rect_bytes(nr, nc, N.dt_code(dtype)))
        blocks = bench.Dev(N, nbytes)
        held.append(blocks)
        try:
            N.call("snpmi_dev_memset", blocks.p, 0xFF, nbytes)
            N.call("snpmi_dev_syrk_rect", pa, pitch_a, nr, pb, pitch_b, nc, m, lut.p, N.dt_code(dtype), blocks.p, 0, None, 0)
            N.call("snpmi_stream_sync")
            host = np.empty((-(-nc // 256), -(-nr // 256), 256, 256), dtype=dtype)
            assert host.nbytes == nbytes
            N.call("snpmi_memcpy_d2h", N.ptr(host), blocks.p, nbytes)
        finally:
            for d in (lut, stats, a, b):
                d.free()
        out[dtype] = (host, blocks)
    yield out
    for d in held:
        d.free()


@pytest.mark.parametrize("device_out", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("order_c", [1, 0])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rect_extract(raw_blocks, dtype, order_c, scale, device_out):
    """Blocks -> K_out against the documented layout (slot bj * nba + bi, row-major 256 x 256),
    bit for bit: (T)((double)v * scale) restates the kernel's arithmetic.  Catches: the F order
    written transposed or with the wrong leading dimension, the scale dropped or applied in T,
    a device output routed through the host staging path."""
    dtype = np.dtype(dtype)
    host, blocks = raw_blocks[dtype]
    nr, nc = len(B_ROWS), len(B_COLS)
    full = host.transpose(1, 2, 0, 3).reshape(host.shape[1] * 256, host.shape[0] * 256)[:nr, :nc]
    assert np.isfinite(full).all() and full.any()
    expect = (full.astype(np.float64) * scale).astype(dtype)
    K = np.full((nr, nc), 7.0, dtype=dtype, order="C" if order_c else "F")
    if device_out:
        dev = bench.Dev(N, K.nbytes)
        try:
            N.call("snpmi_dev_memset", dev.p, 0xFF, K.nbytes)
            N.call("snpmi_dev_rect_extract", blocks.p, nr, nc, N.dt_code(dtype), order_c, scale, dev.p)
            N.call("snpmi_memcpy_d2h", N.ptr(K), dev.p, K.nbytes)
        finally:
            dev.free()
    else:
        N.call("snpmi_dev_rect_extract", blocks.p, nr, nc, N.dt_code(dtype), order_c, scale, N.ptr(K))
    assert np.array_equal(K, expect)


# ------------------------------------------------------------------- F. residue chunks of a rectangle
def test_residue_chunks_of_a_rectangle(data, whole):
    """257 x 559,105 in f64: 2 x 2185 = 4370 blocks, one more than the 4369 that 4 GiB of residues
    hold (15 moduli x 65536 bytes per block), so the launch is cut into two residue chunks and the
    cut (block 4369 = bi 1, bj 2184) falls inside the last block column.  Catches: the second
    chunk's blocks decoded with the first chunk's coordinates ((b0 + bx) % nba, / nba with b0 > 0),
    or reconstructed into the wrong slot.  The size is the library's constant, not a choice: the
    wall time is printed."""
    packed, pitch, _ = data
    cnt = 128
    nr, nc = 257, 2184 * 256 + 1
    assert -(-nr // 256) * -(-nc // 256) == 4370 > (4 << 30) // (15 * 65536) == 4369
    rows = draw(nr, 61)
    cols = np.random.RandomState(62).randint(0, n, size=nc).astype(np.uint64)
    Kw = whole(cnt)
    t0 = time.perf_counter()
    K = _session(packed, pitch, np.float64, [(0, cnt)], rows, cols)
    t1 = time.perf_counter()
    Krows = Kw[rows.astype(np.intp)]
    for c0 in range(0, nc, 65536):  # in slabs: never two full copies beside the 1.15 GB result
        sl = slice(c0, min(c0 + 65536, nc))
        assert np.array_equal(K[:, sl], Krows[:, cols[sl].astype(np.intp)]), c0
    print("residue chunks: session %.2f s, compare %.2f s" % (t1 - t0, time.perf_counter() - t1))
