"""DistGen on the GPU (csrc/distgen.hip) against the reference, bit for bit: the reference's own
fixture (tests/golden/data/distgen.dist.npz) and the small shapes of tests/golden/distgen.npz
(tools/make_golden_distgen.py ran the reference's DistGen; nothing is restated here).  Then what is
built on it: dtype and order, selections, ``as_snp()`` and its GRM.

The GRM comparisons carry tests/test_gpu_dist.py's tolerances for the dense-operand GRM (1e-5 of max
diag in float32, 1e-10 in float64, ``grm_close``).  Whole-K against the DistData route and the
chunked against the one-chunk K are asserted within them, not bit for bit: the chunk boundaries of
the two routes differ, so the sums are ordered differently."""
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN
from pysnptools_amd import _grm as G
from pysnptools_amd import hbm
from pysnptools_amd.distreader import DistData, DistGen, DistNpz
from pysnptools_amd.standardizer import Beta, Unit
from test_gpu_dist import same_bits
from test_gpu_parity import grm_close

pytestmark = pytest.mark.gpu

# tag -> (seed, iid_count, sid_count, block_size, SNP selection or None): tools/make_golden_distgen.py
CASES = {"n1_b1": (3, 1, 2, 1, None),
         "n5_b3": (7, 5, 7, 3, None),
         "n257_b2": (1, 257, 4, 2, None),
         "n300_b1": (5, 300, 3, 1, None),
         "n4_b1": (11, 4, 6000, 1, [0, 2999, 5999])}
FIXTURE_SIDS = [0, 1, 200, 2200, 10]
_G = {}


def golden():
    if not _G:
        with np.load(os.path.join(GOLDEN, "distgen.npz"), allow_pickle=False) as z:
            _G.update({k: z[k] for k in z.files})
        for v in _G.values():
            v.setflags(write=False)
    return _G


def case(tag):
    seed, n, m, block, sel = CASES[tag]
    gen = DistGen(seed=seed, iid_count=n, sid_count=m, block_size=block)
    return gen if sel is None else gen[:, sel]


def close(K, Kref, tol):
    """``grm_close`` with both kernels in units of Kref's largest diagonal element: Beta(1, 25) weights
    make K tiny (1e-10 here), and ``grm_close`` does not scale by a diagonal below 1."""
    Kref = np.asarray(Kref, dtype=np.float64)
    scale = np.abs(np.diag(Kref)).max()
    assert np.isfinite(Kref).all() and scale > 0
    grm_close(np.asarray(K, dtype=np.float64) / scale, Kref / scale, tol)


def exact(got, want):
    """Same shape, float64, NaN positions and values (the issue's criterion)."""
    return got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


# ---------------------------------------------------------------------------------- the reference's values
def test_reference_fixture():
    ref = DistNpz(os.path.join(DATA, "distgen.dist.npz")).read().val
    assert np.isnan(ref).any()
    gen = DistGen(seed=0, iid_count=1000, sid_count=10 ** 6, block_size=1000)
    got = gen[:, FIXTURE_SIDS].read()
    assert exact(got.val, ref) and same_bits(got.val, ref)
    sub = gen[::10, FIXTURE_SIDS].read()
    assert exact(sub.val, ref[::10]) and np.array_equal(sub.iid, got.iid[::10])


@pytest.mark.parametrize("tag", sorted(CASES))
def test_small_shapes(tag):
    Gd = golden()
    data = case(tag).read()
    assert exact(data.val, Gd[tag + "_val"]) and same_bits(data.val, Gd[tag + "_val"])
    assert data.val.flags["F_CONTIGUOUS"]
    assert np.array_equal(data.iid, Gd[tag + "_iid"]) and np.array_equal(data.sid, Gd[tag + "_sid"])
    assert np.array_equal(data.pos, Gd[tag + "_pos"])


def test_golden_shapes_are_not_degenerate():
    Gd = golden()
    for tag, nan_pairs in (("n5_b3", 3), ("n257_b2", 96), ("n300_b1", 64)):
        block = CASES[tag][3]
        assert np.isnan(Gd[tag + "_val"][:, :block, 0]).sum() == nan_pairs
    v = Gd["n257_b2_val"]
    assert np.array_equal(np.isnan(v[..., 0]), np.isnan(v[..., 1])) and np.array_equal(np.isnan(v[..., 0]), np.isnan(v[..., 2]))


def test_partial_last_batch():
    """sid_count = 7 in batches of 3: SNP 6 is column 0 of a FULL batch seeded seed + 6."""
    want = golden()["n5_b3_val"]
    seed, n, m, block, _ = CASES["n5_b3"]
    assert m % block == 1
    gen = DistGen(seed=seed, iid_count=n, sid_count=m, block_size=block)
    assert exact(gen[:, 6].read().val, want[:, 6:7])
    # the same stream, read as the first SNP of a longer reader's third batch and of a reader seeded there
    assert exact(DistGen(seed, n, 9, block_size=block)[:, 6].read().val, want[:, 6:7])
    assert exact(DistGen(seed + 6, n, 3, block_size=block)[:, 0].read().val, want[:, 6:7])


def test_column_selection():
    gen = DistGen(seed=7, iid_count=5, sid_count=30, block_size=3)
    whole = gen.read().val
    assert exact(whole[:, :6], golden()["n5_b3_val"][:, :6])
    sel = [29, 0, 4, 4, 3, 17]  # unsorted, a repeat, two SNPs of one batch, single SNPs of others
    for order in ("F", "C"):
        got = gen[:, sel].read(order=order).val
        assert exact(got, whole[:, sel])
    assert exact(gen[[4, 0, 0], :][:, sel].read().val, whole[[4, 0, 0]][:, sel])


def test_more_batches_than_workgroup_slots():
    seed, n, m, block, sel = CASES["n4_b1"]
    gen = DistGen(seed=seed, iid_count=n, sid_count=m, block_size=block)
    whole = gen.read().val
    assert whole.shape == (4, 6000, 3)
    halves = np.concatenate([gen[:, :3000].read().val, gen[:, 3000:].read().val], axis=1)
    assert exact(whole, halves)
    assert exact(whole[:, sel], golden()["n4_b1_val"])
    nan = np.isnan(whole[..., 0]).mean()
    assert 0.19 < nan < 0.25  # (24000 draws at 0.218: 4 sigma is 0.011)


# ---------------------------------------------------------------------------------- dtype, order, HBM
@pytest.mark.parametrize("tag", ["n257_b2", "n5_b3"])
def test_dtype_and_order(tag, monkeypatch):
    want = golden()[tag + "_val"]
    gen = case(tag)
    for dtype in (np.float64, np.float32):
        w = want.astype(dtype)
        for order, flag in (("C", "C_CONTIGUOUS"), ("F", "F_CONTIGUOUS"), ("A", "F_CONTIGUOUS")):
            val = gen.read(order=order, dtype=dtype).val
            assert isinstance(val, np.ndarray) and val.flags[flag] and val.dtype == dtype
            assert same_bits(val, w), (dtype, order)
            dev = gen._generate(np.arange(gen.sid_count), "F" if order == "A" else order, dtype)
            assert isinstance(dev, hbm.HbmArray) and dev.order == ("F" if order == "A" else order)
            assert same_bits(dev.get(), w)
    monkeypatch.setenv("ARRAY_MODULE", "hbm")
    for order in ("C", "F"):
        data = gen.read(order=order, dtype=np.float32)
        assert isinstance(data.val, hbm.HbmArray) and data.val.order == order
        assert same_bits(data.val.get(), want.astype(np.float32))
    sub = gen[::2, 1:].read()
    assert isinstance(sub.val, hbm.HbmArray) and exact(sub.val.get(), want[::2, 1:])


def test_other_dtypes_raise():
    with pytest.raises(ValueError, match="not supported"):
        case("n5_b3").read(dtype=np.int8)


def test_seed_limit_is_checked_by_the_library():
    from pysnptools_amd import _native as N

    out = hbm.empty((5, 1, 3), dtype=np.float64)
    idx = N.index_array([7])
    with pytest.raises(ValueError, match="Seed must be between 0 and"):
        N.call("snpmi_dev_distgen_f64", N.ptr(out), 5, 2 ** 32 - 6, 3, N.ptr(idx), 1, 1)
    N.call("snpmi_dev_distgen_f64", N.ptr(out), 5, 2 ** 32 - 7, 3, N.ptr(idx), 1, 1)  # batch seed 2**32 - 1
    assert exact(out.get(), DistGen(2 ** 32 - 1, 5, 3, block_size=3)[:, 1].read(order="C").val)
    with pytest.raises(ValueError, match="device memory"):
        N.call("snpmi_dev_distgen_f64", N.ptr(np.empty((5, 1, 3))), 5, 0, 3, N.ptr(idx), 1, 1)


# ---------------------------------------------------------------------------------- as_snp
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("w", [2, 1])
def test_as_snp(dtype, w):
    gen = DistGen(seed=1, iid_count=257, sid_count=40, block_size=2)
    val = gen.read(dtype=dtype).val
    assert same_bits(val[:, :4], golden()["n257_b2_val"].astype(dtype))
    want = DistData(gen.iid, gen.sid, val=val).as_snp(max_weight=w).read(dtype=dtype).val
    assert np.isnan(want).any() and not np.isnan(want).all()
    for block in (None, 3):
        for order in ("F", "C"):
            got = gen.as_snp(max_weight=w, block_size=block).read(dtype=dtype, order=order).val
            assert isinstance(got, np.ndarray) and got.flags[order + "_CONTIGUOUS"]
            assert same_bits(got, want), (block, order)
            dev = gen.as_snp(max_weight=w, block_size=block).read(dtype=dtype, order=order, xp="hbm").val
            assert isinstance(dev, hbm.HbmArray) and dev.order == order and same_bits(dev.get(), want)
    # (40 SNPs <= 257 iids convert whole whatever block_size is: _dist2snp.py:49; blocks need more SNPs than iids)
    wide = DistGen(seed=7, iid_count=5, sid_count=30, block_size=3)
    wval = wide.read(dtype=dtype).val
    wwant = DistData(wide.iid, wide.sid, val=wval).as_snp(max_weight=w).read(dtype=dtype).val
    for order in ("F", "C"):
        assert same_bits(wide.as_snp(max_weight=w, block_size=4).read(dtype=dtype, order=order).val, wwant)
        dev = wide.as_snp(max_weight=w, block_size=4).read(dtype=dtype, order=order, xp="hbm").val
        assert isinstance(dev, hbm.HbmArray) and dev.order == order and same_bits(dev.get(), wwant)
    sel = [5, 39, 5, 0]
    assert same_bits(gen[:, sel].as_snp(max_weight=w, block_size=3).read(dtype=dtype).val, want[:, sel])
    assert same_bits(gen.as_snp(max_weight=w)[::3, sel].read(dtype=dtype).val, want[::3][:, sel])


# ---------------------------------------------------------------------------------- read_kernel
@pytest.mark.parametrize("dtype,tol", [(np.float32, 1e-5), (np.float64, 1e-10)])
def test_read_kernel(dtype, tol, monkeypatch):
    gen = DistGen(seed=9, iid_count=300, sid_count=512, block_size=8)
    assert G.source_kind(gen.as_snp()) == G.DISTGEN and G.source_kind(gen[:, 3:77].as_snp()) == G.DISTGEN
    assert G.source_kind(gen[::2, :].as_snp()) == G.DIST
    data = DistData(gen.iid, gen.sid, val=gen.read(dtype=dtype).val)
    for std in (Unit(), Beta(1, 25)):
        Kref, tref = data.as_snp()._read_kernel(std, block_size=128, dtype=dtype, return_trained=True)
        K, trained = gen.as_snp()._read_kernel(std, block_size=128, dtype=dtype, return_trained=True)
        assert isinstance(K, np.ndarray) and K.dtype == dtype and np.array_equal(K, K.T)
        close(K, Kref, tol)
        # the same conversion and standardize kernels on the same values: identical stats
        assert same_bits(np.asarray(trained.stats), np.asarray(tref.stats))
        assert np.array_equal(gen.as_snp().read_kernel(std, block_size=128, dtype=dtype).val, K)
        # the trained standardizer of the first call applied in a second
        close(gen.as_snp()._read_kernel(trained, block_size=128, dtype=dtype), Kref, tol)
        # a SNP range that starts inside a batch, and an iid subset (the generic block loop)
        sub = gen[:, 3:77].as_snp().read_kernel(std, dtype=dtype).val
        close(sub, data[:, 3:77].as_snp().read_kernel(std, dtype=dtype).val, tol)
        few = gen[::2, :].as_snp().read_kernel(std, dtype=dtype).val
        close(few, data[::2, :].as_snp().read_kernel(std, dtype=dtype).val, tol)
    # several chunks (here: two batches each) against the one-chunk K
    chunks = []
    real = G.Session.add_dist

    def add_dist(self, val, col0, cols, *args):
        chunks.append(cols)
        return real(self, val, col0, cols, *args)

    monkeypatch.setattr(G.Session, "add_dist", add_dist)
    K1 = gen.as_snp()._read_kernel(Unit(), dtype=dtype)
    assert chunks == [512]
    del chunks[:]
    from pysnptools_amd.snpreader.snpreader import _native_grm

    monkeypatch.setattr(G.feed_distgen, "__defaults__", (16 * 3 * 300 * np.dtype(dtype).itemsize,))
    Kc = _native_grm(gen.as_snp(), Unit(), np.dtype(dtype), None, False)[0]
    assert chunks == [16] * 32
    close(Kc, K1, tol)
    del chunks[:]
    monkeypatch.setattr(G.feed_distgen, "__defaults__", (1,))  # never less than one batch
    Kb = _native_grm(gen[:, :100].as_snp(), Unit(), np.dtype(dtype), None, False)[0]
    assert chunks == [8] * 12 + [4]
    close(Kb, data[:, :100].as_snp().read_kernel(Unit(), dtype=dtype).val, tol)


def test_feed_distgen_takes_chunk_bytes():
    import inspect

    assert list(inspect.signature(G.feed_distgen).parameters)[-1] == "chunk_bytes"
    assert list(inspect.signature(G.feed_snpgen).parameters)[-1] == "chunk_bytes"


# ---------------------------------------------------------------------------------- empty
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_empty_selections(dtype):
    gen = DistGen(seed=2, iid_count=6, sid_count=9, block_size=2)
    for order, flag in (("F", "F_CONTIGUOUS"), ("C", "C_CONTIGUOUS")):
        v = gen[:, []].read(dtype=dtype, order=order).val
        assert v.shape == (6, 0, 3) and v.dtype == dtype and v.flags[flag]
        v = gen[[], :].read(dtype=dtype, order=order).val
        assert v.shape == (0, 9, 3) and v.dtype == dtype and v.flags[flag]
        none = DistGen(seed=2, iid_count=0, sid_count=9, block_size=2)
        assert none.iid_count == 0
        v = none.read(dtype=dtype, order=order).val
        assert v.shape == (0, 9, 3) and v.dtype == dtype and v.flags[flag]
    sub = gen[:, []].as_snp()
    assert sub.sid_count == 0
    v = sub.read(dtype=dtype).val
    assert v.shape == (6, 0) and v.dtype == dtype
    K = sub.read_kernel(Unit(), dtype=dtype).val
    assert K.shape == (6, 6) and K.dtype == dtype and not K.any()
