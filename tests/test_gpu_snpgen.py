"""SnpGen on the GPU: the MT19937 stream against numpy, the generated values bit for bit against
the reference's (goldens made by tools/make_golden.py and tools/make_golden_snpgen.py), subsets,
and the fused standardize / GRM / HBM paths at the tolerances of tests/test_gpu_parity.py."""
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN
from pysnptools_amd import _native as N
from pysnptools_amd import hbm
from pysnptools_amd.kernelreader import SnpKernel
from pysnptools_amd.snpreader import Bed, SnpGen, SnpReader
from pysnptools_amd.standardizer import Beta, Unit
from test_gpu_parity import grm_close, rel_close

pytestmark = pytest.mark.gpu

BIG_SID = [0, 1, 200, 2200, 10]
_cache = {}


def g(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    return _cache[name]


def from_i8(v, dtype):
    out = v.astype(dtype)
    out[v == -127] = np.nan
    return out


def case(name):
    """(reader of the case's SNPs, expected int8 values), built once."""
    key = "case:" + name
    if key not in _cache:
        if name == "big":    # two batches of 3 rounds, an unsorted index
            gen = SnpGen(seed=0, iid_count=1000, sid_count=1000 * 1000, block_size=1000)[:, BIG_SID]
            exp = g("snpgen")["val_i8"]
        elif name == "dist":  # the default block (1000) is wider than sid_count
            gen, exp = SnpGen(seed=0, iid_count=100, sid_count=100), g("dist_x")["val_i8"]
        else:
            C = g("snpgen_cases")
            seed, n, m, block = (int(x) for x in C[name + "_params"])
            gen = SnpGen(seed=seed, iid_count=n, sid_count=m, block_size=block or None)[:, C[name + "_sid"]]
            exp = C[name + "_val_i8"]
        _cache[key] = (gen, exp)
    return _cache[key]


# ---------------------------------------------------------------------------------- 1. raw stream
@pytest.mark.parametrize("seed", [0, 1, 5489, 2 ** 32 - 1])
def test_raw_stream_is_numpys(seed):
    """1255 doubles = 2510 words: four regenerations, the last one left mid-state."""
    out = hbm.empty((1255, 1), dtype=np.float64)
    N.call("snpmi_dev_mt19937_random_sample", seed, 1255, N.ptr(out))
    exp = np.random.RandomState(seed).random_sample(1255)
    assert np.array_equal(out.get().reshape(-1).view(np.uint64), exp.view(np.uint64))


# ---------------------------------------------------------------------------------- 2. values
@pytest.mark.parametrize("name", ["big", "dist", "b8", "tiny", "upper", "long", "n32", "b100"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", ["F", "C"])
def test_values_bit_exact(name, dtype, order):
    gen, exp = case(name)
    got = gen.read(order=order, dtype=dtype).val
    assert got.dtype == dtype and got.shape == exp.shape and got.flags[order + "_CONTIGUOUS"]
    assert np.array_equal(np.isnan(got), exp == -127)
    assert np.array_equal(got, from_i8(exp, dtype), equal_nan=True)


def test_values_match_the_reference_bed_files_and_int8():
    gen, exp = case("big")
    ref = Bed(os.path.join(DATA, "snpgen.bed"), count_A1=False).read().val
    assert np.array_equal(gen.read().val, ref, equal_nan=True)
    assert np.array_equal(gen.read(dtype=np.int8, _require_float32_64=False).val, exp)
    gen, _ = case("dist")
    ref = Bed(os.path.join(DATA, "dist_x.bed"), count_A1=False).read().val
    assert np.array_equal(gen.read().val, ref, equal_nan=True)


def test_upper_bound_on_the_allele_count_is_live():
    """At iid_count=2 a SNP with c_j in {3, 4} is rejected; the golden is the reference's output."""
    gen, exp = case("upper")
    val = gen.read().val
    assert np.nansum(val, axis=0).max() <= 2 and np.nansum(val, axis=0).min() >= 1
    assert np.array_equal(val, from_i8(exp, np.float64), equal_nan=True)


# ---------------------------------------------------------------------------------- 3. subsets, re-reads
def test_subsets_and_rereads():
    gen = SnpGen(seed=7, iid_count=37, sid_count=50, block_size=8)
    full = from_i8(g("snpgen_cases")["b8_val_i8"], np.float64)
    for order in ("F", "C"):
        got = gen[::-3, [5, 2, 2, 40]].read(order=order).val
        assert np.array_equal(got, full[::-3][:, [5, 2, 2, 40]], equal_nan=True)
        assert got.flags[order + "_CONTIGUOUS"]
    mask = np.arange(37) % 5 != 1
    assert np.array_equal(gen[mask, 3:29].read(dtype=np.float32).val, full[mask, 3:29].astype(np.float32),
                          equal_nan=True)
    a, b = gen.read().val, gen.read().val
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, full, equal_nan=True)
    assert np.array_equal(gen[:, 49:50].read().val, full[:, 49:50], equal_nan=True)  # the batch past sid_count


@pytest.mark.parametrize("n,m,block", [(37, 50, 8), (1000, 600, 100)])
def test_tiny_scratch_forces_batch_groups_same_bits(n, m, block):
    gen = SnpGen(seed=7, iid_count=n, sid_count=m, block_size=block)
    sid = np.r_[np.arange(m)[::-1], [3, 3, 0]]
    a, pitch = gen._packed(sid)
    a = a.get()
    gen._scratch_bytes = 1  # one batch per group
    b = gen._packed(sid)[0].get()
    assert np.array_equal(a, b)
    assert not a[:, (n + 3) // 4:].any()  # the pad bytes of the pitch are zero
    if n % 4:
        assert not (a[:, n // 4] >> (2 * (n % 4))).any()  # and the pad iids of the last byte


# ---------------------------------------------------------------------------------- 4. fused paths
@pytest.mark.parametrize("tag,dtype,tol", [("f64", np.float64, 1e-10), ("f32", np.float32, 1e-5)])
@pytest.mark.parametrize("order", ["F", "C"])
def test_standardize_vs_reference(tag, dtype, tol, order):
    for name, keys in (("big", ("unit", "beta")), ("dist", ("unit",))):
        gen, _ = case(name)
        G = g("snpgen" if name == "big" else "dist_x")
        for key in keys:
            std = Unit() if key == "unit" else Beta(1, 25)
            d, tr = gen.read(order=order, dtype=dtype).standardize(std, return_trained=True)
            rel_close(d.val, G["%s_%s" % (key, tag)], tol)
            rel_close(tr.stats, G["%s_stats_%s" % (key, tag)], tol)
            # the one-step form (stats from the code counts, decode through the per-SNP table)
            d2, tr2 = SnpReader._as_snpdata(gen, std, False, order, dtype, None)
            assert d2.val.dtype == dtype and d2.val.flags[order + "_CONTIGUOUS"]
            rel_close(d2.val, G["%s_%s" % (key, tag)], tol)
            rel_close(tr2.stats, G["%s_stats_%s" % (key, tag)], tol)
            # and its trained form reproduces it
            d3, _ = SnpReader._as_snpdata(gen, tr2, False, order, dtype, None)
            rel_close(d3.val, d2.val, tol)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-5)])
def test_grm_vs_reference_and_bed(dtype, tol):
    gen = SnpGen(seed=0, iid_count=100, sid_count=100)
    bed = Bed(os.path.join(DATA, "dist_x.bed"), count_A1=False)
    D = g("dist_x")
    K = gen.read_kernel(Unit(), dtype=dtype).val
    assert K.dtype == dtype and K.shape == (100, 100)
    grm_close(K, D["K_unit"], tol)
    assert np.array_equal(K, bed.read_kernel(Unit(), dtype=dtype).val)  # same codes, same kernels
    grm_close(gen.read_kernel(Beta(1, 25), block_size=7, dtype=dtype).val, D["K_beta"], tol)
    assert np.array_equal(SnpKernel(gen, Unit()).read(dtype=dtype).val, K)
    # any sid subset of an all-iid reader streams packed batches too; iid subsets take the block loop
    sub = [40, 3, 99, 3]
    assert np.array_equal(gen[:, sub].read_kernel(Unit(), dtype=dtype).val,
                          bed[:, sub].read_kernel(Unit(), dtype=dtype).val)
    grm_close(gen[::2, :].read_kernel(Unit(), dtype=dtype).val, bed[::2, :].read_kernel(Unit(), dtype=dtype).val, tol)


def test_grm_never_reads_values(monkeypatch):
    """The GRM of an all-iid SnpGen goes packed -> session: no float read of the values."""
    gen = SnpGen(seed=0, iid_count=100, sid_count=100)
    monkeypatch.setattr(SnpGen, "_read", lambda *a, **k: pytest.fail("values were read"))
    monkeypatch.setattr(SnpGen, "_decode", lambda *a, **k: pytest.fail("values were decoded"))
    grm_close(gen[:, 10:90].read_kernel(Unit()).val,
              Bed(os.path.join(DATA, "dist_x.bed"), count_A1=False)[:, 10:90].read_kernel(Unit()).val, 1e-10)


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int8])
def test_read_into_hbm(order, dtype):
    for name in ("dist", "b8", "n32"):  # n32: F order decodes in place; the others drop pad rows
        gen, _ = case(name)
        host = gen.read(order=order, dtype=dtype, _require_float32_64=False).val
        dev = gen.read(order=order, dtype=dtype, _require_float32_64=False, xp="hbm").val
        assert isinstance(dev, hbm.HbmArray) and dev.shape == host.shape and dev.order == order
        assert np.array_equal(dev.get(), host, equal_nan=True)
    gen = SnpGen(seed=7, iid_count=37, sid_count=50, block_size=8)[::-3, [5, 2, 2, 40]]
    dev = gen.read(order=order, dtype=dtype, _require_float32_64=False, xp="hbm").val
    assert isinstance(dev, hbm.HbmArray) and dev.order == order
    assert np.array_equal(dev.get(), gen.read(order=order, dtype=dtype, _require_float32_64=False).val, equal_nan=True)


def _no_value_copies(monkeypatch, limit):
    """HbmArray.get (which numpy conversion goes through too) fails for anything larger than
    ``limit`` elements: the per-SNP stats are small, the values are not."""
    real = hbm.HbmArray.get

    def get(self, order=None):
        if self.size > limit:
            pytest.fail("a %s HbmArray was copied to the host" % (self.shape,))
        return real(self, order)

    monkeypatch.setattr(hbm.HbmArray, "get", get)


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int8])
def test_hbm_read_never_copies_values_to_the_host(monkeypatch, order, dtype):
    """read(xp='hbm') of an all-iid reader, and of a float iid subset, stays in HBM for every iid
    count: 100 and 37 iids leave pad rows behind an F-order decode, 32 do not."""
    expected = {}
    readers = [case("dist")[0], case("b8")[0], case("n32")[0]]
    if dtype != np.int8:
        readers.append(SnpGen(seed=7, iid_count=37, sid_count=50, block_size=8)[::-3, [5, 2, 2, 40]])
    for k, gen in enumerate(readers):
        expected[k] = gen.read(order=order, dtype=dtype, _require_float32_64=False).val
    with monkeypatch.context() as mp:
        _no_value_copies(mp, 0)
        devs = [gen.read(order=order, dtype=dtype, _require_float32_64=False, xp="hbm").val for gen in readers]
    for k, dev in enumerate(devs):
        assert isinstance(dev, hbm.HbmArray) and dev.order == order
        assert np.array_equal(dev.get(), expected[k], equal_nan=True)


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hbm_read_and_standardize_never_copies_values_to_the_host(monkeypatch, order, dtype):
    """The one-step read + standardize under ARRAY_MODULE=hbm: only the [m][2] stats come back."""
    gen, _ = case("dist")
    host, tr_host = SnpReader._as_snpdata(gen, Unit(), False, order, dtype, None)
    monkeypatch.setenv("ARRAY_MODULE", "hbm")
    with monkeypatch.context() as mp:
        _no_value_copies(mp, 2 * gen.sid_count)
        dev, tr_dev = SnpReader._as_snpdata(gen, Unit(), False, order, dtype, None)
    assert isinstance(dev.val, hbm.HbmArray) and dev.val.order == order
    assert np.array_equal(dev.val.get(), host.val, equal_nan=True)
    assert np.array_equal(tr_dev.stats, tr_host.stats)


def test_grm_checks_every_seed_before_the_session_opens(monkeypatch):
    """A batch seed past 2**32 - 1 in a later chunk raises before anything is launched."""
    from pysnptools_amd.snpreader import snpreader as mod

    gen = SnpGen(seed=2 ** 32 - 50, iid_count=20, sid_count=100, block_size=10)  # batches 5.. are out of range
    one_chunk = gen[:, :40].read_kernel(Unit()).val
    calls = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    monkeypatch.setattr(mod._snpgen_grm, "__defaults__", (64 * 10,))  # chunk_bytes: one batch per chunk
    with pytest.raises(ValueError, match=r"Seed must be between 0 and 2\*\*32 - 1"):
        gen.read_kernel(Unit())
    assert not any(c.startswith(("snpmi_grm_", "snpmi_dev_snpgen")) for c in calls)
    grm_close(gen[:, :40].read_kernel(Unit()).val, one_chunk, 1e-10)  # four chunks, the same K
    assert calls.count("snpmi_dev_snpgen_bed") == 4
