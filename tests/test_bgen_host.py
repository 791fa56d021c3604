"""Bgen without a GPU: the native index scan, the metadata the reference pins (bgen.py:651-690,
791-846, 861-879), every refusal, ``Bgen.write``'s bytes and the GRM route it takes.  Values are
checked against the independent decoder of ``bgen_ref``; the GPU decode is in test_gpu_bgen.py."""
import os
import shutil
import struct

import numpy as np
import pytest

import bgen_ref as R
from conftest import DATA
from pysnptools_amd import _grm as G
from pysnptools_amd import _native as N
from pysnptools_amd.distreader import Bgen, DistData
from pysnptools_amd.distreader import bgen as bgen_mod
from pysnptools_amd.standardizer import Unit

EXAMPLE = os.path.join(DATA, "example.bgen")
BIG = os.path.join(DATA, "2500x100.bgen")
BITS1 = os.path.join(DATA, "bits1.bgen")
FIXTURES = [EXAMPLE, BIG, BITS1]


# ------------------------------------------------------------------------- metadata pins
def test_example_metadata():
    bgen = Bgen(EXAMPLE)
    assert (bgen.iid_count, bgen.sid_count) == (500, 199)
    assert tuple(bgen.iid[0]) == ("0", "sample_001") and bgen.iid[-1, 1].endswith("sample_500")
    assert bgen.sid[0] == "SNPID_2,RSID_2"
    assert tuple(bgen.pos[0]) == (1, 0, 2000) and bgen.pos[7, 2] == 9000 and bgen.pos[-1, 2] == 100001
    assert bgen.pos.dtype == np.float64 and bgen.pos.shape == (199, 3)
    assert repr(bgen) == "Bgen('{0}')".format(EXAMPLE)
    by_id = Bgen(EXAMPLE, sid_function="id")
    assert by_id.sid[0] == "SNPID_2" and by_id.sid[7] == "SNPID_9" and by_id.sid[-1] == "SNPID_200"
    assert Bgen(EXAMPLE, sid_function="rsid").sid[0] == "RSID_2"


def test_functions_and_sample_file():
    doubled = Bgen(EXAMPLE, iid_function=lambda s: (s, s), sid_function=lambda i, r: r + "/" + i)
    assert tuple(doubled.iid[0]) == ("sample_001", "sample_001") and doubled.sid[0] == "RSID_2/SNPID_2"
    other = Bgen(EXAMPLE, sample=os.path.join(DATA, "other.sample"))
    assert tuple(other.iid[0]) == ("0", "other_001") and other.iid_count == 500


def test_all_zero_rsids_give_the_ids():
    bgen = Bgen(BIG)
    assert (bgen.iid_count, bgen.sid_count) == (2500, 100)
    assert bgen.sid[0] == "sid_0" and bgen.pos[0, 2] == 9270273


def test_properties_are_fresh_and_flush_reopens():
    bgen = Bgen(BITS1, fresh_properties=False)
    assert bgen.iid.flags["OWNDATA"] and bgen.sid.flags["OWNDATA"] and bgen.pos.flags["OWNDATA"]
    bgen.flush()
    assert bgen.iid_count == 500
    bgen.flush()


def test_no_sample_block_numbers_the_samples(tmp_path):
    block = R.make_block([[1, 2], [3, 0], [0, 0]], 2)
    bgen = Bgen(R.make_file(str(tmp_path / "ns.bgen"), [block], 3, samples=False))
    assert [tuple(r) for r in bgen.iid] == [("0", "sample_0"), ("0", "sample_1"), ("0", "sample_2")]


def test_chromosome_text_and_mixed_rsids(tmp_path):
    block = R.make_block([[1, 2]], 2)
    bgen = Bgen(R.make_file(str(tmp_path / "c.bgen"), [block] * 3, 1, chroms=["01", "X", "22"], rsids=["0", "rs1", ""]))
    assert bgen.pos.tolist() == [[1, 0, 100], [0, 0, 101], [22, 0, 102]]
    assert list(bgen.sid) == ["v0,0", "v1,rs1", "v2,"]  # file-wide rule: not every rsid is "0" (or "")
    same = Bgen(R.make_file(str(tmp_path / "e.bgen"), [block] * 2, 1, rsids=["", ""]))
    assert list(same.sid) == ["v0", "v1"]


def test_default_functions():
    assert bgen_mod.default_iid_function("fam0,ind0") == ("fam0", "ind0")
    assert bgen_mod.default_iid_function("ind0") == ("0", "ind0")
    assert bgen_mod.default_sid_function("SNP1", "rs102343") == "SNP1,rs102343"
    assert bgen_mod.default_sid_function("SNP1", "0") == "SNP1"
    assert bgen_mod.default_sample_function("fam0", "ind0") == "fam0,ind0"
    assert bgen_mod.default_sample_function("0", "ind0") == "ind0"
    assert bgen_mod.default_id_rsid_function("SNP1,rs102343") == ("SNP1", "rs102343")
    assert bgen_mod.default_id_rsid_function("SNP1") == ("SNP1", "0")


def test_comma_samples_split(tmp_path):
    from pysnptools_amd.distreader import DistData

    val = np.zeros((2, 1, 3))
    val[:, :, 0] = 1
    dd = DistData(iid=[["f", "a"], ["0", "b"]], sid=["s"], val=val, pos=[[1, 0, 5]])
    bgen = Bgen.write(str(tmp_path / "w.bgen"), dd, bits=8)
    header, _ = R.walk(bgen.filename)
    assert header["samples"] == ["f,a", "b"]
    assert [tuple(r) for r in bgen.iid] == [("f", "a"), ("0", "b")]


# ------------------------------------------------------------------------- the native index scan
@pytest.mark.parametrize("path", FIXTURES)
def test_index_scan_matches_the_python_walk(path):
    header, variants = R.walk(path)
    bgen = Bgen(path)
    bgen._run_once()
    assert (bgen._rec.shape[0], bgen._n, bgen._flags) == (header["m"], header["n"], header["flags"])
    assert header["layout"] == 2 and header["compression"] == 1
    for name, col in (("offset", 0), ("stored", 1), ("inflated", 2), ("pos", 3)):
        assert list(bgen._rec[:, col]) == [v[name] for v in variants], name
    assert list(bgen._rec[:, 4]) == [len(v["alleles"]) for v in variants]
    assert list(bgen._ids) == [v["id"] for v in variants] and list(bgen._rsids) == [v["rsid"] for v in variants]
    assert list(bgen._alleles) == [",".join(v["alleles"]) for v in variants]
    assert list(bgen._samples) == header["samples"]
    assert list(bgen._chroms) == [v["chrom"] for v in variants]
    assert list(bgen.pos[:, 0]) == [int(v["chrom"]) for v in variants] and not bgen.pos[:, 1].any()
    info = (N.ctypes.c_uint64 * 11)()
    N.call("snpmi_bgen_open", path.encode(), info)
    assert int(info[10]) == os.path.getsize(path) and int(info[4]) == 1
    assert int(info[6]) == max(len(v["id"]) for v in variants)


@pytest.mark.parametrize("path", FIXTURES)
def test_inflated_blocks_pass_the_host_checks(path):
    header, variants = R.walk(path)
    bgen = Bgen(path)
    bgen._run_once()
    for j in (0, len(variants) - 1):
        data, bits = bgen._inflate(j)
        assert data == R.inflate(header, variants[j]) and bits == data[9 + header["n"]]
    assert bits == {EXAMPLE: 32, BIG: 16, BITS1: 1}[path]


def test_the_reference_digit_pins_on_the_python_decoder():
    """bgen.py:861-898.  The first two components of both pins, and the third of the first, are what
    the formula gives; the second pin's third component differs from it in the last bits only."""
    val = R.decode_file(EXAMPLE)
    assert np.all(np.isnan(val[0, 0]))
    np.testing.assert_array_almost_equal(val[1, 0], [0.027802362811705648, 0.00863673794284387, 0.9635608992454505])
    np.testing.assert_array_almost_equal(val[2, 1], [0.97970582847010945, 0.01947019668749305,
                                                     0.00082397484239749366])
    D = 2.0 ** 32 - 1
    assert val[1, 0, 0] == 119410239 / D and val[1, 0, 1] == 37094507 / D
    assert val[2, 1, 0] == 4207804492 / D and val[2, 1, 1] == 83623858 / D
    assert val[1, 0, 2] == 0.9635608992454505


# ------------------------------------------------------------------------- refusals
def _good(n=3):
    return R.make_block([[1, 2]] * n, 2)


def _bits_byte(bits):
    """A good 3-sample block (flags at bytes 8 ... 10, phased at 11) with another bit depth at byte 12."""
    good = _good()
    return good[:12] + bytes([bits]) + good[13:]


def test_missing_file_raises_on_first_use():
    bgen = Bgen(os.path.join(DATA, "no_such_file.bgen"))  # the constructor opens nothing
    with pytest.raises(Exception, match="no_such_file"):
        bgen.iid


@pytest.mark.parametrize("kwargs, match", [({"layout": 1}, "layout 1"), ({"compression": 2}, "zstd")])
def test_header_refusals(tmp_path, kwargs, match):
    path = R.make_file(str(tmp_path / "h.bgen"), [_good()], 3, **kwargs)
    with pytest.raises(ValueError, match=match):
        Bgen(path).iid


@pytest.mark.parametrize("truncate", [1, 20, 40])  # variant 1 is 45 bytes
def test_truncated_file(tmp_path, truncate):
    path = R.make_file(str(tmp_path / "t.bgen"), [_good(), _good()], 3, truncate=truncate)
    with pytest.raises(ValueError, match="truncated.*variant 1"):
        Bgen(path).sid


def test_three_alleles_are_refused_from_the_index(tmp_path):
    path = R.make_file(str(tmp_path / "k.bgen"), [_good(), _good()], 3, k=3)
    bgen = Bgen(path)
    assert bgen.sid_count == 2  # the metadata reads
    with pytest.raises(ValueError, match="variant 1.*3 alleles"):
        bgen._check([1])


@pytest.mark.parametrize("block, match", [
    (R.make_block([[1, 2]] * 3, 2, k=3), "3 alleles"),
    (R.make_block([[1, 2]] * 3, 2, phased=1), "phased"),
    (R.make_block([[1, 2]] * 3, 2, ploidy=1), "diploid"),
    (R.make_block([[1, 2]] * 3, 2, n_field=4), "4 samples"),
    (R.make_block([[1, 2]] * 3, 2, extra=b"\0"), "16 bytes.*need 15"),
    (R.make_block([[1, 2]] * 3, 2)[:-1], "14 bytes.*need 15"),
    (_bits_byte(40), "40 bits"),
    (_bits_byte(0), "0 bits"),
])
@pytest.mark.parametrize("compression", [0, 1])
def test_block_refusals(tmp_path, block, match, compression):
    path = R.make_file(str(tmp_path / "b.bgen"), [_good(), block], 3, compression=compression)
    bgen = Bgen(path)
    bgen._run_once()
    bgen._inflate(0)
    with pytest.raises(ValueError, match="variant 1.*" + match):
        bgen._inflate(1)


def test_wrong_inflated_length(tmp_path):
    path = R.make_file(str(tmp_path / "l.bgen"), [_good()], 3, compression=1, inflated_lie=2)
    bgen = Bgen(path)
    with pytest.raises(ValueError, match="inflates to 15 bytes, its header says 17"):
        bgen._inflate(0) if bgen.sid_count else None


def test_one_missing_sample_flag_with_odd_ploidy_bits(tmp_path):
    good = bytearray(_good())
    good[9] = 0x83  # sample 1: missing, ploidy 3
    path = R.make_file(str(tmp_path / "p.bgen"), [bytes(good)], 3)
    bgen = Bgen(path)
    with pytest.raises(ValueError, match="diploid"):
        bgen._inflate(0) if bgen.sid_count else None


# ------------------------------------------------------------------------- Bgen.write
def _dist(n, m, seed=0, missing=()):
    rng = np.random.default_rng(seed)
    val = rng.dirichlet((1, 1, 1), size=(n, m))
    for i, j in missing:
        val[i, j] = np.nan
    return DistData(iid=[["0", "i%d" % i] for i in range(n)], sid=["s%d" % j for j in range(m)], val=val,
                    pos=[[1 + j, 0, 10 * j] for j in range(m)])


@pytest.mark.parametrize("bits", [1, 2, 3, 8, 16, 17, 31, 32])
@pytest.mark.parametrize("compression", [None, "zlib"])
def test_write_is_read_back_by_the_python_decoder(tmp_path, bits, compression):
    dd = _dist(7, 3, seed=bits, missing=[(0, 0), (6, 2), (3, 1)])
    dd.val[1, 1] = 0  # a triple summing to 0 is written as missing
    bgen = Bgen.write(str(tmp_path / "w.bgen"), dd, bits=bits, compression=compression)
    assert isinstance(bgen, Bgen) and os.listdir(tmp_path) == ["w.bgen"]  # nothing beside the file
    header, variants = R.walk(bgen.filename)
    assert (header["layout"], header["compression"], header["n"], header["m"]) == (2, 1 if compression else 0, 7, 3)
    assert [v["id"] for v in variants] == ["s0", "s1", "s2"] and [v["rsid"] for v in variants] == ["0"] * 3
    assert [v["pos"] for v in variants] == [0, 10, 20] and [v["chrom"] for v in variants] == ["1", "2", "3"]
    back = R.decode_file(bgen.filename)
    want = dd.val.copy()
    want[1, 1] = np.nan
    assert np.array_equal(np.isnan(back), np.isnan(want))
    # largest remainder keeps every component within (2/3) / (2^b - 1) (+ the rounding of p * D)
    bound = (2 / 3) / (2 ** bits - 1) + 4e-16
    assert np.nanmax(np.abs(back - want)) <= bound
    D = 2 ** bits - 1
    ok = ~np.isnan(back[..., 0])
    ints = np.rint(back[ok] * D)
    assert np.all(ints >= 0) and np.all(ints.sum(axis=1) == D)  # the three integers sum to D exactly
    assert list(bgen.sid) == ["s0", "s1", "s2"] and tuple(bgen.iid[0]) == ("0", "i0")


def test_write_ties_go_to_the_lower_index(tmp_path):
    # bits = 1: D = 1, v = p: (1/3, 1/3, 1/3) -> floor 0, one unit to component 0; (0.5, 0.5, 0) -> component 0
    val = np.array([[[1 / 3, 1 / 3, 1 / 3]], [[0.5, 0.5, 0]], [[0, 0.5, 0.5]], [[0.25, 0.25, 0.5]]])
    dd = DistData(iid=[["0", str(i)] for i in range(4)], sid=["s"], val=val, pos=[[1, 0, 1]])
    back = R.decode_file(Bgen.write(str(tmp_path / "t.bgen"), dd, bits=1).filename)
    assert back[:, 0, :].tolist() == [[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]


def test_write_refusals(tmp_path):
    path = str(tmp_path / "r.bgen")
    dd = _dist(3, 2)
    with pytest.raises(ValueError, match="zstd"):
        Bgen.write(path, dd, compression="zstd")
    with pytest.raises(ValueError, match="bits"):
        Bgen.write(path, dd, bits=33)
    for bad in ([0.5, 0.6, 0.0], [-0.1, 0.6, 0.5], [0.3, 0.3, 0.3]):  # the cases of the reference's test_bad_sum
        dd = _dist(3, 2)
        dd.val[1, 1] = bad
        with pytest.raises(ValueError, match="sum to 1"):
            Bgen.write(path, dd)
    dd = _dist(3, 2)
    dd.val[1, 1] = [0.5, 0.5 + 5e-7, 0.0]  # within 1e-6: written
    Bgen.write(path, dd, qctool_path="ignored", cleanup_temp_files=False)


def test_write_to_a_read_only_directory_of_inputs_leaves_no_sidecar(tmp_path):
    shutil.copy(BITS1, str(tmp_path / "in.bgen"))
    os.chmod(str(tmp_path / "in.bgen"), 0o444)
    bgen = Bgen(str(tmp_path / "in.bgen"))
    assert bgen.sid_count == 1 and os.listdir(tmp_path) == ["in.bgen"]


# ------------------------------------------------------------------------- the GRM route
def test_route_is_bgen_for_all_iids_and_the_block_loop_for_an_iid_subset():
    from pysnptools_amd.snpreader.snpreader import _native_grm, _resolve

    bgen = Bgen(BIG)
    for reader in (bgen.as_snp(), bgen[:, 5:50].as_snp(), bgen[:, [7, 3, 3]].as_snp(max_weight=1)):
        base, rows, _ = _resolve(reader)
        assert G.source_kind(base, rows) == G.BGEN
    p = G.plan(bgen[:, [7, 3, 3]].as_snp(), Unit(), np.float32)
    assert p.source == G.BGEN and p.src[0] is bgen and list(p.src[1]) == [7, 3, 3] and (p.n, p.m) == (2500, 3)
    subset = bgen[::2, :].as_snp()
    base, rows, _ = _resolve(subset)
    assert G.source_kind(base, rows) == G.DIST
    assert _native_grm(subset, Unit(), np.dtype(np.float64), None, False) is None  # the generic block loop


def test_chunks_respect_both_bounds():
    bgen = Bgen(BIG)
    bgen._run_once()
    cols = np.arange(100)
    one = list(bgen._chunks(cols, 2500, 4, G.BGEN_CHUNK_BYTES))
    assert one == [slice(0, 100)]
    staged = int(bgen_mod._round8(bgen._rec[:, 2]).sum())
    three = list(bgen._chunks(cols, 1, 4, staged // 3 + 12512 + 16))  # (one row: the staged blocks alone bound it)
    assert len(three) == 3 and three[0].start == 0 and three[-1].stop == 100
    assert all(a.stop == b.start for a, b in zip(three, three[1:]))
    by_out = list(bgen._chunks(cols, 2500, 8, 3 * 2500 * 8 * 40))  # 40 columns of triples
    assert [c.stop - c.start for c in by_out] == [40, 40, 20]
    assert list(bgen._chunks(cols[:2], 2500, 8, 1)) == [slice(0, 1), slice(1, 2)]  # never empty


def test_abi_is_declared_and_bound():
    for name in ("snpmi_bgen_open", "snpmi_bgen_index", "snpmi_dev_bgen_decode_f32", "snpmi_dev_bgen_decode_f64"):
        assert name in N.symbols() and hasattr(N.lib(), name)
    # no device: an empty decode launches nothing and needs none
    N.call("snpmi_dev_bgen_decode_f32", None, 0, None, 0, None, 5, None, 0, 0, 0)
    with pytest.raises(IndexError):
        N.call("snpmi_dev_bgen_decode_f32", None, 0, None, 3, None, 5, None, 2, 0, 0)
    assert struct.calcsize("<QII") == 16  # the kernel's column table entry


def test_every_truncation_of_a_small_file_is_refused(tmp_path):
    """The native walk never reads past the end: each proper prefix raises, the whole file reads."""
    whole = R.make_file(str(tmp_path / "w.bgen"), [_good(), _good()], 3, compression=1)
    size = os.path.getsize(whole)
    assert Bgen(whole).sid_count == 2
    for cut in range(1, size + 1):
        path = R.make_file(str(tmp_path / "c.bgen"), [_good(), _good()], 3, compression=1, truncate=cut)
        assert os.path.getsize(path) == size - cut
        with pytest.raises(ValueError):
            Bgen(path).sid_count


@pytest.mark.parametrize("order", ["F", "C", "A"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_empty_selections_need_no_device(dtype, order):
    bgen = Bgen(EXAMPLE)
    for sel, shape in (((slice(None), []), (500, 0, 3)), (([], slice(None)), (0, 199, 3)), (([], []), (0, 0, 3))):
        data = bgen[sel[0], sel[1]].read(dtype=dtype, order=order)
        assert data.val.shape == shape and data.val.dtype == dtype and isinstance(data.val, np.ndarray)
        assert (data.iid_count, data.sid_count) == shape[:2]
    assert bgen[:, []].as_snp().read(dtype=dtype).val.shape == (500, 0)
