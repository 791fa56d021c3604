"""SnpOperator (pysnptools_amd.linop) and its two C-ABI entries, as far as no device is needed: which
sources it takes, the operand checks that come before any device work, result shapes of empty
products, and the ctypes binding."""
import ctypes
import os

import numpy as np
import pytest

from conftest import DATA, has_gpu_device
from pysnptools_amd import _native as N
from pysnptools_amd.snpreader import Bed, SnpData, SnpGen
from pysnptools_amd.standardizer import Beta, DiagKtoN, Identity, Unit

BED = os.path.join(DATA, "n300.bed")


def _bed():
    return Bed(BED, count_A1=False)


def test_exported_from_the_package():
    import pysnptools_amd
    from pysnptools_amd.linop import MATVEC_CHUNK_BYTES, SEGMENT, SnpOperator

    assert pysnptools_amd.SnpOperator is SnpOperator
    assert MATVEC_CHUNK_BYTES == 1 << 30 and SEGMENT == 256
    with pytest.raises(AttributeError):
        pysnptools_amd.no_such_name


def test_symbols_are_bound():
    lib = N.lib()
    for name, nargs in (("snpmi_dev_packed_tdot", 11), ("snpmi_dev_packed_dot", 12)):
        assert name in N.symbols()
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
        assert fn.argtypes[0] is ctypes.c_void_p and fn.argtypes[5] is ctypes.c_int  # packed, dtype
        assert [fn.argtypes[i] for i in (1, 2, 3, 7, 8, 10)] == [ctypes.c_uint64] * 6


def test_other_sources_raise_type_error():
    from pysnptools_amd.linop import SnpOperator

    data = SnpData(iid=[["f", "a"], ["f", "b"]], sid=["s0", "s1", "s2"], val=np.array([[0., 1, 2], [2, 1, 0]]))
    with pytest.raises(TypeError, match="Bed or a SnpGen"):
        SnpOperator(data, Unit())
    with pytest.raises(TypeError, match="Bed or a SnpGen"):
        SnpOperator(data[:, 1:], Unit())
    with pytest.raises(TypeError, match="Bed or a SnpGen"):
        SnpOperator(np.zeros((3, 2)), Unit())
    with pytest.raises(TypeError, match="DiagKtoN"):
        SnpOperator(_bed(), DiagKtoN())
    with pytest.raises(ValueError, match="float32 or float64"):
        SnpOperator(_bed(), Unit(), dtype=np.int8)


def test_shape_of_sources_and_subsets():
    from pysnptools_amd.linop import SnpOperator

    bed, gen = _bed(), SnpGen(seed=1, iid_count=50, sid_count=300)
    assert SnpOperator(bed, Unit()).shape == (300, 1015)
    assert SnpOperator(bed[::2, 5:100], Beta(1, 25), dtype="float64", resident=False).shape == (150, 95)
    assert SnpOperator(bed[[7, 3], [9, 0, 4]], Identity()).shape == (2, 3)
    assert SnpOperator(gen, Unit()).shape == (50, 300)
    assert SnpOperator(gen[3:, ::2], Unit()).shape == (47, 150)
    assert SnpOperator(bed, Unit()).dtype == np.float32


def test_operand_errors_come_before_any_device_work(monkeypatch):
    """A wrong dtype or row count is a ValueError, raised without one call into the library."""
    from pysnptools_amd.linop import SnpOperator

    op = SnpOperator(_bed()[::2, 5:100], Unit(), dtype="float64")
    called = []
    monkeypatch.setattr(N, "call", lambda name, *a: called.append(name))
    for product, rows in ((op.rmatmat, 150), (op.kernel_matmat, 150), (op.matmat, 95)):
        with pytest.raises(ValueError, match="rows"):
            product(np.ones(rows + 1))
        with pytest.raises(ValueError, match="rows"):
            product(np.ones((rows - 1, 2)))
        with pytest.raises(ValueError, match="float64"):
            product(np.ones(rows, dtype=np.float32))
        with pytest.raises(ValueError, match="float64"):
            product(np.ones((rows, 2), dtype=np.int64))
        with pytest.raises(ValueError, match="dimensions"):
            product(np.ones((rows, 2, 2)))
    assert called == []


def test_empty_products_and_result_shapes():
    """No SNPs, or no columns: the zero product, 1-D for a vector and 2-D for a matrix, without a device."""
    from pysnptools_amd.linop import SnpOperator

    op = SnpOperator(_bed()[:, []], Unit(), dtype="float32")
    assert op.shape == (300, 0)
    v, V = np.ones(300, dtype=np.float32), np.ones((300, 3), dtype=np.float32)
    assert op.rmatmat(v).shape == (0,) and op.rmatmat(V).shape == (0, 3)
    y = op.matmat(np.ones(0, dtype=np.float32))
    Y = op.matmat(np.ones((0, 3), dtype=np.float32))
    assert y.shape == (300,) and Y.shape == (300, 3) and y.dtype == Y.dtype == np.float32
    assert not y.any() and not Y.any() and not op.kernel_matmat(V).any()
    assert op.kernel_matmat(v).shape == (300,)
    full = SnpOperator(_bed(), Unit(), dtype="float64")
    assert full.rmatmat(np.ones((300, 0))).shape == (1015, 0)
    assert full.matmat(np.ones((1015, 0))).shape == (300, 0)


@pytest.mark.skipif(has_gpu_device(), reason="checks the no-device error path")
def test_no_cpu_fallback_without_device():
    from pysnptools_amd.linop import SnpOperator

    op = SnpOperator(_bed(), Unit())
    with pytest.raises(N.NativeError):
        op.rmatmat(np.ones(300, dtype=np.float32))
