"""Generate tests/golden/dist.npz by running the REFERENCE's distreader package itself.

Runs only where the reference checkout is (``make_golden.REF``); the committed outputs are data.
Same import harness as tools/make_golden.py, plus stubs for the BGEN readers the reference's
``distreader`` package imports and that are not installed (``bgen_reader``, ``cbgen``: nothing here
touches BGEN) and the NumPy names ``distnpz.py`` takes from an old scipy.  With these the
reference's own ``distreader`` package imports and runs; no formula is restated.  Also copies the three reference data files the dist tests read
(tiny.dist.memmap, toydata10.dist.npz, distgen.dist.npz) into tests/golden/data/.

Recorded, all through the reference's Python path:
* ``as_snp(max_weight=2 | 1)`` of both npz fixtures, all at once and with block_size=3;
* ``SnpData.as_dist(max_weight=2 | 1)`` of a small matrix holding 0, 1, 2, NaN, 0.5 and 1.5;
* ``as_snp().read_kernel(Unit() | Beta(1, 25))`` in float64 of toydata10.dist.npz.

Usage:  python tools/make_golden_dist.py
"""
import os
import shutil
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

REF, OUT, DATA = MG.REF, MG.OUT, MG.DATA
FIXTURES = {"tiny.dist.memmap": "pysnptools/examples/tiny.dist.memmap",
            "toydata10.dist.npz": "pysnptools/examples/toydata10.dist.npz",
            "distgen.dist.npz": "tests/datasets/distgen.dist.npz"}


def install_harness():
    MG.install_harness()
    import scipy

    for attr in ("str_", "array", "savez"):  # distnpz.py:4 is `import scipy as np` (pre-1.x aliases)
        if not hasattr(scipy, attr):
            setattr(scipy, attr, getattr(np, attr))
    for name in ("bgen_reader", "bgen_reader._multimemmap", "cbgen"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                stub = types.ModuleType(name)
                stub.__getattr__ = lambda attr: None  # any name imports; none is ever called
                sys.modules[name] = stub


def main():
    install_harness()
    warnings.simplefilter("ignore")
    from pysnptools.distreader import DistNpz
    from pysnptools.snpreader import SnpData
    from pysnptools.standardizer import Beta, Unit

    os.makedirs(DATA, exist_ok=True)
    for name, rel in FIXTURES.items():
        dst = os.path.join(DATA, name)
        shutil.copyfile(os.path.join(REF, rel), dst)
        os.chmod(dst, 0o644)

    g = {}
    for tag in ("toydata10", "distgen"):
        dist = DistNpz(os.path.join(DATA, tag + ".dist.npz"))
        for mw in (2, 1):
            whole = dist.as_snp(max_weight=mw).read(force_python_only=True).val
            block = dist.as_snp(max_weight=mw, block_size=3).read(force_python_only=True).val
            g["%s_snp_w%d" % (tag, mw)] = whole
            g["%s_snp_w%d_b3" % (tag, mw)] = block
    vals = np.array([[0, 1, 2, np.nan], [0.5, 1.5, 2, 0], [1, np.nan, 0.5, 1.5]], dtype=np.float64)
    sd = SnpData(iid=[["f%d" % i, "i%d" % i] for i in range(vals.shape[0])],
                 sid=["s%d" % j for j in range(vals.shape[1])], val=vals)
    g["as_dist_in"] = vals
    for mw in (2, 1):
        g["as_dist_w%d" % mw] = sd.as_dist(max_weight=mw).read(force_python_only=True).val
    toy = DistNpz(os.path.join(DATA, "toydata10.dist.npz"))
    g["toydata10_K_unit"] = toy.as_snp().read_kernel(Unit(), force_python_only=True).val
    g["toydata10_K_beta"] = toy.as_snp().read_kernel(Beta(1, 25), force_python_only=True).val
    np.savez_compressed(os.path.join(OUT, "dist.npz"), **g)
    print("dist goldens written:", {k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
