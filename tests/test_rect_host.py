"""Host-side checks of the direct K[rows, cols] path (pysnptools_amd.kernelreader.rect) that need no
GPU: the routing decision, the mode switch, which readers / standardizers qualify, and the list of
matched diagonal positions."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, ROOT
from pysnptools_amd.kernelreader import rect as R


def test_set_grm_rect_validation_and_env_default():
    old = R.grm_rect_mode()
    try:
        with pytest.raises(ValueError):
            R.set_grm_rect("sometimes")
        for mode in ("never", "always", "auto"):
            R.set_grm_rect(mode)
            assert R.grm_rect_mode() == mode
    finally:
        R.set_grm_rect(old)
    from pysnptools_amd.kernelreader import set_grm_rect

    assert set_grm_rect is R.set_grm_rect
    code = "from pysnptools_amd.kernelreader import rect; print(rect.grm_rect_mode())"
    for env, want in ((None, "auto"), ("always", "always"), ("bogus", "auto")):
        e = {k: v for k, v in os.environ.items() if k != "PST_GRM_RECT"}
        if env is not None:
            e["PST_GRM_RECT"] = env
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


def test_auto_decision_on_both_sides_of_the_80_percent_line():
    n, nr, nc = 500_000, 1024, 500_000
    item = 8
    t = (n + 127) // 128
    whole = t * (t + 1) // 2 * 128 * 128 * item + n * n * item // 8
    rect = ((nr + 255) // 256) * ((nc + 255) // 256) * 65536 * item
    assert rect == 4 * 1954 * 65536 * 8
    free = 256 << 30
    # the whole K does not fit, the rectangle does
    assert whole > 0.8 * free and rect < 0.8 * free
    assert R.use_rect(n, nr, nc, np.float64, 1, free, "auto")
    # the whole K just fits: the present route
    assert not R.use_rect(n, nr, nc, np.float64, 1, int(whole / 0.8) + 1, "auto")
    assert R.use_rect(n, nr, nc, np.float64, 1, int(whole / 0.8) - 1, "auto")
    # neither fits
    assert not R.use_rect(n, nr, nc, np.float64, 1, int(rect / 0.8) - 1, "auto")
    assert R.use_rect(n, nr, nc, np.float64, 1, int(rect / 0.8) + 1, "auto")
    # small problems keep the whole-K route under auto
    assert not R.use_rect(500, 70, 320, np.float32, 1, free, "auto")
    # a process group of more than one rank never takes it
    for mode in ("auto", "always"):
        assert not R.use_rect(n, nr, nc, np.float64, 2, free, mode)
    assert R.use_rect(500, 70, 320, np.float32, 1, free, "always")
    assert not R.use_rect(n, nr, nc, np.float64, 1, free, "never")


def test_which_sources_qualify():
    from pysnptools_amd.snpreader import Bed, SnpData, SnpGen
    from pysnptools_amd.standardizer import Beta, Identity, Unit, UnitTrained

    b = Bed(os.path.join(DATA, "toydata.bed"), count_A1=False)
    for std in (Unit(), Beta(1, 25), Identity(), UnitTrained(b.sid, np.ones((b.sid_count, 2)))):
        for dt in (np.float32, np.float64):
            assert R.rect_source(b, std, dt) is not None
    assert R.rect_source(b, Unit(), np.int8) is None
    base, rows, cols, _ = R.rect_source(b[::2, 10:20], Unit(), np.float64)
    assert base is b and list(rows[:3]) == [0, 2, 4] and list(cols) == list(range(10, 20))
    gen = SnpGen(seed=1, iid_count=40, sid_count=100)
    assert R.rect_source(gen, Unit(), np.float32) is not None
    assert R.rect_source(gen[:, 5:50], Unit(), np.float32) is not None
    assert R.rect_source(gen[::2, :], Unit(), np.float32) is None  # an iid subset of a SnpGen
    sd = SnpData(iid=[["f", "i%d" % i] for i in range(4)], sid=["s0", "s1"], val=np.zeros((4, 2)))
    assert R.rect_source(sd, Unit(), np.float64) is None

    class Other(Unit):
        pass

    from pysnptools_amd.standardizer.standardizer import _std_args

    if _std_args(Other()) is None:
        assert R.rect_source(b, Other(), np.float64) is None


def test_diag_pairs_with_repeats():
    rows = np.array([5, 9, 5, 2, 7])
    cols = np.array([7, 5, 1, 5, 2, 2])
    got = R.diag_pairs(rows, cols)
    want = sorted((r, c) for r in range(len(rows)) for c in range(len(cols)) if rows[r] == cols[c])
    assert got.dtype == np.uint32 and sorted(map(tuple, got.tolist())) == want and len(want) == 7
    assert R.diag_pairs(np.array([3, 4]), np.array([0, 1])).shape == (0, 2)
    assert R.diag_pairs(np.array([], dtype=np.int64), cols).shape == (0, 2)
    # None = all iids in order
    got = R.diag_pairs(None, np.array([2, 0, 2]), n_rows=3)
    assert sorted(map(tuple, got.tolist())) == [(0, 1), (2, 0), (2, 2)]
    got = R.diag_pairs(np.array([1, 3]), None, n_cols=3)
    assert sorted(map(tuple, got.tolist())) == [(0, 1)]
    got = R.diag_pairs(None, None, n_rows=4, n_cols=3)
    assert sorted(map(tuple, got.tolist())) == [(0, 0), (1, 1), (2, 2)]
