"""Generate tests/golden/snpgen_cases.npz by running the REFERENCE's SnpGen itself.

Runs only where the reference is present (tools/make_golden.py's import harness).  The file holds
data only: per case its parameters ``<name>_params`` = [seed, iid_count, sid_count, block_size
(0 = default)], the selected SNP indices ``<name>_sid`` and the values ``<name>_val_i8`` (int8,
-127 = missing), plus the ``pos`` table of two readers.

Usage:  python tools/make_golden_snpgen.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUT, install_harness, to_i8  # noqa: E402

# name -> (seed, iid_count, sid_count, block_size or None, sid selection or None)
CASES = {
    "b8": (7, 37, 50, 8, None),            # n % 4 = 1, 7 batches, the last one runs past sid_count
    "tiny": (5, 3, 9, 4, None),            # fewer iids than one packed byte
    "upper": (1, 2, 16, 16, None),         # c_j <= iid_count rejects SNPs that c_j != 0 would keep
    "long": (11, 100003, 3, None, None),   # default block 1, long column
    "n32": (13, 32, 70, 24, None),         # n % 16 = 0 (F order decodes in place); 256 % block != 0
    "b100": (2, 1000, 300, None, list(range(0, 300, 7))),  # default block 100: no power of two, 3 batches
}


def main():
    install_harness()
    from pysnptools.snpreader.snpgen import SnpGen

    warnings.simplefilter("ignore")
    g = {}
    for name, (seed, n, m, block, sel) in CASES.items():
        gen = SnpGen(seed=seed, iid_count=n, sid_count=m, block_size=block)
        sid = np.arange(m) if sel is None else np.array(sel)
        val = gen[:, sid].read().val
        assert val.shape == (n, len(sid))
        g[name + "_params"] = np.array([seed, n, m, block or 0], dtype=np.int64)
        g[name + "_sid"] = sid.astype(np.int64)
        g[name + "_val_i8"] = to_i8(val)
    g["pos_0_100_100"] = SnpGen(seed=0, iid_count=100, sid_count=100).pos
    g["pos_3_10_1000_c5"] = SnpGen(seed=3, iid_count=10, sid_count=1000, chrom_count=5).pos
    path = os.path.join(OUT, "snpgen_cases.npz")
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    assert size <= 1 << 20, "snpgen_cases.npz is %d bytes: over the committed-file limit" % size
    print("written", path, size, "bytes")


if __name__ == "__main__":
    main()
