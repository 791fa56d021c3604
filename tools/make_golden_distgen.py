"""Generate tests/golden/distgen.npz by running the REFERENCE's own ``DistGen``.

Runs only where the reference checkout is (``make_golden.REF``); the committed output is data.  Same
import harness as tools/make_golden_dist.py; no formula is restated.  Recorded in float64, each
with its ``iid``, ``sid`` and ``pos`` (keys ``<tag>_val`` / ``_iid`` / ``_sid`` / ``_pos``; ``CASES``
below is also what tests/test_gpu_distgen.py constructs):

* ``n1_b1``    1 iid, one-SNP batches: 4 doubles per stream, one partial tile;
* ``n5_b3``    5 iids, 7 SNPs in batches of 3: no regeneration of the state; the last batch is partial;
* ``n257_b2``  257 iids, batches of 2: several tiles and regenerations, a last partial tile;
* ``n300_b1``  300 iids, one-SNP batches: the layout of large cohorts;
* ``n4_b1``    SNPs 0, 2999 and 5999 of 4 iids x 6000 one-SNP batches.

Usage:  python tools/make_golden_distgen.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_dist as MGD  # noqa: E402

# tag -> (seed, iid_count, sid_count, block_size, SNP selection or None)
CASES = {"n1_b1": (3, 1, 2, 1, None),
         "n5_b3": (7, 5, 7, 3, None),
         "n257_b2": (1, 257, 4, 2, None),
         "n300_b1": (5, 300, 3, 1, None),
         "n4_b1": (11, 4, 6000, 1, [0, 2999, 5999])}


def main():
    MGD.install_harness()
    warnings.simplefilter("ignore")
    from pysnptools.distreader import DistGen

    g = {}
    for tag, (seed, n, m, block, sel) in CASES.items():
        gen = DistGen(seed=seed, iid_count=n, sid_count=m, block_size=block)
        data = (gen if sel is None else gen[:, sel]).read(order="C", dtype=np.float64)
        g[tag + "_val"] = np.ascontiguousarray(data.val)
        g[tag + "_iid"] = np.array(data.iid, dtype="U")
        g[tag + "_sid"] = np.array(data.sid, dtype="U")
        g[tag + "_pos"] = np.array(data.pos, dtype=np.float64)
        first = data.val[:, :block, 0]
        print(tag, data.val.shape, "NaN (iid, SNP) pairs of the first batch: %d of %d" % (np.isnan(first).sum(), first.size))
    np.savez_compressed(os.path.join(MGD.OUT, "distgen.npz"), **g)
    print("distgen goldens written:", os.path.getsize(os.path.join(MGD.OUT, "distgen.npz")), "bytes")


if __name__ == "__main__":
    main()
