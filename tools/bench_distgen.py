"""Rate of the GPU DistGen generator (csrc/distgen.hip) beside k_snpgen's, and the GRM it feeds.

Prints one JSON line:

* ``generator``: for 500k iids x 64 SNPs (B = 1) and 1000 iids x 100,000 SNPs (B = 100), float64 and
  float32, C and F order: the wall time of one ``snpmi_dev_distgen_*`` call (best of ``--reps`` after
  one warm-up), the MT19937 words its workgroups consumed per second (a batch is 4 n B doubles =
  8 n B words) and (iid, SNP) triples per second; ``wg`` = workgroups in flight (one per batch, at
  most 8 per CU) and ``words_per_s_per_wg`` the rate of one;
* ``snpgen``: tools/bench_snpgen.py's words/s of ``k_snpgen`` in the same process, at the same two
  shapes and at its own long 500k shape;
* ``read_kernel``: ``DistGen(...).as_snp().read_kernel(Unit(), dtype=float32)`` at ``--iids`` x
  ``--snps`` (50k x 8192) beside the same cohort made on the host with NumPy (distgen.py:154-165
  restated with a ``RandomState`` per batch), wrapped in a ``DistData`` and run through the
  stored-distribution route, which uploads the 12 bytes per value and component it reads.

Usage: python tools/bench_distgen.py [--reps 3] [--iids 50000] [--snps 8192] [--skip-kernel]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run_generator(hbm, DistGen, name, iid_count, sid_count, block_size, dtype, order, reps, cus):
    gen = DistGen(seed=332, iid_count=iid_count, sid_count=sid_count, block_size=block_size)
    block = gen._block_size
    out = hbm.empty((iid_count, sid_count, 3), dtype=dtype, order=order)
    sid = np.arange(sid_count)
    best = None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        gen._generate_into(out, sid)  # synchronous
        t = time.perf_counter() - t0
        if r > 0:
            best = t if best is None else min(best, t)
    batches = (sid_count + block - 1) // block
    words = batches * 8 * iid_count * block
    wg = min(batches, 8 * cus)
    return {"shape": name, "iid_count": iid_count, "block_size": block, "snps": sid_count, "batches": batches,
            "dtype": np.dtype(dtype).name, "order": order, "seconds": round(best, 6), "wg": wg,
            "words_per_s": round(words / best, 1), "words_per_s_per_wg": round(words / best / wg, 1),
            "triples_per_s": round(iid_count * sid_count / best, 1),
            "out_gb_per_s": round(out.nbytes / best / 1e9, 2)}


def host_cohort(seed, n, m, block, dtype):
    """The reference's values on the host (distgen.py:154-165), F order as ``read()`` gives them."""
    val = np.empty((n, m, 3), dtype=dtype, order="F")
    for start in range(0, m, block):
        rs = np.random.RandomState(seed + start)
        v = rs.random_sample((n, block, 3))
        v /= v.sum(axis=2, keepdims=True)
        v[rs.random_sample((n, block)) < .218, :] = np.nan
        stop = min(start + block, m)
        val[:, start:stop, :] = v[:, :stop - start, :]
    return val


def run_kernel(DistGen, DistData, Unit, n, m):
    gen = DistGen(seed=332, iid_count=n, sid_count=m)
    res = {"iid_count": n, "snps": m, "block_size": gen._block_size, "dtype": "float32"}
    gen[:, :gen._block_size].as_snp().read_kernel(Unit(), dtype=np.float32)  # warm-up: scratch, K pages
    t0 = time.perf_counter()
    K = gen.as_snp().read_kernel(Unit(), dtype=np.float32).val
    res["distgen_read_kernel_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    val = host_cohort(332, n, m, gen._block_size, np.float32)
    res["host_generate_s"] = round(time.perf_counter() - t0, 3)
    data = DistData(gen.iid, gen.sid, val=val)
    t0 = time.perf_counter()
    Kh = data.as_snp().read_kernel(Unit(), dtype=np.float32).val
    res["distdata_read_kernel_s"] = round(time.perf_counter() - t0, 3)
    res["upload_gb"] = round(val.nbytes / 1e9, 2)
    # (the first 512 rows: a difference of the whole 10 GB matrices would double the host memory)
    res["max_abs_diff_over_max_diag_512_rows"] = float(np.abs(K[:512] - Kh[:512]).max() / np.abs(np.diag(Kh)).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iids", type=int, default=50000)
    ap.add_argument("--snps", type=int, default=8192)
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    import bench_snpgen

    from pysnptools_amd import _native as N
    from pysnptools_amd import hbm
    from pysnptools_amd.distreader import DistData, DistGen
    from pysnptools_amd.snpreader import SnpGen
    from pysnptools_amd.standardizer import Unit

    name = ctypes.create_string_buffer(128)
    mem, cus = ctypes.c_uint64(0), ctypes.c_int(0)
    N.call("snpmi_device_info", 0, name, 128, ctypes.byref(mem), ctypes.byref(cus))
    uuid, pci, clk = (ctypes.c_uint8 * 16)(), (ctypes.c_int * 3)(), ctypes.c_int()
    N.call("snpmi_device_ids", 0, uuid, pci, ctypes.byref(clk))
    box = {"gpu": name.value.decode(errors="replace"), "cus": cus.value, "uuid": bytes(uuid).hex(),
           "pci": "%04x:%02x:%02x" % tuple(pci), "sclk_max_mhz": clk.value / 1e3}
    generator = [run_generator(hbm, DistGen, shape, n, m, None, dtype, order, args.reps, cus.value)
                 for shape, n, m in (("500k_x_64_b1", 500000, 64), ("1000_x_100k_b100", 1000, 100000))
                 for dtype in (np.float64, np.float32) for order in ("C", "F")]
    snpgen = [bench_snpgen.run_shape(N, SnpGen, "500k_x_64_b1", 500000, None, 64, args.reps),
              bench_snpgen.run_shape(N, SnpGen, "1000_x_100k_b100", 1000, 100, 100000, args.reps),
              bench_snpgen.run_shape(N, SnpGen, "500k_default_block_long", 500000, None, 32768, 1)]
    out = {"bench": "distgen", "box": box, "generator": generator, "snpgen": snpgen}
    if not args.skip_kernel:
        out["read_kernel"] = run_kernel(DistGen, DistData, Unit, args.iids, args.snps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
