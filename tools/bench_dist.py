"""Rates of the distribution -> dosage kernels (csrc/dist.hip) and of the GRM of ``dist.as_snp()``.

Prints one JSON line:
* ``dist_to_snp``: ``snpmi_dist_to_snp_f32`` on device-resident data (rows x cols triples, default
  50k x 8192), F -> F and C -> F, median of ``--reps`` HIP-event timings after one warm-up, and the
  GB/s on the algorithmic 16 bytes per genotype (12 read + 4 written);
* ``memcpy_d2d``: ``snpmi_dev_memcpy_d2d`` moving the same byte count (rows * cols * 8 bytes copied =
  16 bytes of traffic per genotype) in the same process;
* ``grm``: wall time of ``DistData.as_snp().read_kernel(Unit(), dtype=float32)`` over host values
  (the session route: slabs uploaded, converted, standardized and accumulated in HBM) beside the
  route that existed before -- the conversion in NumPy on the host, then ``SnpData.read_kernel``;
* the box the numbers come from.

Usage: python tools/bench_dist.py [--rows 50000] [--cols 8192] [--reps 5] [--no-grm]
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


def box_id(N):
    name = ctypes.create_string_buffer(128)
    mem, cus = ctypes.c_uint64(0), ctypes.c_int(0)
    N.call("snpmi_device_info", 0, name, 128, ctypes.byref(mem), ctypes.byref(cus))
    uuid, pci, clk = (ctypes.c_uint8 * 16)(), (ctypes.c_int * 3)(), ctypes.c_int()
    N.call("snpmi_device_ids", 0, uuid, pci, ctypes.byref(clk))
    return {"gpu": name.value.decode(errors="replace"), "cus": cus.value, "uuid": bytes(uuid).hex(),
            "pci": "%04x:%02x:%02x" % tuple(pci), "sclk_max_mhz": clk.value / 1e3}


def event_ms(N, fn, reps):
    ev = []
    for _ in range(2):
        e = ctypes.c_void_p()
        N.call("snpmi_event_create", ctypes.byref(e))
        ev.append(e)
    fn()  # warm-up (scratch, code objects)
    N.call("snpmi_stream_sync")
    ms = []
    for _ in range(reps):
        N.call("snpmi_event_record", ev[0])
        fn()
        N.call("snpmi_event_record", ev[1])
        N.call("snpmi_event_sync", ev[1])
        t = ctypes.c_float(0)
        N.call("snpmi_event_elapsed_ms", ev[0], ev[1], ctypes.byref(t))
        ms.append(t.value)
    for e in ev:
        N.call("snpmi_event_destroy", e)
    return float(np.median(ms))


def host_triples(rows, cols, seed=7):
    """rows x cols x 3 float32 in F order: a seeded block of 64 SNPs (2% NaN triples) repeated."""
    rng = np.random.default_rng(seed)
    blk = min(cols, 64)
    p = rng.random((rows, blk, 3), dtype=np.float32)
    p /= p.sum(axis=-1, keepdims=True)
    p[rng.random((rows, blk)) < 0.02] = np.nan
    out = np.empty((rows, cols, 3), dtype=np.float32, order="F")
    for c0 in range(0, cols, blk):
        out[:, c0:c0 + blk] = p[:, :min(blk, cols - c0)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--cols", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-grm", action="store_true")
    args = ap.parse_args()
    from pysnptools_amd import _native as N
    from pysnptools_amd import hbm
    from pysnptools_amd.distreader import DistData
    from pysnptools_amd.snpreader import SnpData
    from pysnptools_amd.standardizer import Unit

    rows, cols = args.rows, args.cols
    res = {"bench": "dist", "box": box_id(N), "rows": rows, "cols": cols, "dtype": "float32"}
    val = host_triples(rows, cols)
    dev = hbm.asarray(val)  # the same bytes serve as the F-order and as the C-order array
    out = hbm.empty((rows, cols), dtype=np.float32, order="F")
    geno = rows * cols
    res["dist_to_snp"] = {}
    for tag, order_c in (("F_to_F", 0), ("C_to_F", 1)):
        ms = event_ms(N, lambda: N.call("snpmi_dist_to_snp_f32", dev.snpmi_ptr, rows, cols, 0, cols, order_c, 2.0,
                                        out.snpmi_ptr, 0), args.reps)
        res["dist_to_snp"][tag] = {"ms": round(ms, 4), "GB_per_s": round(16 * geno / ms / 1e6, 1)}
    scratch = hbm.empty((rows, cols, 2), dtype=np.float32, order="F")
    ms = event_ms(N, lambda: N.call("snpmi_dev_memcpy_d2d", scratch.snpmi_ptr, dev.snpmi_ptr, 8 * geno), args.reps)
    res["memcpy_d2d"] = {"ms": round(ms, 4), "GB_per_s": round(16 * geno / ms / 1e6, 1)}
    del scratch, out, dev

    if not args.no_grm:
        iid = np.array([["f%d" % i, "i%d" % i] for i in range(rows)])
        sid = np.array(["s%d" % j for j in range(cols)])
        dist = DistData(iid, sid, val)
        dist.as_snp()[:, :64].read_kernel(Unit(), dtype=np.float32)  # warm-up: scratch and tiles allocated
        t0 = time.perf_counter()
        K = dist.as_snp().read_kernel(Unit(), dtype=np.float32).val
        t_new = time.perf_counter() - t0
        t0 = time.perf_counter()
        weights = np.array([0, .5, 1], dtype=np.float32) * 2.0
        snp = np.empty((rows, cols), dtype=np.float32, order="F")
        for c0 in range(0, cols, 256):  # the reference's host pass, in blocks of bounded temporaries
            snp[:, c0:c0 + 256] = (val[:, c0:c0 + 256] * weights).sum(axis=-1)
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        K_old = SnpData(iid, sid, snp).read_kernel(Unit(), dtype=np.float32).val
        t_old = time.perf_counter() - t0
        scale = float(np.abs(np.diag(K_old)).max())
        res["grm"] = {"as_snp_read_kernel_s": round(t_new, 3), "host_convert_s": round(t_host, 3),
                      "snpdata_read_kernel_s": round(t_old, 3), "host_route_s": round(t_host + t_old, 3),
                      "max_abs_diff_over_max_diag": float(np.abs(K[:512] - K_old[:512]).max() / scale)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
