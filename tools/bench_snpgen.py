"""Rate of the GPU SnpGen generator (csrc/snpgen.hip) beside numpy's RandomState on one host thread.

Prints one JSON line: for each shape the wall time of one ``snpmi_dev_snpgen_bed`` call (best of
``--reps``, after one warm-up), the MT19937 words its generator workgroups consumed
(``snpmi_dev_snpgen_rounds`` x 2 * block * (1 + 3 * iid_count)) per second and SNPs per second;
``host_doubles_per_s`` is ``RandomState.random_sample`` on one thread of the same box (a double is
two words).  Usage: python tools/bench_snpgen.py [--reps 3] [--snps 4096]
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


def run_shape(N, SnpGen, name, iid_count, block_size, sid_count, reps):
    gen = SnpGen(seed=332, iid_count=iid_count, sid_count=sid_count, block_size=block_size)
    block = gen._block_size
    sid = np.arange(sid_count)
    best, rounds = None, ctypes.c_uint64(0)
    for r in range(reps + 1):
        t0 = time.perf_counter()
        packed, _ = gen._packed(sid)  # synchronous
        t = time.perf_counter() - t0
        del packed
        if r > 0:
            best = t if best is None else min(best, t)
    N.call("snpmi_dev_snpgen_rounds", ctypes.byref(rounds))
    batches = (sid_count + block - 1) // block
    words = rounds.value * 2 * block * (1 + 3 * iid_count)
    return {"shape": name, "iid_count": iid_count, "block_size": block, "snps": sid_count, "batches": batches,
            "rounds_per_batch": round(rounds.value / batches, 3), "seconds": round(best, 6),
            "words_per_s": round(words / best, 1), "snps_per_s": round(sid_count / best, 2)}


def host_rate(count=20_000_000):
    rs = np.random.RandomState(332)
    rs.random_sample(1000)
    t0 = time.perf_counter()
    rs.random_sample(count)
    return count / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--snps", type=int, default=4096, help="SNPs of the 500k-iid shape")
    ap.add_argument("--long-snps", type=int, default=32768, help="SNPs of the long 500k-iid shape (4 GB of codes)")
    args = ap.parse_args()
    from pysnptools_amd import _native as N
    from pysnptools_amd.snpreader import SnpGen

    name = ctypes.create_string_buffer(128)
    mem, cus = ctypes.c_uint64(0), ctypes.c_int(0)
    N.call("snpmi_device_info", 0, name, 128, ctypes.byref(mem), ctypes.byref(cus))
    uuid, pci, clk = (ctypes.c_uint8 * 16)(), (ctypes.c_int * 3)(), ctypes.c_int()
    N.call("snpmi_device_ids", 0, uuid, pci, ctypes.byref(clk))
    box = {"gpu": name.value.decode(errors="replace"), "cus": cus.value, "uuid": bytes(uuid).hex(),
           "pci": "%04x:%02x:%02x" % tuple(pci), "sclk_max_mhz": clk.value / 1e3}
    shapes = [run_shape(N, SnpGen, "500k_default_block", 500000, None, args.snps, args.reps),
              # enough batches per workgroup slot that the slowest batch's rounds stop dominating
              run_shape(N, SnpGen, "500k_default_block_long", 500000, None, args.long_snps, 1),
              run_shape(N, SnpGen, "1000x1000_block", 1000, 1000, 256 * 1000, args.reps),
              run_shape(N, SnpGen, "1000x1000_block_long", 1000, 1000, 2048 * 1000, 1),
              run_shape(N, SnpGen, "500k_single_batch", 500000, None, 1, args.reps),
              run_shape(N, SnpGen, "1000x1000_single_batch", 1000, 1000, 1000, args.reps)]
    host = host_rate()
    print(json.dumps({"bench": "snpgen", "box": box, "shapes": shapes,
                      "host_doubles_per_s": round(host, 1), "host_words_per_s": round(2 * host, 1)}), flush=True)


if __name__ == "__main__":
    main()
