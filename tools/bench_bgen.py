"""Rates of the Bgen reader's stages (csrc/bgen.hip, distreader/bgen.py) and of the GRM it feeds.

The files are written here with ``Bgen.write`` from a ``DistGen`` (16 bits, zlib), then one JSON
line is printed:

* ``scan``: ``snpmi_bgen_open`` + ``snpmi_bgen_index`` over a file of ``--scan-variants`` short
  variants (2 samples each): variants per second of the native walk, and of the whole ``_run_once``
  (which adds the str arrays, sid and pos);
* ``inflate``: pread + ``zlib.decompress`` + the host checks of ``--decode-snps`` blocks of the
  ``--iids`` file on the reader's thread pool: GB/s of inflated bytes at that thread count;
* ``decode``: one ``snpmi_dev_bgen_decode_*`` call over those staged blocks (best of ``--reps``
  after a warm-up; the call is synchronous and includes its table upload) per dtype and order: GB/s
  of output written and of traffic (output + staged blocks), beside ``snpmi_dev_memcpy_d2d`` of the
  output's bytes (traffic: twice that) and the decode's traffic rate as a fraction of the copy's;
* ``read_kernel``: ``Bgen(...).as_snp().read_kernel(Unit(), dtype=float32)`` at ``--iids`` x
  ``--snps`` (50k x 8192) beside the same triples held by a host ``DistData``.

Usage: python tools/bench_bgen.py [--reps 3] [--iids 50000] [--snps 8192] [--decode-snps 2048]
                                  [--scan-variants 100000] [--skip-kernel] [--dir DIR]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def best_of(reps, fn):
    best = None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        t = time.perf_counter() - t0
        if r > 0 or reps == 0:
            best = t if best is None else min(best, t)
    return best


def run_scan(N, Bgen, DistData, folder, variants):
    val = np.zeros((2, variants, 3))
    val[:, :, 0] = 1
    data = DistData(iid=[["0", "a"], ["0", "b"]], sid=["rs%d" % j for j in range(variants)], val=val,
                    pos=np.column_stack([np.ones(variants), np.zeros(variants), np.arange(variants)]))
    path = Bgen.write(os.path.join(folder, "scan.bgen"), data, bits=8, block_size=variants).filename
    info = (ctypes.c_uint64 * 11)()

    def native():
        N.call("snpmi_bgen_open", path.encode(), info)
        m, n = int(info[0]), int(info[1])
        rec = np.zeros((m, 5), dtype=np.uint64)
        raw = [np.zeros(c, dtype="S%d" % max(int(w), 1)) for c, w in zip((n, m, m, m, m), info[5:10])]
        args = []
        for a, w in zip(raw, info[5:10]):
            args += [N.ptr(a), int(w)]
        N.call("snpmi_bgen_index", path.encode(), m, n, N.ptr(rec), *args)

    t_native = best_of(2, native)
    t_all = best_of(1, lambda: Bgen(path)._run_once())
    return {"variants": variants, "file_mb": round(os.path.getsize(path) / 1e6, 1),
            "native_seconds": round(t_native, 4), "native_variants_per_s": round(variants / t_native, 1),
            "run_once_seconds": round(t_all, 4), "run_once_variants_per_s": round(variants / t_all, 1)}


def run_inflate(bgen, count, threads):
    def go():
        with ThreadPoolExecutor(max_workers=threads) as pool:
            return sum(len(d) for d, _ in pool.map(bgen._inflate, range(count)))

    t = best_of(1, go)
    nbytes = int(bgen._rec[:count, 2].sum())
    return {"blocks": count, "threads": threads, "inflated_gb": round(nbytes / 1e9, 3),
            "stored_gb": round(int(bgen._rec[:count, 1].sum()) / 1e9, 3), "seconds": round(t, 4),
            "inflated_gb_per_s": round(nbytes / t / 1e9, 3)}


def run_decode(N, hbm, bgen, count, reps):
    n = bgen.iid_count
    cols = np.arange(count)
    res = []
    for dtype, order in ((np.float32, "F"), (np.float64, "F"), (np.float32, "C"), (np.float64, "C")):
        out = hbm.empty((n, count, 3), dtype=dtype, order=order)
        bgen._decode_into(out, count, 0, cols)  # stages the blocks (and warms up)
        st = bgen._staging
        uniq_off = np.concatenate(([0], np.cumsum((bgen._rec[:count, 2] + 7) // 8 * 8)))[:-1]
        table = np.empty((count, 3), dtype=np.uint64)
        table[:, 0], table[:, 1], table[:, 2] = uniq_off, 16, n
        total = int(uniq_off[-1] + (bgen._rec[count - 1, 2] + 7) // 8 * 8 + 16)
        t = best_of(reps, lambda: N.call("snpmi_dev_bgen_decode_" + N.suffix(dtype), N.ptr(st.dev), total,
                                         N.ptr(table), count, None, n, N.ptr(out), count, 0, 1 if order == "C" else 0))
        src = hbm.empty((n, count, 3), dtype=dtype, order=order)

        def copy():
            N.call("snpmi_dev_memcpy_d2d", N.ptr(out), N.ptr(src), out.nbytes)
            N.call("snpmi_stream_sync")

        tc = best_of(reps, copy)
        res.append({"iid_count": n, "snps": count, "bits": 16, "dtype": np.dtype(dtype).name, "order": order,
                    "seconds": round(t, 6), "out_gb": round(out.nbytes / 1e9, 3),
                    "read_gb": round(total / 1e9, 3), "out_gb_per_s": round(out.nbytes / t / 1e9, 1),
                    "copy_seconds": round(tc, 6), "copy_gb_per_s": round(out.nbytes / tc / 1e9, 1),
                    # both as HBM traffic: the decode reads `total` and writes `out`, the copy moves `out` twice
                    "traffic_gb_per_s": round((out.nbytes + total) / t / 1e9, 1),
                    "copy_traffic_gb_per_s": round(2 * out.nbytes / tc / 1e9, 1),
                    "fraction_of_copy_rate": round((out.nbytes + total) / t / (2 * out.nbytes / tc), 3)})
        del out, src
    return res


def run_kernel(bgen, DistData, Unit, m):
    n = bgen.iid_count
    res = {"iid_count": n, "snps": m, "bits": 16, "dtype": "float32"}
    reader = bgen[:, :m]
    bgen[:, :4].as_snp().read_kernel(Unit(), dtype=np.float32)  # warm-up: scratch, K pages
    t0 = time.perf_counter()
    K = reader.as_snp().read_kernel(Unit(), dtype=np.float32).val
    res["bgen_read_kernel_s"] = round(time.perf_counter() - t0, 3)
    note("bgen read_kernel", res["bgen_read_kernel_s"])
    t0 = time.perf_counter()
    data = reader.read(dtype=np.float32)
    res["bgen_read_to_host_s"] = round(time.perf_counter() - t0, 3)
    stored = DistData(data.iid, data.sid, val=data.val)
    t0 = time.perf_counter()
    Kh = stored.as_snp().read_kernel(Unit(), dtype=np.float32).val
    res["distdata_read_kernel_s"] = round(time.perf_counter() - t0, 3)
    res["upload_gb"] = round(data.val.nbytes / 1e9, 2)
    res["max_abs_diff_over_max_diag_512_rows"] = float(np.abs(K[:512] - Kh[:512]).max() / np.abs(np.diag(Kh)).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iids", type=int, default=50000)
    ap.add_argument("--snps", type=int, default=8192)
    ap.add_argument("--decode-snps", type=int, default=2048)
    ap.add_argument("--scan-variants", type=int, default=100000)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()

    from pysnptools_amd import _native as N
    from pysnptools_amd import hbm
    from pysnptools_amd.distreader import Bgen, DistData, DistGen
    from pysnptools_amd.standardizer import Unit
    from pysnptools_amd.util import get_num_threads

    name = ctypes.create_string_buffer(128)
    mem, cus = ctypes.c_uint64(0), ctypes.c_int(0)
    N.call("snpmi_device_info", 0, name, 128, ctypes.byref(mem), ctypes.byref(cus))
    out = {"bench": "bgen", "box": {"gpu": name.value.decode(errors="replace"), "cus": cus.value}}
    with tempfile.TemporaryDirectory(dir=args.dir) as folder:
        out["scan"] = run_scan(N, Bgen, DistData, folder, args.scan_variants)
        note("scan", out["scan"])
        m = args.decode_snps if args.skip_kernel else max(args.snps, args.decode_snps)
        t0 = time.perf_counter()
        bgen = Bgen.write(os.path.join(folder, "cohort.bgen"), DistGen(seed=332, iid_count=args.iids, sid_count=m),
                          bits=16, compression="zlib", block_size=64)
        out["write"] = {"iid_count": args.iids, "snps": m, "seconds": round(time.perf_counter() - t0, 1),
                        "file_gb": round(os.path.getsize(bgen.filename) / 1e9, 3)}
        note("write", out["write"])
        bgen._run_once()
        threads = get_num_threads(None)
        out["inflate"] = run_inflate(bgen, args.decode_snps, threads)
        note("inflate", out["inflate"])
        out["decode"] = run_decode(N, hbm, bgen, args.decode_snps, args.reps)
        note("decode", out["decode"])
        if not args.skip_kernel:
            out["read_kernel"] = run_kernel(bgen, DistData, Unit, args.snps)
        bgen.flush()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
