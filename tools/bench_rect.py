"""Rate of the two-operand ("rect") GRM kernels beside the SYRK's, in one process.

Default: rows in {1024, 4096} x cols = 50,000 iids x 62,500 synthetic SNPs (bench.synth), f32 and
f64 -- ms per snpmi_dev_syrk_rect launch, TF/s (2 rows cols snps / t; f64 also the int8 op/s of
the residue products) and, beside it, the same figures of snpmi_dev_syrk_packed at the same iids
and SNPs.  Prints one JSON line.

--session: K[:rows, :] through the session entries (snpmi_grm_rect_begin / add_packed / end) into
host memory, e.g. --iids 500000 --rows 1024 --snps 8192 --session, a size at which the whole K's
tiles do not fit one device.
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
import bench  # noqa: E402
from pysnptools_amd import _native as N  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up (scratch allocation, LUT caches)
    N.call("snpmi_stream_sync")
    ev = bench.Events(N, 2)
    ms = []
    for _ in range(reps):
        N.call("snpmi_event_record", ev.ev[0])
        fn()
        N.call("snpmi_event_record", ev.ev[1])
        N.call("snpmi_event_sync", ev.ev[1])
        t = ctypes.c_float(0)
        N.call("snpmi_event_elapsed_ms", ev.ev[0], ev.ev[1], ctypes.byref(t))
        ms.append(t.value)
    return float(np.median(ms))


def moduli_sum(fn):
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    N.call("snpmi_crt_block_moduli_stats", ctypes.byref(a), ctypes.byref(b), 1)
    fn()
    N.call("snpmi_stream_sync")
    N.call("snpmi_crt_block_moduli_stats", ctypes.byref(a), ctypes.byref(b), 1)
    return a.value, b.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iids", type=int, default=50_000)
    ap.add_argument("--snps", type=int, default=62_500)
    ap.add_argument("--rows", default="1024,4096")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--session", action="store_true")
    ap.add_argument("--no-syrk", action="store_true", help="skip the snpmi_dev_syrk_packed reference rate")
    ap.add_argument("--syrk-only", action="store_true",
                    help="only the snpmi_dev_syrk_packed rates (also runs on a library without the rect entries, SNPMI_LIB)")
    a = ap.parse_args()
    n, m = a.iids, a.snps
    rows_list = [int(x) for x in a.rows.split(",")]
    pitch = int(N.lib().snpmi_packed_pitch(n))
    packed = bench.Dev(N, pitch * m)
    bench.synth(N, packed.p, pitch, n, 0, m, 41, 0.05)
    name = ctypes.create_string_buffer(256)
    tot, cus = ctypes.c_uint64(), ctypes.c_int()
    N.call("snpmi_device_info", 0, name, 256, ctypes.byref(tot), ctypes.byref(cus))
    free, total = ctypes.c_uint64(), ctypes.c_uint64()
    N.call("snpmi_device_memory", ctypes.byref(free), ctypes.byref(total))
    out = {"tool": "bench_rect", "device": name.value.decode(), "cus": cus.value, "iids": n, "snps": m, "results": []}
    for dname in a.dtypes.split(","):
        dtype = np.dtype({"f32": np.float32, "f64": np.float64}[dname])
        dt = N.dt_code(dtype)
        if a.session:
            for rows in rows_list:
                ri = np.arange(rows, dtype=np.uint64)
                K = np.empty((rows, n), dtype=dtype)
                st = np.empty((m, 2), dtype=dtype)
                t0 = time.perf_counter()
                N.call("snpmi_grm_rect_begin", rows, n, dt)
                N.call("snpmi_grm_rect_add_packed_" + dname, packed.p, pitch, n, m, 0, N.STD_UNIT, 0.0, 0.0, 0, N.ptr(st),
                       N.ptr(ri), None)
                N.call("snpmi_grm_rect_end", 1.0, 1, N.ptr(K))
                wall = time.perf_counter() - t0
                # spot check on the host: a few rows x the first / last few cols from the codes and the
                # per-SNP table (f64), relative to the largest of those rows' diagonals
                lut = bench.Dev(N, m * 4 * dtype.itemsize)
                sdev = bench.Dev(N, m * 2 * dtype.itemsize)
                N.call("snpmi_dev_snp_stats", packed.p, pitch, n, m, 0, N.STD_UNIT, 0.0, 0.0, 0, dt, sdev.p, lut.p)
                hl = np.empty((m, 4), dtype=dtype)
                N.call("snpmi_memcpy_d2h", N.ptr(hl), lut.p, hl.nbytes)
                hp = np.empty((m, pitch), dtype=np.uint8)
                N.call("snpmi_memcpy_d2h", N.ptr(hp), packed.p, hp.nbytes)
                lut.free()
                sdev.free()
                rr = np.array([0, 1, 255, 256, rows - 1])
                cc = np.array([0, 1, 255, 256, 257, n // 2, n - 257, n - 2, n - 1])

                def zs(ix):
                    codes = (hp[:, ix // 4] >> (2 * (ix % 4)).astype(np.uint8)) & 3
                    return np.take_along_axis(hl.astype(np.float64), codes.astype(np.intp), axis=1).T

                Zr, Zc = zs(rr), zs(cc)
                spot = np.abs(K[np.ix_(rr, cc)] - Zr @ Zc.T).max() / np.einsum("ij,ij->i", Zr, Zr).max()
                out["results"].append({
                    "spot_check_err_over_max_diag": float(spot),
                    "mode": "session", "dtype": dname, "rows": rows, "cols": n, "wall_s": round(wall, 3),
                    "whole_k_tile_bytes": int(N.lib().snpmi_grm_tile_bytes(n, dt)), "free_bytes_at_start": free.value,
                    "rect_block_bytes": int(N.lib().snpmi_grm_rect_bytes(rows, n, dt)),
                    "finite": bool(np.isfinite(K).all()), "k00": float(K[0, 0]), "k_last": float(K[-1, -1])})
            continue
        lut, stats = bench.Dev(N, m * 4 * dtype.itemsize), bench.Dev(N, m * 2 * dtype.itemsize)
        N.call("snpmi_dev_snp_stats", packed.p, pitch, n, m, 0, N.STD_UNIT, 0.0, 0.0, 0, dt, stats.p, lut.p)
        if not a.no_syrk:
            tiles = bench.Dev(N, int(N.lib().snpmi_grm_tile_bytes(n, dt)))

            def syrk():
                N.call("snpmi_dev_syrk_packed", packed.p, pitch, n, m, lut.p, dt, tiles.p, 0)

            ms = timed(syrk, a.reps)
            nb = (n + 255) // 256
            r = {"mode": "syrk", "dtype": dname, "iids": n, "ms": round(ms, 2),
                 "tflops": round(2.0 * (nb * (nb + 1) // 2) * 65536 * m / ms / 1e9, 1)}
            if dname == "f64":
                sr, blocks = moduli_sum(syrk)
                r["int8_tops"] = round(2.0 * sr * 65536 * m / ms / 1e9, 1)
                r["moduli_per_block"] = round(sr / max(blocks, 1), 2)
            out["results"].append(r)
            tiles.free()
        for rows in ([] if a.syrk_only else rows_list):
            ri = np.arange(rows, dtype=np.uint64)
            po = int(N.lib().snpmi_packed_pitch(rows))
            didx, A = bench.Dev(N, rows * 8), bench.Dev(N, po * m)
            N.call("snpmi_memcpy_h2d", didx.p, N.ptr(ri), ri.nbytes)
            N.call("snpmi_dev_repack", packed.p, pitch, n, didx.p, rows, m, A.p, po)
            blocks = bench.Dev(N, int(N.lib().snpmi_grm_rect_bytes(rows, n, dt)))

            def rect():
                N.call("snpmi_dev_syrk_rect", A.p, po, rows, packed.p, pitch, n, m, lut.p, dt, blocks.p, 0, None, 0)

            ms = timed(rect, a.reps)
            g = ((rows + 255) // 256) * ((n + 255) // 256)
            r = {"mode": "rect", "dtype": dname, "rows": rows, "cols": n, "blocks": g, "ms": round(ms, 2),
                 "tflops": round(2.0 * g * 65536 * m / ms / 1e9, 1)}
            if dname == "f64":
                sr, nblk = moduli_sum(rect)
                r["int8_tops"] = round(2.0 * sr * 65536 * m / ms / 1e9, 1)
                r["moduli_per_block"] = round(sr / max(nblk, 1), 2)
            out["results"].append(r)
            for d in (didx, A, blocks):
                d.free()
        lut.free()
        stats.free()
    packed.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
