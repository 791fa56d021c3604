"""Rates of the packed-SNP products (csrc/matvec.hip): Z^T V, Z W and K V = Z (Z^T V) at the cfg4
launch shape, 50,000 iids x 62,500 SNPs of synthetic codes (bench.synth) resident in HBM.

Per dtype (f32, f64) and k in {1, 8, 32}, the legs ``tdot`` (snpmi_dev_packed_tdot), ``dot``
(snpmi_dev_packed_dot) and ``kernel_matmat`` (the two in a row): best of ``--reps`` after a warm-up,
HIP events on the compute stream.  Each leg is reported as

* milliseconds;
* packed GB/s (the codes read once per column panel are counted once), beside this process's
  ``snpmi_dev_memcpy_d2d`` rate over the same bytes as traffic (read + write);
* FMA/s (N M k per product);
* the fraction of the lower bound max(packed bytes / copy traffic rate, N M (k + 3) / VALU rate), the
  VALU rate taken as CUs x 64 lanes x ``--ghz`` one-lane operations per second; ``limit`` names the
  larger term.

Beside them: ``snpmi_dev_decode_standardize`` of the same block (f32), which is what materializing Z
alone costs.  One JSON line on stdout, also written to ``--out``.

Usage: python tools/bench_matvec.py [--iids 50000] [--snps 62500] [--reps 3] [--ghz 2.4]
                                    [--out profiles/matvec/bench_matvec.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def best_ms(N, ev, reps, fn):
    """Best of ``reps`` timed runs after one warm-up, in ms of the compute stream."""
    best = None
    for r in range(reps + 1):
        ev.record(0)
        fn()
        ev.record(1)
        N.call("snpmi_stream_sync")
        if r > 0:
            t = ev.ms(0, 1)
            best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iids", type=int, default=50000)
    ap.add_argument("--snps", type=int, default=62500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matvec", "bench_matvec.json"))
    args = ap.parse_args()

    from pysnptools_amd import _native as N

    n, m = args.iids, args.snps
    name = ctypes.create_string_buffer(128)
    mem, cus = ctypes.c_uint64(0), ctypes.c_int(0)
    N.call("snpmi_device_info", 0, name, 128, ctypes.byref(mem), ctypes.byref(cus))
    valu = cus.value * 64 * args.ghz * 1e9
    out = {"bench": "matvec", "box": {"gpu": name.value.decode(errors="replace"), "cus": cus.value},
           "iid_count": n, "sid_count": m, "reps": args.reps, "valu_lane_ops_per_s": valu}
    pitch = int(N.lib().snpmi_packed_pitch(n))
    nbytes = pitch * m
    packed = bench.Dev(N, nbytes)
    bench.synth(N, packed.p, pitch, n, 0, m, 41, 0.02)
    ev = bench.Events(N, 2)

    other = bench.Dev(N, nbytes)
    t_copy = best_ms(N, ev, args.reps, lambda: N.call("snpmi_dev_memcpy_d2d", other.p, packed.p, nbytes))
    other.free()
    copy_rate = 2 * nbytes / (t_copy * 1e-3)
    out["packed_gb"] = round(nbytes / 1e9, 4)
    out["copy"] = {"ms": round(t_copy, 4), "traffic_gb_per_s": round(copy_rate / 1e9, 1)}
    note("copy", out["copy"])

    # what materializing Z alone costs (fused stats + decode, f32 F order)
    ld = (n + 15) // 16 * 16
    lut, stats = bench.Dev(N, m * 16), bench.Dev(N, m * 8)
    free, total = ctypes.c_uint64(), ctypes.c_uint64()
    N.call("snpmi_device_memory", ctypes.byref(free), ctypes.byref(total))
    mz = min(m, int(free.value * 0.8) // (ld * 4))
    Z = bench.Dev(N, ld * mz * 4)
    t_dec = best_ms(N, ev, args.reps, lambda: N.call(
        "snpmi_dev_decode_standardize", packed.p, pitch, n, mz, 0, N.STD_UNIT, 0.0, 0.0, 0, N.DT_F32, stats.p, lut.p,
        Z.p, ld))
    Z.free()
    out["decode_standardize_f32"] = {"snps": mz, "ms": round(t_dec, 3), "z_gb": round(ld * mz * 4 / 1e9, 2),
                                     "written_gb_per_s": round(ld * mz * 4 / (t_dec * 1e-3) / 1e9, 1)}
    note("decode_standardize", out["decode_standardize_f32"])
    lut.free()
    stats.free()

    rng = np.random.default_rng(0)
    legs = []
    for dtype in (np.dtype(np.float32), np.dtype(np.float64)):
        dt, item = N.dt_code(dtype), dtype.itemsize
        lut, stats = bench.Dev(N, m * 4 * item), bench.Dev(N, m * 2 * item)
        N.call("snpmi_dev_snp_stats", packed.p, pitch, n, m, 0, N.STD_UNIT, 0.0, 0.0, 0, dt, stats.p, lut.p)
        for k in args.ks:
            V, G, Y = bench.Dev(N, n * k * item), bench.Dev(N, m * k * item), bench.Dev(N, n * k * item)
            host = rng.standard_normal((k, n)).astype(dtype)
            N.call("snpmi_memcpy_h2d", V.p, N.ptr(host), host.nbytes)

            def tdot():
                N.call("snpmi_dev_packed_tdot", packed.p, pitch, n, m, lut.p, dt, V.p, n, k, G.p, m)

            def dot():
                N.call("snpmi_dev_packed_dot", packed.p, pitch, n, m, lut.p, dt, G.p, m, k, Y.p, n, 0)

            def both():
                tdot()
                dot()

            for leg, fn, products in (("tdot", tdot, 1), ("dot", dot, 1), ("kernel_matmat", both, 2)):
                ms = best_ms(N, ev, args.reps, fn)
                sec = ms * 1e-3
                t_mem = products * nbytes / copy_rate
                t_valu = products * n * m * (k + 3) / valu
                row = {"leg": leg, "dtype": dtype.name, "k": k, "ms": round(ms, 3),
                       "packed_gb_per_s": round(products * nbytes / sec / 1e9, 1),
                       "copy_traffic_gb_per_s": round(copy_rate / 1e9, 1),
                       "fma_per_s": float("%.4g" % (products * n * m * k / sec)),
                       "bound_ms": round(max(t_mem, t_valu) * 1e3, 3), "limit": "valu" if t_valu > t_mem else "memory",
                       "fraction_of_bound": round(max(t_mem, t_valu) / sec, 3)}
                legs.append(row)
                note(row)
            for b in (V, G, Y):
                b.free()
        lut.free()
        stats.free()
    out["legs"] = legs
    ev.destroy()
    packed.free()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
