"""Rates of the SNP-pair kernels (csrc/pairs.hip) at 50,000 iids of synthetic codes (bench.synth)
resident in HBM.  Best of ``--reps`` after a warm-up, HIP events on the compute stream.

``values``: snpmi_dev_pair_values, F order, f32 and f64, 62,500 pairs (the output size of
bench_matvec.py's Z), beside its two ceilings in this process: snpmi_dev_decode of the same output
shape and a device copy of the same bytes.

``tdot``: snpmi_dev_pair_tdot over 1000 x 1000 and 4000 x 4000 SNPs, k in {1, 8}, f32 and f64, beside
* its VALU bound N P (k + 1) / (CUs x 64 lanes x ``--ghz``) -- one multiply and k FMAs per pair value;
* snpmi_dev_packed_tdot's time per output row at the same N and k (a pair's row costs one of those
  plus the pair's own multiply and second decode);
* the time writing those P pair columns with pair_values alone would take, at the rate measured above
  (a figure from that rate: 16 million columns of 50,000 values do not fit anywhere).

One JSON line on stdout, also written to ``--out``.

Usage: python tools/bench_pairs.py [--iids 50000] [--pairs 62500] [--reps 3] [--ghz 2.4]
                                   [--out profiles/pairs/bench_pairs.json]
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
from bench_matvec import best_ms, note  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iids", type=int, default=50000)
    ap.add_argument("--pairs", type=int, default=62500)
    ap.add_argument("--sides", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs", "bench_pairs.json"))
    args = ap.parse_args()

    from pysnptools_amd import _native as N

    n, count = args.iids, args.pairs
    m = max(count, 2 * max(args.sides))  # packed SNPs: the decode's columns, and both sides of the scan
    name = ctypes.create_string_buffer(128)
    mem, cus = ctypes.c_uint64(0), ctypes.c_int(0)
    N.call("snpmi_device_info", 0, name, 128, ctypes.byref(mem), ctypes.byref(cus))
    valu = cus.value * 64 * args.ghz * 1e9
    out = {"bench": "pairs", "box": {"gpu": name.value.decode(errors="replace"), "cus": cus.value},
           "iid_count": n, "reps": args.reps, "valu_lane_ops_per_s": valu}
    pitch = int(N.lib().snpmi_packed_pitch(n))
    packed = bench.Dev(N, pitch * m)
    bench.synth(N, packed.p, pitch, n, 0, m, 41, 0.02)
    ev = bench.Events(N, 2)
    rng = np.random.default_rng(0)
    ld = (n + 15) // 16 * 16

    def at(dev, offset):
        return ctypes.c_void_p(dev.p.value + int(offset))

    idx_host = (np.arange(count, dtype=np.uint32), rng.permutation(count).astype(np.uint32))
    idx0, idx1 = bench.Dev(N, count * 4), bench.Dev(N, count * 4)
    for dev, host in zip((idx0, idx1), idx_host):
        N.call("snpmi_memcpy_h2d", dev.p, N.ptr(host), host.nbytes)

    values, tdot = [], []
    for dtype in (np.dtype(np.float32), np.dtype(np.float64)):
        dt, item = N.dt_code(dtype), dtype.itemsize
        lut, stats = bench.Dev(N, m * 4 * item), bench.Dev(N, m * 2 * item)
        N.call("snpmi_dev_snp_stats", packed.p, pitch, n, m, 0, N.STD_UNIT, 0.0, 0.0, 0, dt, stats.p, lut.p)
        nbytes = ld * count * item
        Z, other = bench.Dev(N, nbytes), bench.Dev(N, nbytes)
        t_val = best_ms(N, ev, args.reps, lambda: N.call(
            "snpmi_dev_pair_values", packed.p, pitch, lut.p, packed.p, pitch, lut.p, n, idx0.p, idx1.p, count, dt, 0,
            Z.p, ld))
        t_dec = best_ms(N, ev, args.reps, lambda: N.call("snpmi_dev_decode", packed.p, pitch, n, count, lut.p, dt, 0,
                                                         Z.p, ld))
        t_copy = best_ms(N, ev, args.reps, lambda: N.call("snpmi_dev_memcpy_d2d", other.p, Z.p, nbytes))
        Z.free()
        other.free()
        row = {"leg": "pair_values", "dtype": dtype.name, "order": "F", "pairs": count, "out_gb": round(nbytes / 1e9, 2),
               "ms": round(t_val, 3), "written_gb_per_s": round(nbytes / (t_val * 1e-3) / 1e9, 1),
               "decode_ms": round(t_dec, 3), "decode_written_gb_per_s": round(nbytes / (t_dec * 1e-3) / 1e9, 1),
               "copy_ms": round(t_copy, 3), "copy_written_gb_per_s": round(nbytes / (t_copy * 1e-3) / 1e9, 1),
               "fraction_of_decode": round(t_dec / t_val, 3), "fraction_of_copy": round(t_copy / t_val, 3)}
        values.append(row)
        note(row)
        ms_per_column = t_val / count

        for side in args.sides:
            pairs = side * side
            for k in args.ks:
                V, G, G1 = bench.Dev(N, n * k * item), bench.Dev(N, pairs * k * item), bench.Dev(N, side * k * item)
                host = rng.standard_normal((k, n)).astype(dtype)
                N.call("snpmi_memcpy_h2d", V.p, N.ptr(host), host.nbytes)
                t = best_ms(N, ev, args.reps, lambda: N.call(
                    "snpmi_dev_pair_tdot", packed.p, pitch, lut.p, side, at(packed, side * pitch), pitch,
                    at(lut, 4 * side * item), side, n, None, None, dt, V.p, n, k, G.p, pairs))
                t_single = best_ms(N, ev, args.reps, lambda: N.call(
                    "snpmi_dev_packed_tdot", packed.p, pitch, n, side, lut.p, dt, V.p, n, k, G1.p, side))
                bound = n * pairs * (k + 1) / valu * 1e3
                row = {"leg": "pair_tdot", "dtype": dtype.name, "n_a": side, "n_b": side, "k": k, "ms": round(t, 3),
                       "pair_rows_per_s": float("%.4g" % (pairs / (t * 1e-3))),
                       "lane_ops_per_s": float("%.4g" % (n * pairs * (k + 1) / (t * 1e-3))),
                       "valu_bound_ms": round(bound, 3), "fraction_of_valu_bound": round(bound / t, 3),
                       "us_per_pair_row": round(t * 1e3 / pairs, 4),
                       "packed_tdot_us_per_row": round(t_single * 1e3 / side, 4),
                       "pair_values_alone_ms": round(ms_per_column * pairs, 1)}
                tdot.append(row)
                note(row)
                for b in (V, G, G1):
                    b.free()
        lut.free()
        stats.free()
    out["values"], out["tdot"] = values, tdot
    ev.destroy()
    for b in (packed, idx0, idx1):
        b.free()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
