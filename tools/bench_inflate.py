"""Device-side inflate (csrc/inflate.hip) beside the host route it replaces, in one process.

The file has the shape of tools/bench_bgen.py's inflate leg -- ``--iids`` samples at 16 bits, zlib,
written once with ``Bgen.write`` from a ``DistGen`` -- and one JSON line is printed:

* ``host_inflate``: pread + ``zlib.decompress`` + the host checks of ``--blocks`` blocks on the reader's
  thread pool (bench_bgen's leg, unchanged);
* ``pread`` / ``upload``: the stored bytes of those blocks read into the page-locked buffer on the same
  pool, and their copy to HBM;
* ``dev_inflate``: one ``snpmi_dev_inflate`` over them (best of ``--reps`` after a warm-up; synchronous,
  with its table upload and status read-back): seconds, GB/s of inflated bytes, and symbols per second
  from the symbol count of ``--sample`` blocks walked by the small pure-Python counter below;
* ``dev_check``: one ``snpmi_dev_bgen_check`` over the inflated blocks;
* ``read_kernel``: ``Bgen(...).as_snp().read_kernel(Unit(), dtype=float32)`` at ``--iids`` x ``--snps``
  under ``inflate="host"`` and ``inflate="device"``, alternated ``--kernel-reps`` times, and whether the
  two kernels are the same bits.

Usage: python tools/bench_inflate.py [--reps 3] [--iids 50000] [--snps 8192] [--blocks 2048]
                                     [--sample 2] [--kernel-reps 2] [--skip-kernel] [--dir DIR]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_bgen import best_of, note, run_inflate  # noqa: E402


def count_symbols(stream):
    """Huffman symbols (literals, length/distance pairs counted once, end-of-block codes) of a zlib
    stream, and its stored-block bytes: a bit-by-bit walk, for a handful of blocks only."""
    bits = np.unpackbits(np.frombuffer(stream, dtype=np.uint8), bitorder="little").tolist()
    at = 16
    lbase_extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dextra = [0] * 4 + [e for e in range(1, 14) for _ in range(2)]

    def take(n):
        nonlocal at
        v = 0
        for k in range(n):
            v |= bits[at + k] << k
        at += n
        return v

    def table(lens):
        count = [0] * 16
        for ln in lens:
            count[ln] += 1
        count[0] = 0
        offs = [0] * 17
        for ln in range(1, 16):
            offs[ln + 1] = offs[ln] + count[ln]
        sym = [0] * len(lens)
        for s, ln in enumerate(lens):
            if ln:
                sym[offs[ln]] = s
                offs[ln] += 1
        return count, sym

    def decode(t):
        nonlocal at
        count, sym = t
        code = first = index = 0
        for ln in range(1, 16):
            code |= bits[at]
            at += 1
            c = count[ln]
            if code - c < first:
                return sym[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise ValueError("bad code")

    symbols = stored = 0
    last = 0
    while not last:
        last, kind = take(1), take(2)
        if kind == 0:
            at = (at + 7) // 8 * 8
            n = take(16)
            at += 16 + 8 * n
            stored += n
            continue
        if kind == 1:
            lt, dt = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 30)
        else:
            hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][k]] = take(3)
            ct, lens = table(cl), []
            while len(lens) < hlit + hdist:
                s = decode(ct)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + take(2))
                else:
                    lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
            lt, dt = table(lens[:hlit]), table(lens[hlit:])
        while True:
            s = decode(lt)
            symbols += 1
            if s == 256:
                break
            if s > 256:
                at += lbase_extra[s - 257]
                extra = dextra[decode(dt)]  # (decode moves `at`: not inside an augmented assignment to it)
                at += extra
    return symbols, stored


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iids", type=int, default=50000)
    ap.add_argument("--snps", type=int, default=8192)
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--sample", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=2)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()

    from pysnptools_amd import _native as N
    from pysnptools_amd import hbm
    from pysnptools_amd.distreader import Bgen, DistGen
    from pysnptools_amd.standardizer import Unit
    from pysnptools_amd.util import get_num_threads

    name = ctypes.create_string_buffer(128)
    mem, cus = ctypes.c_uint64(0), ctypes.c_int(0)
    N.call("snpmi_device_info", 0, name, 128, ctypes.byref(mem), ctypes.byref(cus))
    out = {"bench": "inflate", "box": {"gpu": name.value.decode(errors="replace"), "cus": cus.value}}
    with tempfile.TemporaryDirectory(dir=args.dir) as folder:
        m = args.blocks if args.skip_kernel else max(args.snps, args.blocks)
        t0 = time.perf_counter()
        host = Bgen.write(os.path.join(folder, "cohort.bgen"), DistGen(seed=332, iid_count=args.iids, sid_count=m),
                          bits=16, compression="zlib", block_size=64)
        out["write"] = {"iid_count": args.iids, "snps": m, "seconds": round(time.perf_counter() - t0, 1),
                        "file_gb": round(os.path.getsize(host.filename) / 1e9, 3)}
        note("write", out["write"])
        host._run_once()
        threads = get_num_threads(None)
        count = args.blocks
        out["host_inflate"] = run_inflate(host, count, threads)
        note("host_inflate", out["host_inflate"])

        # the device route's stages, one by one, over the same blocks
        dev = Bgen(host.filename, inflate="device")
        dev._run_once()
        at, stored, lengths = (dev._rec[:count, k] for k in range(3))
        src = np.concatenate(([0], np.cumsum(stored)))
        offsets = np.concatenate(([0], np.cumsum((lengths + 7) // 8 * 8)))
        src_total, total = int(src[-1]), int(offsets[-1]) + 16
        from pysnptools_amd.distreader.bgen import _Staging

        staging = _Staging()
        staging.reserve(src_total)
        view = staging.view

        def read_all():
            dev._map(threads, lambda k: os.preadv(dev._fd, [view[int(src[k]):int(src[k + 1])]], int(at[k])), count)

        t_read = best_of(1, read_all)
        t_up = best_of(args.reps, lambda: N.call("snpmi_memcpy_h2d", N.ptr(staging.dev), staging.host, src_total))
        blocks = hbm.zeros((total,), dtype=np.uint8)
        table = np.empty((count, 4), dtype=np.uint64)
        table[:, 0], table[:, 1], table[:, 2], table[:, 3] = src[:-1], stored, offsets[:-1], lengths
        status = np.zeros(count, dtype=np.uint32)
        t_inf = best_of(args.reps, lambda: N.call("snpmi_dev_inflate", N.ptr(staging.dev), src_total, N.ptr(blocks),
                                                  total, N.ptr(table), count, N.ptr(status)))
        assert not status.any(), "a block did not inflate"
        rec = np.zeros((count, 10), dtype=np.uint64)
        pairs = np.ascontiguousarray(table[:, 2:])
        t_chk = best_of(args.reps, lambda: N.call("snpmi_dev_bgen_check", N.ptr(blocks), total, N.ptr(pairs), count,
                                                  args.iids, N.ptr(rec)))
        assert np.all(rec[:, 0] == 0) and np.all(rec[:, 1] == 16) and np.all(rec[:, 9] == lengths.astype(np.uint64))
        # the inflated bytes are the host route's
        data, _ = host._inflate(count - 1)
        got = blocks.get()[int(offsets[count - 1]):int(offsets[count - 1]) + len(data)].tobytes()
        assert got == data, "device and host inflate disagree"
        sampled = [count_symbols(bytes(view[int(src[k]):int(src[k + 1])])) for k in range(min(args.sample, count))]
        per_block = float(np.mean([s for s, _ in sampled])) if sampled else 0.0
        inflated = int(lengths.sum())
        out["pread"] = {"blocks": count, "threads": threads, "stored_gb": round(src_total / 1e9, 3),
                        "seconds": round(t_read, 4)}
        out["upload"] = {"stored_gb": round(src_total / 1e9, 3), "seconds": round(t_up, 5),
                         "gb_per_s": round(src_total / t_up / 1e9, 1)}
        out["dev_inflate"] = {"blocks": count, "stored_gb": round(src_total / 1e9, 3),
                              "inflated_gb": round(inflated / 1e9, 3), "seconds": round(t_inf, 5),
                              "inflated_gb_per_s": round(inflated / t_inf / 1e9, 2),
                              "symbols_per_block_sampled": round(per_block, 1), "blocks_sampled": len(sampled),
                              "stored_block_bytes_sampled": int(sum(b for _, b in sampled)),
                              "symbols_per_s": round(per_block * count / t_inf, 1),
                              "speedup_over_host_inflate": round(out["host_inflate"]["seconds"] / t_inf, 2)}
        out["dev_check"] = {"blocks": count, "seconds": round(t_chk, 6),
                            "read_gb_per_s": round(count * args.iids / t_chk / 1e9, 1)}
        out["device_stages_seconds"] = round(t_read + t_up + t_inf + t_chk, 4)
        note({k: out[k] for k in ("pread", "upload", "dev_inflate", "dev_check")})
        staging.release()
        del blocks

        if not args.skip_kernel:
            res = {"iid_count": args.iids, "snps": args.snps, "bits": 16, "dtype": "float32", "host_s": [], "device_s": []}
            kernels = {}
            for reader in (host, dev):
                reader[:, :4].as_snp().read_kernel(Unit(), dtype=np.float32)  # warm-up: scratch, staging, K pages
            for _ in range(args.kernel_reps):
                for key, reader in (("host", host), ("device", dev)):
                    t0 = time.perf_counter()
                    kernels[key] = reader[:, :args.snps].as_snp().read_kernel(Unit(), dtype=np.float32).val
                    res[key + "_s"].append(round(time.perf_counter() - t0, 3))
                    note("read_kernel", key, res[key + "_s"][-1])
            res["same_values"] = bool(np.array_equal(kernels["host"], kernels["device"]))
            res["host_best_s"], res["device_best_s"] = min(res["host_s"]), min(res["device_s"])
            res["speedup"] = round(res["host_best_s"] / res["device_best_s"], 3)
            out["read_kernel"] = res
        host.flush()
        dev.flush()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
