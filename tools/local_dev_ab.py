"""Measure the short-circuit reader's delivery into device memory (hdfs3_local_reader_read_dev) against
what a caller who wants a local block's bytes on the GPU had to do before it.

A block file of --mib MiB (default 128) and its .meta (512 B chunks) are written to a temporary directory
and read once, so the page cache is warm. A reader with the default buffer and window sizes is opened per
pass and the block is read in calls of 4 MiB and in one call, by two legs that alternate pass by pass:
  read_dev     hdfs3_local_reader_read_dev straight into a device buffer
  read_h2d     per call: hdfs3_local_reader_read into a pinned host buffer, then hdfs3_memcpy_h2d of what
               it returned to the device buffer
Per pass: GiB/s of block data (open and close of the reader outside the clock, the last byte in device
memory inside it) and this process's CPU seconds per GiB (getrusage, user + system, every thread). After
every pass the device buffer is downloaded and compared with the file, byte for byte.

The kernel's own cost is measured apart: --launches (default 200) back-to-back calls of one aligned 4 MiB
range, ended by one synchronise, through hdfs3_deliver_verified_dev_async (behind a clean result word, gate
words alternating) and through hdfs3_gather_dev_async, alternating, on a warmed device: microseconds per call
by the host clock around the loop, which at this size is the rate at which the stream takes launches.

One JSON line per pass and one summary line per (call size, leg) with medians over the passes (DESIGN.md
§5.7; builder-measured, never bench `value`). --out DIR also writes them to DIR/local_dev_ab.jsonl."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import resource
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

GIB = 1 << 30
LEGS = ("read_dev", "read_h2d")
BPC = 512


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import CrcContext, DeviceBuffer, LocalBlockReader
    from util import oracle_compute, splitmix_bytes

    lib = _native.lib()
    total = args.mib << 20
    data = splitmix_bytes(total, 0x10CA)
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    with tempfile.TemporaryDirectory() as tmp, CrcContext(0) as ctx:
        d_path, m_path = os.path.join(tmp, "blk"), os.path.join(tmp, "blk.meta")
        with open(d_path, "wb") as f:
            f.write(data.tobytes())
        with open(m_path, "wb") as f:
            f.write(struct.pack(">hBI", 1, 2, BPC) + oracle_compute(data, BPC).tobytes())
        assert np.array_equal(np.fromfile(d_path, dtype=np.uint8), data)  # and the page cache is warm

        dev = DeviceBuffer(total)
        p_host = ctypes.c_void_p()
        assert lib.hdfs3_host_malloc_pinned(ctypes.byref(p_host), total) == 0
        host = p_host.value

        def one_pass(leg, call):
            ctx.memset(dev, 0, total)
            with LocalBlockReader(d_path, m_path) as r:
                rd, rdev, h2d, rr, cx, d = (lib.hdfs3_local_reader_read, lib.hdfs3_local_reader_read_dev,
                                            lib.hdfs3_memcpy_h2d, r.r, ctx.ctx, dev.ptr)
                calls = 0
                c0, t0 = cpu_seconds(), time.perf_counter()
                pos = 0
                while pos < total:
                    n = min(call, total - pos)
                    if leg == "read_dev":
                        got = rdev(rr, d + pos, n)
                    else:
                        got = rd(rr, host, n)
                        if got > 0:
                            assert h2d(cx, d + pos, host, got) == 0
                    assert got > 0, (leg, pos, got)
                    pos += got
                    calls += 1
                dt, cpu = time.perf_counter() - t0, cpu_seconds() - c0
                st = r.device_stats()
            assert np.array_equal(ctx.download(dev, total), data), (leg, call)
            assert st["bytes_delivered"] == (total if leg == "read_dev" else 0)
            return {"GiB_per_s": round(total / dt / GIB, 3), "client_cpu_s_per_gib": round(cpu * GIB / total, 4),
                    "calls": calls, "deliver_launches": st["deliver_launches"]}

        sizes = (4 << 20, total)
        results = {}
        for call in sizes:
            for leg in LEGS:  # warm-up: resources pooled, code objects loaded
                one_pass(leg, call)
        for rep in range(args.passes):  # the legs alternate, pass by pass
            for call in sizes:
                for leg in LEGS:
                    r = one_pass(leg, call)
                    results.setdefault((call, leg), []).append(r)
                    emit({"case": "local_dev_ab_pass", "call_bytes": call, "leg": leg, "pass": rep, "bytes": total,
                          "bpc": BPC, "checked": True, **r})
        for (call, leg), rs in results.items():
            med = {k: statistics.median(r[k] for r in rs) for k in ("GiB_per_s", "client_cpu_s_per_gib")}
            emit({"case": "local_dev_ab", "call_bytes": call, "leg": leg, "passes": len(rs), "bytes": total, "bpc": BPC,
                  **med, "GiB_per_s_min_max": [min(r["GiB_per_s"] for r in rs), max(r["GiB_per_s"] for r in rs)],
                  "calls": rs[0]["calls"], "deliver_launches": rs[0]["deliver_launches"]})
        for call in sizes:
            a, b = (statistics.median(r["GiB_per_s"] for r in results[(call, leg)]) for leg in LEGS)
            ca, cb = (statistics.median(r["client_cpu_s_per_gib"] for r in results[(call, leg)]) for leg in LEGS)
            emit({"case": "read_dev_over_read_h2d", "call_bytes": call, "rate_ratio": round(a / b, 3),
                  "client_cpu_ratio": round(ca / cb, 3) if cb else None})

        # ---- the kernel alone: a guarded delivery against the plain gather, one aligned 4 MiB range ---------
        n = 4 << 20
        src, dst, words = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(24)
        ctx.upload(data[:n], src)
        ctx.memset(words, 0, 24)
        rng = (_native.CopyRange * 1)()
        rng[0].src_off, rng[0].dst_off, rng[0].len = 0, 0, n
        guards = [_native.DeliverGuard(words.ptr, words.ptr + 8 + 8 * i, words.ptr + 16 - 8 * i, 0, 0, 1 << 20, BPC)
                  for i in range(2)]
        deliver, gather, cx = lib.hdfs3_deliver_verified_dev_async, lib.hdfs3_gather_dev_async, ctx.ctx

        def launches(kind, count):
            t0 = time.perf_counter()
            if kind == "deliver":
                for i in range(count):
                    assert deliver(cx, dst.ptr, n, src.ptr, n, rng, 1, ctypes.byref(guards[i & 1])) == 0
            else:
                for i in range(count):
                    assert gather(cx, dst.ptr, n, src.ptr, n, rng, 1) == 0
            ctx.synchronize()
            return (time.perf_counter() - t0) / count * 1e6

        per = {"deliver": [], "gather": []}
        for kind in per:
            launches(kind, args.launches)  # warm-up
        for rep in range(args.passes):
            for kind in per:
                per[kind].append(launches(kind, args.launches))
        assert np.array_equal(ctx.download(dst, n), data[:n])
        med = {k: statistics.median(v) for k, v in per.items()}
        emit({"case": "deliver_vs_gather_4MiB", "launches_per_pass": args.launches, "passes": args.passes,
              "deliver_us_per_call": round(med["deliver"], 3), "gather_us_per_call": round(med["gather"], 3),
              "deliver_us_min_max": [round(min(per["deliver"]), 3), round(max(per["deliver"]), 3)],
              "gather_us_min_max": [round(min(per["gather"]), 3), round(max(per["gather"]), 3)],
              "guard_cost_us": round(med["deliver"] - med["gather"], 3),
              "deliver_GiB_per_s": round(n / (med["deliver"] * 1e-6) / GIB, 1),
              "gather_GiB_per_s": round(n / (med["gather"] * 1e-6) / GIB, 1)})
        for b in (src, dst, words, dev):
            b.free()
        lib.hdfs3_host_free_pinned(p_host)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "local_dev_ab.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
