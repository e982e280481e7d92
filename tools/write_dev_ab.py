"""Measure the output stream's write from device memory (hdfs3_output_write_dev) against what a caller
whose data is in HBM had to do before it.

--gib GiB (default 1) are written through an hdfs3_output_stream (128 MiB blocks, 512 B chunks, 64-packet
batches) into a C sink, in calls of 4 MiB and of 64 KiB, by three legs that alternate pass by pass:
  write        hdfs3_output_write from a pinned host buffer (the data never was on the GPU)
  d2h_write    per call: the bytes copied from device memory into a pinned bounce buffer (synchronous
               copy), then hdfs3_output_write of the bounce buffer
  write_dev    hdfs3_output_write_dev straight from device memory
Per pass: GiB/s of user data, this process's CPU seconds per GiB (getrusage, user + system), and the median
and 90th percentile wall time of one call (the 64 KiB rows show what write_dev's one event wait per call
costs). Every pass is checked: with --sink compare (default) the sink compares every packet's data with
the source at its position, byte for byte; with --sink count (the sink of the other write measurements,
which reads one byte per cache line) the packet and wire-byte counts are checked. --sink both runs both.

One JSON line per pass and one summary line per (sink, call size, leg) with medians over the passes
(builder-measured, never bench `value`). --out DIR also writes them to
DIR/write_dev_ab.jsonl."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import resource
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

GIB = 1 << 30
LEGS = ("write", "d2h_write", "write_dev")
BLOCK = 128 << 20
D2H = 2  # hipMemcpyDeviceToHost


def hip_runtime():
    try:
        l = ctypes.CDLL("libamdhip64.so")
    except OSError:
        l = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    l.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    l.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    l.hipHostFree.argtypes = [ctypes.c_void_p]
    return l


def pinned(hip, nbytes):
    p = ctypes.c_void_p()
    rc = hip.hipHostMalloc(ctypes.byref(p), nbytes, 0)
    if rc != 0:
        raise RuntimeError(f"hipHostMalloc: HIP error {rc}")
    return p, np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def expected_packets(total):
    """every block: ceil(chunks / 127) data packets + its empty last packet (512 B chunks, 64 KiB packets)"""
    n = 0
    for off in range(0, total, BLOCK):
        n += -(-(min(BLOCK, total - off) // 512) // 127) + 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--sink", choices=("compare", "count", "both"), default="compare")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import CrcContext, DeviceBuffer, OutputStream
    from util import splitmix_bytes

    lib, lb, hip = _native.lib(), _native.loopback(), hip_runtime()
    sinks = {"compare": ctypes.cast(lb.hdfs3_loopback_compare_sink, ctypes.c_void_p).value,
             "count": ctypes.cast(lb.hdfs3_loopback_count_sink, ctypes.c_void_p).value}
    total = int(args.gib * GIB) // (4 << 20) * (4 << 20)
    source = splitmix_bytes(total, 0xDE)
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    with CrcContext(0) as ctx:
        p_host, host = pinned(hip, total)
        host[:] = source
        p_bounce, _ = pinned(hip, 4 << 20)
        dev = DeviceBuffer(total)
        for off in range(0, total, 256 << 20):
            ctx.upload(source[off:off + (256 << 20)], dev, off)

        def one_pass(leg, call, sink_kind):
            user = (ctypes.c_uint64 * 6)()
            if sink_kind == "compare":
                user[0] = source.ctypes.data
            s =OutputStream(block_size=BLOCK, batch_packets=args.batch, raw_sink=sinks[sink_kind],
                             raw_user=ctypes.addressof(user))
            h, w, wd, st = p_host.value, lib.hdfs3_output_write, lib.hdfs3_output_write_dev, s.s
            bounce, d = p_bounce.value, dev.ptr
            per_call = np.zeros(total // call)
            clock = time.perf_counter
            c0, t0 = cpu_seconds(), clock()
            t = t0
            for i, off in enumerate(range(0, total, call)):
                if leg == "write":
                    got = w(st, h + off, call)
                elif leg == "d2h_write":
                    rc = hip.hipMemcpy(bounce, d + off, call, D2H)
                    assert rc == 0, rc
                    got = w(st, bounce, call)
                else:
                    got = wd(st, d + off, call)
                assert got == call, (leg, off, got)
                t1 = clock()
                per_call[i] = t1 - t
                t = t1
            dstats = s.device_stats()
            batches = s.stats()["gpu_batches"]
            s.close()
            dt, cpu = clock() - t0, cpu_seconds() - c0
            if sink_kind == "compare":
                assert user[1] == total and user[4] == 0, (leg, call, "position", user[1], "bad packets", user[4],
                                                           "first bad seqno", int(user[5]) - 1)
                packets, wire = int(user[2]), int(user[3])
            else:
                packets, wire = int(user[0]), int(user[1])
            assert packets == expected_packets(total), (packets, expected_packets(total))
            assert wire == total + 4 * (total // 512) + 31 * packets, wire
            assert dstats["bytes_from_device"] == (total if leg == "write_dev" else 0)
            return {"GiB_per_s": round(total / dt / GIB, 3), "client_cpu_s_per_gib": round(cpu * GIB / total, 4),
                    "call_us_median": round(float(np.median(per_call)) * 1e6, 2),
                    "call_us_p90": round(float(np.percentile(per_call, 90)) * 1e6, 2),
                    "scatter_launches": dstats["scatter_launches"], "gpu_batches": batches}

        kinds = ("compare", "count") if args.sink == "both" else (args.sink,)
        calls = (4 << 20, 64 << 10)
        results = {}
        for kind in kinds:
            for call in calls:
                for leg in LEGS:  # warm-up: arenas pooled, pages touched
                    one_pass(leg, call, kind)
            for rep in range(args.passes):  # the legs alternate, pass by pass
                for call in calls:
                    for leg in LEGS:
                        r = one_pass(leg, call, kind)
                        results.setdefault((kind, call, leg), []).append(r)
                        emit({"case": "write_dev_ab_pass", "sink": kind, "call_bytes": call, "leg": leg, "pass": rep,
                              "bytes": total, "batch_packets": args.batch, "checked": True, **r})
        for (kind, call, leg), rs in results.items():
            med = {k: statistics.median(r[k] for r in rs) for k in ("GiB_per_s", "client_cpu_s_per_gib", "call_us_median",
                                                                     "call_us_p90")}
            emit({"case": "write_dev_ab", "sink": kind, "call_bytes": call, "leg": leg, "passes": len(rs), "bytes": total,
                  "batch_packets": args.batch, **med,
                  "GiB_per_s_min_max": [min(r["GiB_per_s"] for r in rs), max(r["GiB_per_s"] for r in rs)],
                  "scatter_launches": rs[0]["scatter_launches"], "gpu_batches": rs[0]["gpu_batches"]})
        for kind in kinds:
            for call in calls:
                b, c = (statistics.median(r["GiB_per_s"] for r in results[(kind, call, leg)]) for leg in LEGS[1:])
                cb, cc = (statistics.median(r["client_cpu_s_per_gib"] for r in results[(kind, call, leg)])
                          for leg in LEGS[1:])
                emit({"case": "write_dev_over_d2h_write", "sink": kind, "call_bytes": call, "rate_ratio": round(c / b, 3),
                      "client_cpu_ratio": round(cc / cb, 3) if cb else None})
        dev.free()
        hip.hipHostFree(p_host)
        hip.hipHostFree(p_bounce)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "write_dev_ab.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
