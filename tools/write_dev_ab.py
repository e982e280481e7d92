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

The pieces section (--section pieces, or both: the default) is the checkpoint writer's case, many device
buffers that are not neighbours in memory: the same bytes cut into pieces of 4 KiB, 64 KiB and 1 MiB that lie
256 bytes apart in device memory, written by
  d2h_write    one bounce copy + hdfs3_output_write per piece
  write_dev    one hdfs3_output_write_dev per piece
  writev_dev   one hdfs3_output_writev_dev per 64 pieces
with the same sinks and checks; a call's time is reported per call and per piece.

One JSON line per pass and one summary line per (sink, call size, leg) with medians over the passes
(builder-measured, never bench `value`). --out DIR also writes them to
DIR/write_dev_ab.jsonl (--section pieces alone: DIR/writev_dev_ab.jsonl)."""
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
PIECE_LEGS = ("d2h_write", "write_dev", "writev_dev")
PIECES = (4 << 10, 64 << 10, 1 << 20)
PER_CALL = 64   # pieces of one writev_dev call
PIECE_GAP = 256  # bytes between two pieces in device memory: no two are one range
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
    ap.add_argument("--section", choices=("calls", "pieces", "both"), default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import CrcContext, DeviceBuffer, OutputStream
    from util import splitmix_bytes

    lib, lb, hip = _native.lib(), _native.loopback(), hip_runtime()
    sinks = {"compare": ctypes.cast(lb.hdfs3_loopback_compare_sink, ctypes.c_void_p).value,
             "count": ctypes.cast(lb.hdfs3_loopback_count_sink, ctypes.c_void_p).value}
    total = int(args.gib * GIB) // (PER_CALL << 20) * (PER_CALL << 20)  # whole writev_dev calls of 1 MiB pieces
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

        # hdfs3_output_writev_dev with the iovec given as an address: one array holds every call's entries
        wv = ctypes.CFUNCTYPE(ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int)(("hdfs3_output_writev_dev", lib))

        def one_pass(leg, call, sink_kind, pieces=None):
            """pieces = (device address of piece 0, address of a DevIovec per piece): the source is `call`-byte
            pieces PIECE_GAP apart; else the one device buffer"""
            user = (ctypes.c_uint64 * 6)()
            if sink_kind == "compare":
                user[0] = source.ctypes.data
            s =OutputStream(block_size=BLOCK, batch_packets=args.batch, raw_sink=sinks[sink_kind],
                             raw_user=ctypes.addressof(user))
            h, w, wd, st = p_host.value, lib.hdfs3_output_write, lib.hdfs3_output_write_dev, s.s
            bounce, d = p_bounce.value, dev.ptr
            pitch, step = call, call
            if pieces:
                d, iov = pieces
                pitch = call + PIECE_GAP
                if leg == "writev_dev":
                    step = PER_CALL * call
            per_call = np.zeros(total // step)
            clock = time.perf_counter
            c0, t0 = cpu_seconds(), clock()
            t = t0
            for i, off in enumerate(range(0, total, step)):
                if leg == "write":
                    got = w(st, h + off, call)
                elif leg == "d2h_write":
                    rc = hip.hipMemcpy(bounce, d + off // call * pitch, call, D2H)
                    assert rc == 0, rc
                    got = w(st, bounce, call)
                elif leg == "write_dev":
                    got = wd(st, d + off // call * pitch, call)
                else:
                    got = wv(st, iov + off // call * ctypes.sizeof(_native.DevIovec), PER_CALL)
                assert got == step, (leg, off, got)
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
            assert dstats["bytes_from_device"] == (total if leg in ("write_dev", "writev_dev") else 0)
            return {"GiB_per_s": round(total / dt / GIB, 3), "client_cpu_s_per_gib": round(cpu * GIB / total, 4),
                    "call_us_median": round(float(np.median(per_call)) * 1e6, 2),
                    "call_us_p90": round(float(np.percentile(per_call, 90)) * 1e6, 2),
                    "scatter_launches": dstats["scatter_launches"], "gpu_batches": batches}

        kinds = ("compare", "count") if args.sink == "both" else (args.sink,)
        calls = (4 << 20, 64 << 10) if args.section != "pieces" else ()
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
        pres = {}
        for piece in PIECES if args.section != "calls" else ():
            n = total // piece
            gapped = DeviceBuffer(n * (piece + PIECE_GAP))
            img = np.zeros((min(n, (256 << 20) // piece), piece + PIECE_GAP), np.uint8)
            for k in range(0, n, img.shape[0]):  # 256 MiB of pieces at a time
                rows = min(img.shape[0], n - k)
                img[:rows, :piece] = source[k * piece:(k + rows) * piece].reshape(rows, piece)
                ctx.upload(img[:rows], gapped, k * (piece + PIECE_GAP))
            iov = (_native.DevIovec * n)()
            addr = np.ctypeslib.as_array(ctypes.cast(iov, ctypes.POINTER(ctypes.c_uint64)), shape=(n, 2))
            addr[:, 0] = np.uint64(gapped.ptr) + np.arange(n, dtype=np.uint64) * np.uint64(piece + PIECE_GAP)
            addr[:, 1] = piece
            where = (gapped.ptr, ctypes.addressof(iov))
            for kind in kinds:
                for leg in PIECE_LEGS:
                    one_pass(leg, piece, kind, where)
                for rep in range(args.passes):
                    for leg in PIECE_LEGS:
                        r = one_pass(leg, piece, kind, where)
                        per = PER_CALL if leg == "writev_dev" else 1
                        r["piece_us_median"] = round(r["call_us_median"] / per, 3)
                        pres.setdefault((kind, piece, leg), []).append(r)
                        emit({"case": "writev_dev_ab_pass", "sink": kind, "piece_bytes": piece, "pieces_per_call": per,
                              "leg": leg, "pass": rep, "bytes": total, "batch_packets": args.batch, "checked": True, **r})
            gapped.free()
        for (kind, piece, leg), rs in pres.items():
            med = {k: statistics.median(r[k] for r in rs) for k in ("GiB_per_s", "client_cpu_s_per_gib", "call_us_median",
                                                                     "call_us_p90", "piece_us_median")}
            emit({"case": "writev_dev_ab", "sink": kind, "piece_bytes": piece,
                  "pieces_per_call": PER_CALL if leg == "writev_dev" else 1, "leg": leg, "passes": len(rs), "bytes": total,
                  "batch_packets": args.batch, **med,
                  "GiB_per_s_min_max": [min(r["GiB_per_s"] for r in rs), max(r["GiB_per_s"] for r in rs)],
                  "scatter_launches": rs[0]["scatter_launches"], "gpu_batches": rs[0]["gpu_batches"]})
        for kind in kinds if pres else ():
            for piece in PIECES:
                b, c, dd = (statistics.median(r["GiB_per_s"] for r in pres[(kind, piece, leg)]) for leg in PIECE_LEGS)
                emit({"case": "writev_dev_ratios", "sink": kind, "piece_bytes": piece, "writev_over_write_dev": round(dd / c, 3),
                      "writev_over_d2h_write": round(dd / b, 3)})
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
        name = "writev_dev_ab.jsonl" if args.section == "pieces" else "write_dev_ab.jsonl"
        with open(os.path.join(args.out, name), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
