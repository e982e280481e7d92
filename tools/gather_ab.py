"""Measure the range gather (csrc/crc32c_gather.hip) and the block reader's device delivery.

  gather   one gather launch against the runtime's device-to-device copies of the same ranges on the same
           stream, for the reader's two batch shapes (1 x 4 MiB aligned; 64 x 64 KiB with a 7-byte relative
           misalignment), alternating regions of --iters repetitions between two events, medians of --reps
           regions, after a warm-up region of each. And the kernel's roofline row: one 256 MiB range
           against a 256 MiB runtime copy (algorithmic bytes 2 x len).
  reader   a --gib GiB loopback block (datanode in a child process, started before the GPU is touched) read
           with hdfs3_block_reader_read and with hdfs3_block_reader_read_dev, alternating passes: rate,
           this process's CPU time per GiB and the reader's phase counters (hdfs3_reader_phase_ns).

One JSON line per measurement (builder-measured, never bench `value`)."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))  # loopback helper

GIB = 1 << 30
D2D = 3  # hipMemcpyDeviceToDevice
PHASES = ("receive", "alloc", "launch", "wait", "copy_out", "rx_idle", "caller_idle", "rx_cpu")


class Hip:
    """The few runtime calls the baseline needs, straight from libamdhip64 (no wrapper's host overhead)."""

    def __init__(self):
        try:
            self.l = ctypes.CDLL("libamdhip64.so")
        except OSError:
            self.l = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.l.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        self.l.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.l.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.l.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.l.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def event(self):
        e = ctypes.c_void_p()
        self.ok(self.l.hipEventCreate(ctypes.byref(e)))
        return e

    def region_ms(self, stream, e0, e1, body, iters):
        self.ok(self.l.hipEventRecord(e0, stream))
        for _ in range(iters):
            body()
        self.ok(self.l.hipEventRecord(e1, stream))
        self.ok(self.l.hipEventSynchronize(e1))
        ms = ctypes.c_float()
        self.ok(self.l.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        return ms.value


def gather_cases(args):
    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import CrcContext, DeviceBuffer

    hip = Hip()
    shapes = {
        "1x4MiB": [(4096, 0, 4 << 20)],
        "64x64KiB_mis7": [(4096 + i * 66064 + 7, i * 65536, 65536) for i in range(64)],
        "1x256MiB": [(0, 0, 256 << 20)],
    }
    with CrcContext(0) as ctx:
        stream = ctypes.c_void_p(_native.lib().hdfs3_crc_ctx_get_stream(ctx.ctx))
        e0, e1 = hip.event(), hip.event()
        for name, ranges in shapes.items():
            total = sum(r[2] for r in ranges)
            src_len = max(r[0] + r[2] for r in ranges) + 64
            src = np.random.default_rng(3).integers(0, 256, src_len, dtype=np.uint8)
            d_src, d_a, d_b = ctx.upload(src), DeviceBuffer(total), DeviceBuffer(total)
            arr = ctx._ranges(ranges)
            lib, n = ctx._lib, len(ranges)

            def gather():
                rc = lib.hdfs3_gather_dev_async(ctx.ctx, d_a.ptr, total, d_src.ptr, src_len, arr, n)
                assert rc == 0, rc

            def copies():
                for s, d, ln in ranges:
                    hip.ok(hip.l.hipMemcpyAsync(d_b.ptr + d, d_src.ptr + s, ln, D2D, stream))

            gather()
            copies()
            ctx.synchronize()
            assert np.array_equal(ctx.download(d_a, total), ctx.download(d_b, total)), name
            iters = max(1, min(args.iters, (8 << 30) // total))
            for body in (gather, copies):  # warm-up regions
                hip.region_ms(stream, e0, e1, body, iters)
            tg, tc = [], []
            for _ in range(args.reps):  # alternating regions
                tg.append(hip.region_ms(stream, e0, e1, gather, iters) * 1e3 / iters)
                tc.append(hip.region_ms(stream, e0, e1, copies, iters) * 1e3 / iters)
            g, c = statistics.median(tg), statistics.median(tc)
            print(json.dumps({"case": "gather_vs_runtime_copies", "shape": name, "ranges": n, "bytes": total,
                              "iters_per_region": iters, "regions": args.reps,
                              "gather_us": round(g, 3), "gather_us_min_max": [round(min(tg), 3), round(max(tg), 3)],
                              "runtime_copies_us": round(c, 3),
                              "runtime_copies_us_min_max": [round(min(tc), 3), round(max(tc), 3)],
                              "gather_over_copies_time": round(g / c, 3),
                              "gather_algorithmic_TBps": round(2 * total / g / 1e6, 3),
                              "runtime_copy_algorithmic_TBps": round(2 * total / c / 1e6, 3),
                              "gather_fraction_of_copy_rate": round(c / g, 3)}), flush=True)
            for b in (d_src, d_a, d_b):
                b.free()


def reader_case(args, dn, served):
    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import BlockReader, CrcContext, DeviceBuffer

    lib = _native.lib()
    n = served.nbytes
    chunk = 4 << 20
    host = np.zeros(n, np.uint8)
    with CrcContext(0) as ctx:
        dev = DeviceBuffer(n)

        def one_pass(device):
            ph = (ctypes.c_uint64 * 8)()
            lib.hdfs3_reader_phase_ns(ph, 8, 1)
            c0, t0 = time.process_time(), time.perf_counter()
            with BlockReader("127.0.0.1", dn.port, 1, 0, n, batch_packets=args.batch) as r:
                pos = 0
                while pos < n:
                    got = (r.read_into_device(dev.ptr + pos, min(chunk, n - pos)) if device
                           else r.read_into(host, pos, min(chunk, n - pos)))
                    assert got > 0
                    pos += got
                st = r.device_stats()
            dt, cpu = time.perf_counter() - t0, time.process_time() - c0
            lib.hdfs3_reader_phase_ns(ph, 8, 1)
            return {"path": "read_dev" if device else "read", "GiB_per_s": round(n / dt / GIB, 3),
                    "client_cpu_s_per_gib": round(cpu * GIB / n, 4),
                    "reader_phase_s_per_gib": {k: round(ph[i] * 1e-9 * GIB / n, 4) for i, k in enumerate(PHASES)},
                    "gather_launches": st["gather_launches"]}

        for device in (False, True):  # warm-up, and the bytes
            one_pass(device)
        assert np.array_equal(host, served)
        for off in range(0, n, 256 << 20):
            m = min(256 << 20, n - off)
            assert np.array_equal(ctx.download(dev, m, off), served[off:off + m])
        for rep in range(args.passes):
            for device in (False, True):
                print(json.dumps({"case": "reader_client_cpu", "pass": rep, "bytes": n, "batch_packets": args.batch,
                                  **one_pass(device)}), flush=True)
        dev.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--skip-reader", action="store_true")
    ap.add_argument("--skip-gather", action="store_true")
    args = ap.parse_args()
    dn = served = None
    if not args.skip_reader:
        # the datanode child starts before this process touches the GPU
        from loopback import ChildDatanode
        from util import oracle_compute, splitmix_bytes

        n = int(args.gib * GIB) // 65536 * 65536
        data = splitmix_bytes(n, 0xD0)
        dn = ChildDatanode()
        served = dn.share_blocks(data, oracle_compute(data, 512), [(1, 0, n)], 512, tag="gather_ab")
    try:
        if not args.skip_gather:
            gather_cases(args)
        if dn:
            reader_case(args, dn, served)
    finally:
        if dn:
            dn.stop()


if __name__ == "__main__":
    main()
