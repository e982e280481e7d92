"""Measure a local replica read through the input stream (hdfs3_input_set_local_replicas) against the same
stream over a loopback datanode and against the bare short-circuit reader.

One block of --mib MiB (default 128) with 512 B chunks: its block file and .meta are written to a temporary
directory and read once, so the page cache is warm, and a loopback datanode in a child process (started before
this process touches the GPU) serves the same bytes. The block is read into a device buffer in read_dev calls
of 4 MiB by three legs that alternate pass by pass, each with the default buffer, window and batch sizes:
  stream_local   hdfs3_input_read_dev on a stream with the replica registered
  stream_remote  the same stream with no table: OP_READ_BLOCK over loopback (what every stream did before)
  local_reader   hdfs3_local_reader_read_dev on a reader of the block file
The streams are opened outside the clock and open their block reader on the first read, inside it;
local_reader's open is inside the clock as well, so every leg pays for opening its reader. Per pass: GiB/s of block data (the last
byte in device memory inside the clock) and this process's CPU seconds per GiB (getrusage, user + system, every
thread; the datanode's own CPU is the child's and not counted). After every pass the device buffer is
downloaded and compared with the block, byte for byte.

One JSON line per pass, one summary line per leg with medians over the passes, and one line with the ratios
(builder-measured, never bench `value`). --out DIR also writes them to
DIR/input_local_ab.jsonl."""
from __future__ import annotations

import argparse
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
LEGS = ("stream_local", "stream_remote", "local_reader")
BPC = 512
CALL = 4 << 20
BLOCK_ID = 4100


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from loopback import ChildDatanode
    from util import oracle_compute, splitmix_bytes

    total = args.mib << 20
    data = splitmix_bytes(total, 0x10CB)
    words = oracle_compute(data, BPC)
    node = ChildDatanode()  # before anything here opens the GPU
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    try:
        node.share_blocks(data, words, [(BLOCK_ID, 0, total)], BPC, tag="input_local_ab")

        from libhdfs3_amd import _native
        from libhdfs3_amd.engine import CrcContext, DeviceBuffer, InputStream, LocalBlockReader

        lib = _native.lib()
        with tempfile.TemporaryDirectory() as tmp, CrcContext(0) as ctx:
            d_path, m_path = os.path.join(tmp, "blk"), os.path.join(tmp, "blk.meta")
            with open(d_path, "wb") as f:
                f.write(data.tobytes())
            with open(m_path, "wb") as f:
                f.write(struct.pack(">hBI", 1, 2, BPC) + words.tobytes())
            assert np.array_equal(np.fromfile(d_path, dtype=np.uint8), data)  # and the page cache is warm
            dev = DeviceBuffer(total)

            def drain(read, handle):
                pos = calls = 0
                while pos < total:
                    got = read(handle, dev.ptr + pos, min(CALL, total - pos))
                    assert got > 0, (pos, got, lib.hdfs3_crc_last_error())
                    pos += got
                    calls += 1
                return calls

            def one_pass(leg):
                ctx.memset(dev, 0, total)
                extra = {}
                if leg == "local_reader":
                    c0, t0 = cpu_seconds(), time.perf_counter()
                    with LocalBlockReader(d_path, m_path) as r:
                        calls = drain(lib.hdfs3_local_reader_read_dev, r.r)
                        dt, cpu = time.perf_counter() - t0, cpu_seconds() - c0
                else:
                    with InputStream([(BLOCK_ID, total, [("127.0.0.1", node.port)])]) as s:
                        if leg == "stream_local":
                            s.set_local_replicas([(0, 0, d_path, m_path)])
                        c0, t0 = cpu_seconds(), time.perf_counter()
                        calls = drain(lib.hdfs3_input_read_dev, s.s)
                        dt, cpu = time.perf_counter() - t0, cpu_seconds() - c0
                        extra = {**s.local_stats(), "readers_opened": s.stats()["readers_opened"]}
                    assert extra["local_bytes"] == (total if leg == "stream_local" else 0), extra
                    assert extra["readers_opened"] == (0 if leg == "stream_local" else 1), extra
                assert np.array_equal(ctx.download(dev, total), data), leg
                return {"GiB_per_s": round(total / dt / GIB, 3), "client_cpu_s_per_gib": round(cpu * GIB / total, 4),
                        "calls": calls, **extra}

            results = {}
            for leg in LEGS:  # warm-up: resources pooled, code objects loaded
                one_pass(leg)
            for rep in range(args.passes):  # the legs alternate, pass by pass
                for leg in LEGS:
                    r = one_pass(leg)
                    results.setdefault(leg, []).append(r)
                    emit({"case": "input_local_ab_pass", "leg": leg, "pass": rep, "bytes": total, "call_bytes": CALL,
                          "bpc": BPC, "checked": True, **r})
            med = {}
            for leg, rs in results.items():
                med[leg] = {k: statistics.median(r[k] for r in rs) for k in ("GiB_per_s", "client_cpu_s_per_gib")}
                emit({"case": "input_local_ab", "leg": leg, "passes": len(rs), "bytes": total, "call_bytes": CALL,
                      "bpc": BPC, **med[leg], "GiB_per_s_min_max": [min(r["GiB_per_s"] for r in rs),
                                                                    max(r["GiB_per_s"] for r in rs)]})

            def ratio(a, b, key):
                return round(med[a][key] / med[b][key], 3) if med[b][key] else None

            emit({"case": "input_local_ab_ratios",
                  "local_over_remote_rate": ratio("stream_local", "stream_remote", "GiB_per_s"),
                  "local_over_remote_client_cpu": ratio("stream_local", "stream_remote", "client_cpu_s_per_gib"),
                  "local_over_bare_reader_rate": ratio("stream_local", "local_reader", "GiB_per_s"),
                  "local_over_bare_reader_client_cpu": ratio("stream_local", "local_reader", "client_cpu_s_per_gib")})
            dev.free()
    finally:
        node.stop()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "input_local_ab.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
