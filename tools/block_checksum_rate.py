"""Time the block checksums (include/hdfs3_crc.h) on one 128 MiB block at 512 B chunks.
"MD5 of CRC32": hdfs3_block_checksum_dev (GPU CRC words + D2H + host MD5) against its host MD5
alone (hdfs3_block_checksum_crcs over the same 1 MiB of words) and hashlib's MD5.
Composite CRC: hdfs3_block_composite_crc_dev (GPU CRC words + their reduction on the GPU, 4 bytes
back), the reduction alone over resident words (one call and its wait; and `--chain` calls with
one wait, per call), and beside it a barriered one-chunk compute launch on the same stream timed the
same two ways (the cost of a launch), and the block's compute launch alone.
One JSON line per case; medians of `--reps` calls after 3 warm-ups."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from libhdfs3_amd.engine import CrcContext, DeviceBuffer, block_checksum_crcs, block_composite_crc_crcs  # noqa: E402


def med(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=128 << 20)
    ap.add_argument("--bpc", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", type=int, default=100)
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, a.bytes, dtype=np.uint8)
    with CrcContext(0) as ctx:
        d = ctx.upload(data)
        crc = ctx.compute(data, a.bpc)
        md5, n = ctx.block_checksum_dev(d.ptr, a.bytes, a.bpc)
        assert md5 == hashlib.md5(crc.tobytes()).digest() == block_checksum_crcs(crc)
        t_dev = med(lambda: ctx.block_checksum_dev(d.ptr, a.bytes, a.bpc), a.reps)
        last = a.bytes - (n - 1) * a.bpc
        assert ctx.block_composite_crc_dev(d.ptr, a.bytes, a.bpc) == block_composite_crc_crcs(crc, a.bpc, last)
        t_comp = med(lambda: ctx.block_composite_crc_dev(d.ptr, a.bytes, a.bpc), a.reps)
        d_crc, d_out, d_one = ctx.upload(crc), DeviceBuffer(4), DeviceBuffer(4)

        def chained(fn, k):
            for _ in range(k):
                fn()
            ctx.synchronize()

        def reduce_words():
            ctx.block_composite_crc_words_dev(d_crc.ptr, n, a.bpc, last, d_out.ptr)

        def one_chunk():
            ctx.compute_dev(d.ptr, a.bpc, a.bpc, d_one.ptr)

        t_red = med(lambda: chained(reduce_words, 1), a.reps)
        t_red_chain = med(lambda: chained(reduce_words, a.chain), a.reps) / a.chain
        t_one = med(lambda: chained(one_chunk, 1), a.reps)
        t_one_chain = med(lambda: chained(one_chunk, a.chain), a.reps) / a.chain
        t_words = med(lambda: chained(lambda: ctx.compute_dev(d.ptr, a.bytes, a.bpc, d_crc.ptr), 1), a.reps)
    t_md5 = med(lambda: block_checksum_crcs(crc), a.reps)
    t_hashlib = med(lambda: hashlib.md5(crc.tobytes()).digest(), a.reps)
    base = {"block_bytes": a.bytes, "bpc": a.bpc, "crc_words": n}
    for case, t in (("hdfs3_block_checksum_dev", t_dev), ("hdfs3_block_checksum_crcs (host MD5 only)", t_md5),
                    ("hashlib.md5 of the words", t_hashlib), ("hdfs3_block_composite_crc_dev", t_comp),
                    ("hdfs3_crc32c_compute_dev + wait (the words alone)", t_words),
                    ("composite reduction of resident words + wait", t_red),
                    (f"composite reduction, per call of {a.chain} chained", t_red_chain),
                    ("one-chunk compute launch + wait", t_one),
                    (f"one-chunk compute launch, per call of {a.chain} chained", t_one_chain)):
        print(json.dumps({**base, "case": case, "ms": round(t * 1e3, 3),
                          "block_GiBps": round(a.bytes / t / 2**30, 2)}), flush=True)


if __name__ == "__main__":
    main()
