"""Composite CRC: the CRC of a whole block or file from its chunk CRCs (include/hdfs3_crc.h).

CPU tests: the host forms through the library against the oracle's CRC of the whole buffer, for both
polynomials, and their argument errors. GPU tests: the reduction kernel (crc32c_compose.hip) over
resident words against the host form, at every word count where the lane / wave / workgroup / grid
tree changes shape, and the form that starts from the block's data against the oracle.
"""
import errno
import os
import re

import numpy as np
import pytest

from util import REPO, oracle_compute, oracle_compute_crc32, oracle_crc, oracle_crc32, splitmix_bytes

# the reduction tree's constants (libhdfs3_amd/csrc/crc32c_kernels.h; test_tree_constants_match_the_kernel)
K = 4           # kComposeLaneWords: words per lane
THREADS = 256   # kComposeThreads: 4 waves per workgroup
SPAN = K * THREADS  # kComposeSpan: words per workgroup, and the fan-in of every further level

CRC32, CRC32C = 1, 2


def whole_crc(data, ctype=CRC32C):
    return oracle_crc(data) if ctype == CRC32C else oracle_crc32(data)


def chunk_words(data, bpc, ctype=CRC32C):
    return oracle_compute(data, bpc) if ctype == CRC32C else oracle_compute_crc32(data, bpc)


def last_len_of(nbytes, bpc):
    return nbytes - (nbytes - 1) // bpc * bpc if nbytes else 0


# ---- CPU ---------------------------------------------------------------------------

def test_tree_constants_match_the_kernel():
    text = open(os.path.join(REPO, "libhdfs3_amd", "csrc", "crc32c_kernels.h")).read()
    assert int(re.search(r"kComposeLaneWords = (\d+);", text).group(1)) == K
    assert int(re.search(r"kComposeThreads = (\d+);", text).group(1)) == THREADS
    assert "kComposeSpan = uint64_t(kComposeLaneWords) * kComposeThreads;" in text


@pytest.fixture(scope="module")
def host_data():
    return splitmix_bytes(64 * 1024 * 16 + 300, 0xC0C0)


@pytest.mark.parametrize("ctype", [CRC32C, CRC32])
@pytest.mark.parametrize("bpc", [7, 512, 4096, 65536])
def test_block_composite_of_held_words_is_the_crc_of_the_data(host_data, bpc, ctype):
    from libhdfs3_amd.engine import block_composite_crc_crcs

    for nbytes in (0, 1, bpc - 1, bpc, bpc + 1, 64 * 1024 * 16 + 300):
        data = host_data[:nbytes]
        got = block_composite_crc_crcs(chunk_words(data, bpc, ctype), bpc, last_len_of(nbytes, bpc), ctype)
        assert got == whole_crc(data, ctype), (nbytes, bpc, ctype)


def test_composite_does_not_depend_on_the_chunk_size(host_data):
    from libhdfs3_amd.engine import block_composite_crc_crcs

    nbytes = host_data.nbytes
    a = block_composite_crc_crcs(oracle_compute(host_data, 512), 512, last_len_of(nbytes, 512))
    b = block_composite_crc_crcs(oracle_compute(host_data, 4096), 4096, last_len_of(nbytes, 4096))
    assert a == b == oracle_crc(host_data)


@pytest.mark.parametrize("ctype", [CRC32C, CRC32])
def test_crc_compose_of_two_ranges(host_data, ctype):
    from libhdfs3_amd.engine import crc_compose

    for total, cut in ((0, 0), (1, 0), (1, 1), (1000, 1), (1000, 999), (70000, 4096), (host_data.nbytes, 512 * 1024)):
        a, b = host_data[:cut], host_data[cut:total]
        assert crc_compose(whole_crc(a, ctype), whole_crc(b, ctype), b.nbytes, ctype) == \
            whole_crc(host_data[:total], ctype), (total, cut)


@pytest.mark.parametrize("ctype", [CRC32C, CRC32])
def test_file_composite_is_the_crc_of_the_concatenation(ctype):
    from libhdfs3_amd.engine import file_checksum_composite_crc

    sizes = (8 << 20, 8 << 20, (3 << 20) + 1000)
    data = splitmix_bytes(sum(sizes), 0xF11E)
    blocks, off = [], 0
    for s in sizes:
        blocks.append(data[off:off + s])
        off += s
    got = file_checksum_composite_crc([whole_crc(b, ctype) for b in blocks], list(sizes), ctype)
    assert got == whole_crc(data, ctype)
    assert file_checksum_composite_crc([], [], ctype) == 0


def test_host_forms_reject_bad_arguments():
    import ctypes

    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import Hdfs3CrcError, block_composite_crc_crcs, crc_compose, file_checksum_composite_crc

    words = np.zeros(8, np.uint8)
    for call in (lambda: crc_compose(1, 2, 3, ctype=0),
                 lambda: crc_compose(1, 2, 3, ctype=3),
                 lambda: block_composite_crc_crcs(words, 512, 512, ctype=7),
                 lambda: block_composite_crc_crcs(words, 0, 1),
                 lambda: block_composite_crc_crcs(words, 512, 0),
                 lambda: block_composite_crc_crcs(words, 512, 513),
                 lambda: file_checksum_composite_crc([1], [1], ctype=0)):
        with pytest.raises(Hdfs3CrcError) as e:
            call()
        assert e.value.rc == -errno.EINVAL
    lib = _native.lib()
    out = ctypes.c_uint32(0)
    assert lib.hdfs3_crc_compose(2, 1, 2, 3, None) == -errno.EINVAL
    assert lib.hdfs3_block_composite_crc_crcs(2, None, 2, 512, 512, ctypes.byref(out)) == -errno.EINVAL
    assert lib.hdfs3_block_composite_crc_crcs(2, words.ctypes.data, 2, 512, 512, None) == -errno.EINVAL
    assert lib.hdfs3_file_checksum_composite_crc(2, None, None, 1, ctypes.byref(out)) == -errno.EINVAL
    # no words: last_len is not looked at, and the empty block is 0
    assert lib.hdfs3_block_composite_crc_crcs(2, None, 0, 512, 0, ctypes.byref(out)) == 0 and out.value == 0
    # the device forms check their arguments before any device work
    assert lib.hdfs3_block_composite_crc_dev(None, None, 0, 512, ctypes.byref(out)) == -errno.EINVAL
    assert lib.hdfs3_block_composite_crc_words_dev_async(None, None, 0, 512, 0, None) == -errno.EINVAL


# ---- GPU ---------------------------------------------------------------------------

# Word counts where the tree changes shape. The reduction runs over the n - 1 whole chunks (the last
# word joins in the final step), so every edge is taken in n - 1 and in n: a lane's run (K), a wave
# (64 K), a workgroup (SPAN: from there a second level), two workgroups, and a full second level
# (SPAN^2 = 2^20: from there a third level).
WORD_COUNTS = sorted({1, 2, K - 1, K, K + 1, K + 2, 64 * K - 1, 64 * K, 64 * K + 1, 64 * K + 2,
                      SPAN - 1, SPAN, SPAN + 1, SPAN + 2, 2 * SPAN, 2 * SPAN + 1, 2 * SPAN + 2,
                      SPAN * SPAN - 1, SPAN * SPAN, SPAN * SPAN + 1, SPAN * SPAN + 2, (1 << 20) + 1})
MAX_WORDS = max(WORD_COUNTS)


def read_word(ctx, dev, offset=0):
    return int(ctx.download(dev, 4, offset=offset).view("<u4")[0])


@pytest.fixture(scope="module")
def random_words(gpu_ctx):
    words = splitmix_bytes(4 * MAX_WORDS, 0x5EED5)
    return words, gpu_ctx.upload(words)


@pytest.mark.gpu
@pytest.mark.parametrize("ctype", [CRC32C, CRC32])
@pytest.mark.parametrize("bpc", [512, 4096, 7, 65536])
def test_gpu_words_form_matches_the_host_form(gpu_ctx, random_words, bpc, ctype):
    from libhdfs3_amd.engine import DeviceBuffer, block_composite_crc_crcs

    words, d_words = random_words
    cases = [(n, last) for n in WORD_COUNTS for last in (1, bpc - 1, bpc)]
    d_out = DeviceBuffer(4 * len(cases))
    gpu_ctx.memset(d_out, 0xA5, 4 * len(cases))
    gpu_ctx.set_checksum_type(ctype)
    try:
        for i, (n, last) in enumerate(cases):
            gpu_ctx.block_composite_crc_words_dev(d_words.ptr, n, bpc, last, d_out.ptr + 4 * i)
        got = gpu_ctx.download(d_out, 4 * len(cases)).view("<u4")
    finally:
        gpu_ctx.set_checksum_type(CRC32C)
    for i, (n, last) in enumerate(cases):
        assert int(got[i]) == block_composite_crc_crcs(words[:4 * n], bpc, last, ctype), (n, last, bpc, ctype)


@pytest.mark.gpu
def test_gpu_words_form_at_a_word_offset_and_empty(gpu_ctx, random_words):
    """Words that start anywhere on a 4-byte boundary (the tail of a stored array), no words at all,
    and pointers the call refuses."""
    from libhdfs3_amd.engine import DeviceBuffer, Hdfs3CrcError, block_composite_crc_crcs

    words, d_words = random_words
    d_out = DeviceBuffer(4)
    for first, n in ((1, SPAN + 5), (3, 2 * SPAN + 7), (SPAN - 1, 3)):
        gpu_ctx.block_composite_crc_words_dev(d_words.ptr + 4 * first, n, 512, 100, d_out.ptr)
        assert read_word(gpu_ctx, d_out) == block_composite_crc_crcs(words[4 * first:4 * (first + n)], 512, 100)
    gpu_ctx.memset(d_out, 0xFF, 4)
    gpu_ctx.block_composite_crc_words_dev(d_words.ptr, 0, 512, 0, d_out.ptr)
    assert read_word(gpu_ctx, d_out) == 0
    for args in ((d_words.ptr + 2, 4, 512, 512, d_out.ptr), (d_words.ptr, 4, 512, 0, d_out.ptr),
                 (d_words.ptr, 4, 512, 513, d_out.ptr), (d_words.ptr, 4, 0, 1, d_out.ptr),
                 (None, 4, 512, 512, d_out.ptr), (d_words.ptr, 4, 512, 512, None)):
        with pytest.raises(Hdfs3CrcError) as e:
            gpu_ctx.block_composite_crc_words_dev(*args)
        assert e.value.rc == -errno.EINVAL


@pytest.fixture(scope="module")
def block_data(gpu_ctx):
    data = splitmix_bytes((16 << 20) + 8, 0xB10C)
    return data, gpu_ctx.upload(data), {}


# 12288 = 3 x 4096 takes the pieces + combine compute at every length (8192 only from 256 MiB)
@pytest.mark.gpu
@pytest.mark.parametrize("bpc", [512, 2048, 4096, 8192, 12288])
def test_gpu_data_form_matches_the_oracle(gpu_ctx, block_data, bpc):
    data, d_data, want = block_data
    for nbytes in (1, 300, 64 * 1024 * 16 + 300, (16 << 20) + 8):
        if nbytes not in want:
            want[nbytes] = oracle_crc(data[:nbytes])
        assert gpu_ctx.block_composite_crc_dev(d_data.ptr, nbytes, bpc) == want[nbytes], (nbytes, bpc)
    assert gpu_ctx.block_composite_crc_dev(d_data.ptr, 0, bpc) == 0
    assert gpu_ctx.block_composite_crc_dev(None, 0, bpc) == 0


@pytest.mark.gpu
def test_gpu_data_form_crc32_and_unaligned_data(gpu_ctx, block_data):
    data, d_data, _ = block_data
    n = 64 * 1024 * 16 + 300
    gpu_ctx.set_checksum_type(CRC32)
    try:
        assert gpu_ctx.block_composite_crc_dev(d_data.ptr, n, 512) == oracle_crc32(data[:n])
    finally:
        gpu_ctx.set_checksum_type(CRC32C)
    # an odd start and an odd chunk size: the byte-exact compute kernel feeds the same reduction
    assert gpu_ctx.block_composite_crc_dev(d_data.ptr + 3, n, 512) == oracle_crc(data[3:3 + n])
    assert gpu_ctx.block_composite_crc_dev(d_data.ptr, 100000, 7) == oracle_crc(data[:100000])


@pytest.mark.gpu
def test_gpu_back_to_back_calls_reuse_the_scratch(block_data):
    """A fresh ctx: a small block, a larger one (both buffers grow), then smaller ones again."""
    from libhdfs3_amd.engine import CrcContext

    data, d_data, _ = block_data
    with CrcContext(0) as ctx:
        before = ctx.kernel_launches
        for nbytes, bpc in ((5000, 512), ((16 << 20) + 8, 512), (300, 512), ((8 << 20) + 1, 4096), (5000, 512)):
            assert ctx.block_composite_crc_dev(d_data.ptr, nbytes, bpc) == oracle_crc(data[:nbytes]), (nbytes, bpc)
        # every call: a compute launch and at least one reduction launch
        assert ctx.kernel_launches >= before + 10


@pytest.mark.gpu
def test_gpu_kernel_launches_count_every_level(random_words):
    from libhdfs3_amd.engine import CrcContext, DeviceBuffer

    _, d_words = random_words
    d_out = DeviceBuffer(4)
    with CrcContext(0) as ctx:
        for n, levels in ((1, 1), (SPAN + 1, 1), (SPAN + 2, 2), (SPAN * SPAN + 1, 2), (SPAN * SPAN + 2, 3)):
            before = ctx.kernel_launches
            ctx.block_composite_crc_words_dev(d_words.ptr, n, 512, 512, d_out.ptr)
            assert ctx.kernel_launches == before + levels, n
        ctx.synchronize()


@pytest.mark.gpu
def test_gpu_async_words_form_on_an_attached_stream(random_words):
    """The ctx runs on a stream it does not own (another ctx's); the copy back follows on that stream."""
    from libhdfs3_amd import _native
    from libhdfs3_amd.engine import CrcContext, DeviceBuffer, block_composite_crc_crcs

    words, d_words = random_words
    with CrcContext(0) as owner, CrcContext(0) as ctx:
        stream = _native.lib().hdfs3_crc_ctx_get_stream(owner.ctx)
        ctx.set_stream(stream)
        assert _native.lib().hdfs3_crc_ctx_get_stream(ctx.ctx) == stream
        d_out = DeviceBuffer(8)
        n1, n2 = 3 * SPAN + 17, SPAN * SPAN + 2
        ctx.block_composite_crc_words_dev(d_words.ptr, n1, 4096, 4000, d_out.ptr)
        ctx.block_composite_crc_words_dev(d_words.ptr, n2, 512, 77, d_out.ptr + 4)
        got = ctx.download(d_out, 8).view("<u4")
        assert int(got[0]) == block_composite_crc_crcs(words[:4 * n1], 4096, 4000)
        assert int(got[1]) == block_composite_crc_crcs(words[:4 * n2], 512, 77)
        ctx.set_stream(None)


@pytest.mark.gpu
def test_gpu_single_flipped_bit_changes_the_composite(gpu_ctx, random_words):
    from libhdfs3_amd.engine import DeviceBuffer, block_composite_crc_crcs

    words, _ = random_words
    n = 3 * SPAN + 5
    mine = words[:4 * n].copy()
    d = gpu_ctx.upload(mine)
    d_out = DeviceBuffer(4)
    gpu_ctx.block_composite_crc_words_dev(d.ptr, n, 512, 512, d_out.ptr)
    clean = read_word(gpu_ctx, d_out)
    seen = {clean}
    for index in (0, n // 2, n - 1):
        bad = mine.copy()
        bad[4 * index + 2] ^= 0x08
        gpu_ctx.upload(bad, d)
        gpu_ctx.block_composite_crc_words_dev(d.ptr, n, 512, 512, d_out.ptr)
        got = read_word(gpu_ctx, d_out)
        assert got != clean, index
        assert got == block_composite_crc_crcs(bad, 512, 512), index
        seen.add(got)
    assert len(seen) == 4
