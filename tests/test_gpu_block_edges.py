"""GPU parity of the contiguous-block calls at their small edges: hdfs3_crc32c_verify_dev,
_verify_dev_async(_ex), hdfs3_crc32c_compute_dev and _compute_dev_async_ex over one device block, at the
sizes where the launcher (launch_chunks, launch_wave3 with PITCH = false, launch_r3, launch_pieces) takes
another decision. Everything is compared with the oracle by exact equality: every first bad chunk under
both tail semantics, every computed word, and every byte of the device allocations that must not change.
A verify that skips a chunk passes every clean check, so the verifies here are driven by flips: one byte
in every chunk (sections a, e, f) or in every chunk the decision under test moves (b, d).

With len = 4096 * U + rem, each section sits on these decisions of the launcher:

  a. verify around the wave split: 256-thread workgroups planned at 2 rounds per wave, so 1 ... 8 units
     are one workgroup whose 4 waves take kq = U / 4 rounds and U % 4 of them one more, 9 units the first
     grid of two, 33 and 65 odd splits of larger grids; len % 4096 goes to slow_region, one chunk per
     thread of workgroup 0 (1 ... 8 threads at bpc 512); overlapped launches take the solo last step.
  b. verify at the switch points: the grid cap under 256-thread workgroups (2048 units on a 256-CU
     part), the switch to 512-thread workgroups above 4096 units and to 1024 above 16384, where kr goes
     from nwaves - 1 through 0 to 1 and kq steps by one. test_wave_split_table restates that arithmetic
     and pins it to the header's text; the GPU tests assert nothing about CU counts.
  c. compute at the same edges: always 1024 threads (32 units per workgroup, the cap at 8192 units),
     staged word runs at bpc <= 2048 and 64-word line stores at 4096, into word arrays that are 4-byte
     but not 16-byte aligned.
  d. chunks above 4096: bpc 8192 / 16384 / 65536 take the multi-round kernel (launch_r3, grid cap at
     4096 chunks of 8192), 12288 and 20480 pieces and a combine at every length, len < bpc the
     chunk-per-lane kernel; a remainder of 4096 is a whole round that is no chunk.
  e. below one unit (len < 4096 falls to the chunk-per-lane kernel even when aligned) and unaligned
     data or word pointers (launch_chunks' `aligned`), which must give the aligned run's keys and words.
  f. the second polynomial (HDFS3_CHECKSUM_TYPE_CRC32): the same kernels with the CRC-32 table and fold
     images, a and d again on a context of the test's own, pinned to zlib.crc32 over one chunk.

All data is a prefix of one splitmix stream and every reference word list is computed once per chunk size
(Ref); blocks are copied out of it, so a test's pokes never change the reference."""
import os
import zlib

import numpy as np
import pytest

from util import REPO, oracle_compute, oracle_compute_crc32, oracle_verify, splitmix_bytes

gpu = pytest.mark.gpu

CANARY = 0xC3    # around the data and the stored words of a verify
BLANK = 0xA5     # a compute's output allocation
PAD = 64         # canary bytes before and after
OUT_TAIL = 1024  # blank bytes after a compute's words (a staged run is up to 512 bytes)
RES_WORDS = 4096
BIG = 4096 * 16385 + 4095


class Ref:
    """One deterministic byte stream and its per-chunk words at every chunk size, computed once."""

    def __init__(self, compute, nbytes, seed):
        self.compute = compute
        self.data = splitmix_bytes(nbytes, seed)
        self.data.setflags(write=False)
        self._words = {}

    def words(self, bpc, n):
        """the words of data[:n]"""
        have = self._words.get(bpc)
        if have is None or have[0] < n:
            upto = min(self.data.size, max(1 << 20, 1 << (n - 1).bit_length()))
            have = self._words[bpc] = (upto, self.compute(self.data[:upto], bpc))
        full = n // bpc
        w = have[1][:4 * full]
        if n % bpc:
            w = np.concatenate([w, self.compute(self.data[full * bpc:n], bpc)])
        return w

    def first_bad(self, data, bpc, words):
        """(remote, local): the oracle's first bad chunk of the image as it stands, under both semantics"""
        if self.compute is oracle_compute:
            return oracle_verify(data, bpc, words, False), oracle_verify(data, bpc, words, True)
        ne = np.flatnonzero((self.compute(data, bpc).reshape(-1, 4) != words.reshape(-1, 4)).any(axis=1))
        whole = ne[ne < data.size // bpc]
        return (int(whole[0]) if whole.size else -1), (int(ne[0]) if ne.size else -1)


@pytest.fixture(scope="module")
def ref():
    return Ref(oracle_compute, BIG, 0xB10C)


@pytest.fixture(scope="module")
def ref32():
    return Ref(oracle_compute_crc32, 65536 * 33 + 65535, 0xB10C32)


@pytest.fixture(scope="module")
def res(gpu_ctx):
    from libhdfs3_amd.engine import DeviceBuffer

    buf = DeviceBuffer(8 * RES_WORDS)
    yield buf
    buf.free()


@pytest.fixture(scope="module")
def ctx32():
    from libhdfs3_amd.engine import CrcContext

    c = CrcContext(0)
    c.set_checksum_type(1)
    assert c.checksum_type == 1
    yield c
    c.close()


@pytest.fixture(scope="module")
def res32(ctx32):
    from libhdfs3_amd.engine import DeviceBuffer

    buf = DeviceBuffer(8 * RES_WORDS)
    yield buf
    buf.free()


class Block:
    """data[:n] and its words, each between canaries in a host image and in `copies` device allocations;
    the data starts PAD + data_off bytes into its allocation (16-byte aligned at data_off 0), the words
    PAD + word_off into theirs. Pokes go to the image and to the last copy; copy 0 of two stays clean."""

    def __init__(self, ctx, ref, n, bpc, copies=1, data_off=0, word_off=0):
        self.ctx, self.ref, self.n, self.bpc = ctx, ref, n, bpc
        self.nchunks = -(-n // bpc)
        self.d0, self.w0 = PAD + data_off, PAD + word_off
        self.dimg = np.full(self.d0 + n + PAD, CANARY, np.uint8)
        self.dimg[self.d0:self.d0 + n] = ref.data[:n]
        self.wimg = np.full(self.w0 + 4 * self.nchunks + PAD, CANARY, np.uint8)
        self.wimg[self.w0:self.w0 + 4 * self.nchunks] = ref.words(bpc, n)
        self.data = self.dimg[self.d0:self.d0 + n]
        self.words = self.wimg[self.w0:self.w0 + 4 * self.nchunks]
        self.dev = [(ctx.upload(self.dimg), ctx.upload(self.wimg)) for _ in range(copies)]

    def poke(self, kind, off, mask):
        """flip bits of one byte of the data ('d') or of the words ('w'), in the image and on the device:
        one byte travels"""
        img, dev, base = (self.dimg, self.dev[-1][0], self.d0) if kind == "d" else (self.wimg, self.dev[-1][1], self.w0)
        img[base + off] ^= mask
        self.ctx.upload(img[base + off:base + off + 1], dev, offset=base + off)

    def want(self):
        return self.ref.first_bad(self.data, self.bpc, self.words)

    def ptrs(self, copy):
        d, w = self.dev[copy]
        return d.ptr + self.d0, w.ptr + self.w0

    def close_unchanged(self):
        """every copy on the device is byte for byte what was uploaded (the pokes were taken back)"""
        want_w = self.ref.words(self.bpc, self.n)
        for d, w in self.dev:
            for got, base, want in ((self.ctx.download(d, d.nbytes), self.d0, self.ref.data[:self.n]),
                                    (self.ctx.download(w, w.nbytes), self.w0, want_w)):
                assert np.array_equal(got[base:base + want.size], want)
                assert (got[:base] == CANARY).all() and (got[base + want.size:] == CANARY).all()
            d.free()
            w.free()
        assert np.array_equal(self.data, self.ref.data[:self.n]) and np.array_equal(self.words, want_w)


class Runs:
    """Verify launches, each into its own result word of `res`; the words are read back once."""

    def __init__(self, ctx, res):
        self.ctx, self.res = ctx, res
        self._reset()

    def _reset(self):
        self.ctx.memset(self.res, 0, 8 * RES_WORDS)
        self.want, self.note, self.got = [], [], []

    def room(self, launches):
        """between chains only: a memset of the result words must not sit before an overlapped launch"""
        if len(self.want) + launches > RES_WORDS:
            self.finish()
            self._reset()

    def verify(self, blk, copy, local, want, overlap=False, note=None):
        assert len(self.want) < RES_WORDS
        d, w = blk.ptrs(copy)
        self.ctx.verify_dev_async(d, blk.n, blk.bpc, w, self.res.ptr + 8 * len(self.want), bool(local),
                                  overlap_previous=overlap)
        self.want.append(want)
        self.note.append((note, "local" if local else "remote", "overlapped" if overlap else "barriered"))

    def finish(self):
        self.ctx.synchronize()
        words = self.ctx.download(self.res, 8 * len(self.want)).view(np.uint64).tolist()
        got = [self.ctx.decode_result(int(w)) for w in words]
        bad = [(n, g, w) for n, g, w in zip(self.note, got, self.want) if g != w]
        assert not bad, f"{len(bad)} of {len(got)} verifies differ from the oracle; (launch, got, want): {bad[:6]}"
        self.got += got
        return self.got


def run_flips(runs, blk, flips, chain):
    """flips = [([(kind, offset), ...], chunk)]: the pokes of one case and the chunk a local verify must
    report. Each case is verified barriered under both semantics against the oracle over the image as it
    stands; with `chain` (two copies) also as the second and the third launch of an overlapped chain whose
    first launch is barriered, next to the clean copy in both orders."""
    tail = blk.n // blk.bpc if blk.n % blk.bpc else -1
    for i, (pokes, chunk) in enumerate(flips):
        runs.room(14)
        for kind, off in pokes:
            blk.poke(kind, off, 1 << (i % 8))
        want = blk.want()
        # a flipped byte is seen wherever it sits, but for a short tail chunk under remote semantics
        assert want == (-1 if chunk == tail else chunk, chunk), (pokes, chunk, want)
        for local in (0, 1):
            runs.verify(blk, -1, local, want[local], note=pokes)
            if chain:
                for order in ((0, -1, 0), (-1, 0, -1)):
                    for k, copy in enumerate(order):
                        runs.verify(blk, copy, local, want[local] if copy else -1, overlap=k > 0, note=pokes)
        for kind, off in pokes:
            blk.poke(kind, off, 1 << (i % 8))


def data_flip(n, bpc, c, salt=0):
    """a byte of chunk c, at a position that moves through the chunk"""
    return "d", c * bpc + ((c + salt) * 523 + 5) % min(bpc, n - c * bpc)


def every_chunk(n, bpc, word_units=9):
    """one byte in every chunk, then one byte of the stored word of every chunk of the first units"""
    nchunks = -(-n // bpc)
    flips = [([data_flip(n, bpc, c)], c) for c in range(nchunks)]
    flips += [([("w", 4 * c + c % 4)], c) for c in range(min(nchunks, -(-word_units * 4096 // bpc)))]
    return flips


def verify_case(ctx, res, ref, n, bpc, flips, chain, data_off=0, word_off=0):
    """clean under both semantics through the synchronous call, the flips, and nothing changed; the keys"""
    blk = Block(ctx, ref, n, bpc, 2 if chain else 1, data_off, word_off)
    assert blk.want() == (-1, -1)
    d, w = blk.ptrs(-1)
    for local in (False, True):
        assert ctx.verify_dev(d, n, bpc, w, local) == -1, local
    runs = Runs(ctx, res)
    run_flips(runs, blk, flips, chain)
    got = runs.finish()
    blk.close_unchanged()
    return got


def compute_case(ctx, ref, n, bpc, word_offs, overlap=False, data_off=0):
    """compute into blank allocations, the words word_off bytes in: every word the oracle's, every other
    byte still blank, the data and its canaries unchanged. overlap: a second compute of the same data into
    another array, overlapped with the first. Returns the words."""
    from libhdfs3_amd.engine import DeviceBuffer

    want = ref.words(bpc, n)
    d0 = PAD + data_off
    d = DeviceBuffer(d0 + n + PAD)
    ctx.memset(d, CANARY, d.nbytes)
    ctx.upload(ref.data[:n], d, offset=d0)
    for wo in word_offs:
        outs = [DeviceBuffer(wo + want.size + OUT_TAIL) for _ in range(2 if overlap else 1)]
        for o in outs:
            ctx.memset(o, BLANK, o.nbytes)
        ctx.compute_dev(d.ptr + d0, n, bpc, outs[0].ptr + wo)
        if overlap:
            ctx.compute_dev(d.ptr + d0, n, bpc, outs[1].ptr + wo, overlap_previous=True)
        for k, o in enumerate(outs):
            got = ctx.download(o, o.nbytes)
            o.free()
            bad = np.flatnonzero(got[wo:wo + want.size] != want)
            assert bad.size == 0, f"word offset {wo}, array {k}: {bad.size} word bytes differ, the first in chunk " \
                                  f"{int(bad[0]) // 4} of {want.size // 4}"
            assert (got[:wo] == BLANK).all(), (wo, k)
            after = np.flatnonzero(got[wo + want.size:] != BLANK)
            assert after.size == 0, f"word offset {wo}, array {k}: byte {int(after[0])} past the words was written"
    got = ctx.download(d, d.nbytes)
    d.free()
    assert np.array_equal(got[d0:d0 + n], ref.data[:n])
    assert (got[:d0] == CANARY).all() and (got[d0 + n:] == CANARY).all()
    return want


def remainders(bpc):
    """the shapes of len % 4096 at a chunk size up to 4096"""
    out = [("0", 0), ("short", 100)]
    if bpc < 4096:
        out.append(("whole", 4096 - bpc))
    out.append(("whole+short", 4095))
    if bpc == 512:  # with the above, a slow region of every count from 1 to 8 threads
        out += [(f"{k}+1", 512 * k + 1) for k in range(1, 7)]
    return out


SPLIT_UNITS = list(range(1, 21)) + [31, 32, 33, 63, 64, 65]
ROUND_BPCS = [512, 1024, 2048, 4096]


def case_ids(cases):
    return [f"bpc{b}-U{u}-{name}" for b, u, (name, _) in cases]


# ---- a. verify around the wave split ------------------------------------------------------------------
A_CASES = [(bpc, U, r) for bpc in ROUND_BPCS for U in SPLIT_UNITS for r in remainders(bpc)]


@gpu
@pytest.mark.parametrize("bpc,U,rem", A_CASES, ids=case_ids(A_CASES))
def test_verify_around_the_wave_split(gpu_ctx, res, ref, bpc, U, rem):
    n = 4096 * U + rem[1]
    verify_case(gpu_ctx, res, ref, n, bpc, every_chunk(n, bpc), chain=U in (1, 8, 9, 33))


# ---- b. verify at the launcher's switch points --------------------------------------------------------
def wave_split(units, verify, grid_cap=256):
    """launch_wave3's plan for a contiguous block of `units` whole rounds: (threads per workgroup, grid,
    waves, kq, kr); wave w takes kq rounds, plus one when w < kr."""
    tpb = 1024
    if verify:  # compute over a contiguous block keeps 1024 threads
        tpb = 256 if units <= 4096 else 512 if units <= 16384 else 1024
    rpw = 2  # rounds per wave planned
    wpb = tpb // 64
    need = (units + rpw * wpb - 1) // (rpw * wpb)
    grid = max(1, min(need, grid_cap))
    nwaves = grid * wpb
    return tpb, grid, nwaves, units // nwaves, units % nwaves


def test_wave_split_table():
    """The unit counts of sections a, b and c against the split arithmetic of launch_wave3, restated in
    wave_split above, and that arithmetic against the header's own text: a change there fails here, so
    the tables cannot drift from the launcher silently."""
    def squash(s):
        return "".join(s.split())

    csrc = os.path.join(REPO, "libhdfs3_amd", "csrc")
    with open(os.path.join(csrc, "crc32c_wave.h")) as f:
        wave_h = squash(f.read())
    with open(os.path.join(csrc, "ctx.h")) as f:
        ctx_h = squash(f.read())
    for line in [
        "const uint64_t units = PITCH ? (a.npk - 1) * a.geom.upp + a.geom.lunits : a.len / kRoundBytes;",
        "const uint64_t rpw = (LAB & kLabOneRound) != 0 && units <= 4096 ? 1 : 2;",
        "const uint64_t need = (units + rpw * (TPB / 64) - 1) / (rpw * (TPB / 64));",
        "int grid = int(need < uint64_t(grid_cap) ? need : uint64_t(grid_cap));",
        "if (grid < 1) grid = 1;",
        "const uint64_t nwaves = uint64_t(grid) * (TPB / 64);",
        "b.kq = uint32_t(units / nwaves);",
        "b.kr = uint32_t(units % nwaves);",
        "if constexpr ((V || PITCH) && TPB == 1024 && (LAB & kLabWg1024) == 0) {",
        "if (units <= 4096) return launch_wave3<BPC, V, PITCH, SOLO, LAB, 256, true>(a, tab, fold, grid_cap, s);",
        "if (units <= 16384) return launch_wave3<BPC, V, PITCH, SOLO, LAB, 512>(a, tab, fold, grid_cap, s);",
        "const uint32_t K = a.kq + (wave < a.kr ? 1u : 0u);",
        "template <int BPC, bool V, bool PITCH, bool SOLO, int LAB = 0, int TPB = kBlockThreads, bool SMALL = false>",
    ]:
        assert squash(line) in wave_h, line
    assert squash("int grid_cap = 256;") in ctx_h
    with open(os.path.join(csrc, "crc32c_kernels.h")) as f:
        assert squash("constexpr int kBlockThreads = 1024;") in squash(f.read())

    # a: one workgroup of 4 waves up to 8 units, then the first grid of two
    for u in range(1, 9):
        assert wave_split(u, True) == (256, 1, 4, u // 4, u % 4)
    assert wave_split(9, True) == (256, 2, 8, 1, 1)
    assert wave_split(33, True) == (256, 5, 20, 1, 13)
    # b: (units, threads, grid, kq, kr) either side of the grid cap and of the two workgroup sizes
    table = [(2047, 256, 256, 1, 1023), (2048, 256, 256, 2, 0), (2049, 256, 256, 2, 1),
             (4095, 256, 256, 3, 1023), (4096, 256, 256, 4, 0), (4097, 512, 256, 2, 1),
             (16383, 512, 256, 7, 2047), (16384, 512, 256, 8, 0), (16385, 1024, 256, 4, 1)]
    assert [u for u, *_ in table] == SWITCH_UNITS
    for u, tpb, grid, kq, kr in table:
        assert wave_split(u, True) == (tpb, grid, grid * tpb // 64, kq, kr), u
    for lo, mid, hi in (table[0:3], table[3:6], table[6:9]):
        waves = lo[2] * lo[1] // 64
        assert lo[4] == waves - 1 and mid[4] == 0 and hi[4] == 1  # kr: every wave but one, none, one
        assert mid[3] == lo[3] + 1                                  # kq steps by one at the full split
    assert wave_split(2048, True)[1] == 256 and wave_split(2040, True)[1] == 255  # the cap is reached at 2048
    # c: compute keeps 1024 threads: one workgroup up to 32 units, the cap at 8192
    for u, grid, kq, kr in [(1, 1, 0, 1), (16, 1, 1, 0), (17, 1, 1, 1), (32, 1, 2, 0), (33, 2, 1, 1),
                            (8191, 256, 1, 4095), (8192, 256, 2, 0), (8193, 256, 2, 1)]:
        assert wave_split(u, False) == (1024, grid, 16 * grid, kq, kr), u


SWITCH_UNITS = [2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385]
B_CASES = [(bpc, U, r) for bpc in (512, 4096) for U in SWITCH_UNITS for r in (("0", 0), ("whole+short", 4095))] + \
          [(2048, U, r) for U in (4097, 16385) for r in (("0", 0), ("whole+short", 4095))]


@gpu
@pytest.mark.parametrize("bpc,U,rem", B_CASES, ids=case_ids(B_CASES))
def test_verify_at_the_switch_points(gpu_ctx, res, ref, bpc, U, rem):
    """With W waves in the grid of a 256-CU part: a flip in unit 0, in unit W - 1, in unit W (wave 0's
    second round), in the last whole unit, in each slow chunk and in the short tail, barriered and
    overlapped; then two flips at once, of which the earlier chunk must be reported."""
    n = 4096 * U + rem[1]
    cpu = 4096 // bpc
    nchunks = -(-n // bpc)
    W = wave_split(U, True)[2]

    def in_unit(u):
        return u * cpu + (u * 3 + 1) % cpu

    def flip(c):
        return data_flip(n, bpc, c, salt=U)

    units = [u for u in dict.fromkeys([0, W - 1, W, U - 1]) if 0 <= u < U]
    singles = [in_unit(u) for u in units] + list(range(U * cpu, nchunks))
    flips = [([flip(c)], c) for c in singles]
    flips.append(([flip(in_unit(U - 1)), flip(in_unit(1))], in_unit(1)))
    if rem[1]:
        flips.append(([flip(U * cpu), flip(in_unit(0))], in_unit(0)))          # the slow region and unit 0
        flips.append(([flip(nchunks - 1), flip(in_unit(U - 1))], in_unit(U - 1)))  # the short tail and the last unit
    verify_case(gpu_ctx, res, ref, n, bpc, flips, chain=True)


# ---- c. compute at the same edges ---------------------------------------------------------------------
WORD_OFFS = [64, 64 + 4, 64 + 8, 64 + 12]
C_CASES = [(bpc, U, r) for bpc in ROUND_BPCS for U in SPLIT_UNITS + [8191, 8192, 8193] for r in remainders(bpc)]


@gpu
@pytest.mark.parametrize("bpc,U,rem", C_CASES, ids=case_ids(C_CASES))
def test_compute_at_the_edges(gpu_ctx, ref, bpc, U, rem):
    compute_case(gpu_ctx, ref, 4096 * U + rem[1], bpc, WORD_OFFS, overlap=U in (1, 16, 17, 32, 33, 8193))


# ---- d. chunks above 4096 on the contiguous route -----------------------------------------------------
def big_chunk_cases(bpcs):
    out = []
    for bpc in bpcs:
        # N = 0: only a short chunk, the chunk-per-lane fallback
        for N in [0] + list(range(1, 19)) + [33] + ([4095, 4096, 4097] if bpc == 8192 else []):
            out += [(bpc, N, rem) for rem in (0, 100, 4096, bpc - 1) if N or rem]
    return out


def big_chunk_flips(n, bpc, N):
    """one byte in every 4096-byte piece of the first, a middle and the last whole chunk, and one in the
    remainder: a chunk whose second or later round is ignored shows up"""
    R = bpc // 4096
    flips = [([("d", c * bpc + 4096 * i + ((c * R + i) * 523 + 5) % 4096)], c)
             for c in dict.fromkeys([0, N // 2, N - 1]) if 0 <= c < N for i in range(R)]
    if n % bpc:
        flips.append(([("d", N * bpc + (n % bpc) // 2)], N))
    return flips


def big_chunk_case(ctx, res, ref, bpc, N, rem):
    n = bpc * N + rem
    verify_case(ctx, res, ref, n, bpc, big_chunk_flips(n, bpc, N), chain=False)
    return compute_case(ctx, ref, n, bpc, WORD_OFFS)


D_CASES = big_chunk_cases([8192, 16384, 65536, 12288, 20480])


@gpu
@pytest.mark.parametrize("bpc,N,rem", D_CASES, ids=[f"bpc{b}-N{n}-rem{r}" for b, n, r in D_CASES])
def test_chunks_above_4096(gpu_ctx, res, ref, bpc, N, rem):
    big_chunk_case(gpu_ctx, res, ref, bpc, N, rem)


# ---- e. below one unit, and unaligned pointers --------------------------------------------------------
E_CASES = [(bpc, n) for bpc in ROUND_BPCS for n in dict.fromkeys([1, bpc - 1, bpc, bpc + 1, 4095])]


@gpu
@pytest.mark.parametrize("bpc,n", E_CASES, ids=[f"bpc{b}-len{n}" for b, n in E_CASES])
def test_below_one_unit(gpu_ctx, res, ref, bpc, n):
    verify_case(gpu_ctx, res, ref, n, bpc, every_chunk(n, bpc), chain=False)
    compute_case(gpu_ctx, ref, n, bpc, WORD_OFFS)


@gpu
@pytest.mark.parametrize("bpc", [512, 4096, 8192])
@pytest.mark.parametrize("U", [1, 9, 33])
def test_unaligned_pointers_match_the_aligned_run(gpu_ctx, res, ref, bpc, U):
    """The data pointer at +1 and +8 from a 16-byte boundary and, separately, the word pointer at +1 and
    +2 from a 4-byte boundary: the keys of a flip in every chunk and the computed words are those of the
    aligned run (and the oracle's), inside intact canaries."""
    n = 4096 * U + 4095
    flips = every_chunk(n, bpc)
    keys = verify_case(gpu_ctx, res, ref, n, bpc, flips, chain=False)
    words = compute_case(gpu_ctx, ref, n, bpc, [64])
    for data_off, word_off in [(1, 0), (8, 0), (0, 1), (0, 2)]:
        assert verify_case(gpu_ctx, res, ref, n, bpc, flips, False, data_off, word_off) == keys, (data_off, word_off)
        assert np.array_equal(compute_case(gpu_ctx, ref, n, bpc, [64 + word_off], data_off=data_off), words)


# ---- f. the second polynomial -------------------------------------------------------------------------
def zlib_pin(ctx32, ref32, n, bpc):
    """chunk 0 of the block, computed on the GPU, against zlib.crc32: independent of the oracle"""
    from libhdfs3_amd.engine import DeviceBuffer

    d = ctx32.upload(ref32.data[:n])
    out = DeviceBuffer(4 * (-(-n // bpc)))
    ctx32.compute_dev(d.ptr, n, bpc, out.ptr)
    got = ctx32.download(out, out.nbytes)
    d.free()
    out.free()
    assert int(got[:4].view(">u4")[0]) == zlib.crc32(ref32.data[:min(n, bpc)].tobytes())
    assert np.array_equal(got, ref32.words(bpc, n))


F_SPLIT_CASES = [(bpc, U, r) for bpc in (512, 4096) for U in (1, 8, 9, 33) for r in remainders(bpc)]


@gpu
@pytest.mark.parametrize("bpc,U,rem", F_SPLIT_CASES, ids=case_ids(F_SPLIT_CASES))
def test_crc32_verify_around_the_wave_split(ctx32, res32, ref32, bpc, U, rem):
    n = 4096 * U + rem[1]
    verify_case(ctx32, res32, ref32, n, bpc, every_chunk(n, bpc), chain=True)
    zlib_pin(ctx32, ref32, n, bpc)


F_BIG_CASES = big_chunk_cases([16384, 12288])


@gpu
@pytest.mark.parametrize("bpc,N,rem", F_BIG_CASES, ids=[f"bpc{b}-N{n}-rem{r}" for b, n, r in F_BIG_CASES])
def test_crc32_chunks_above_4096(ctx32, res32, ref32, bpc, N, rem):
    want = big_chunk_case(ctx32, res32, ref32, bpc, N, rem)
    # the block's first chunk (a short one at N = 0) against zlib: independent of the oracle
    assert int(want[:4].view(">u4")[0]) == zlib.crc32(ref32.data[:bpc if N else rem].tobytes())
