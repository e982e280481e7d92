// Device code of the gfx950 CRC32C kernels and their launch templates, shared by the
// production translation unit (crc32c_kernels.hip) and the A/B experiments
// (crc32c_experiments.hip): the table image and its lookups, the chunk-per-lane, multi-round and packet
// kernels, the pieces of the round kernel (crc32c_wave.h). No lab code (clock stamps: crc32c_lab.h; read
// ceilings: crc32c_experiments.hip): it reads the same in both builds. Internal; not installed.
#pragma once
// gfx950 (CDNA4) CRC32C kernels for libhdfs3's per-chunk checksum path.
//
// Replaces the per-chunk reset/update/getValue loops of
//   RemoteBlockReader::verifyChecksum   (src/client/RemoteBlockReader.cpp:306-326)
//   LocalBlockReader::readAndVerify     (src/client/LocalBlockReader.cpp:138-163)
//   OutputStreamImpl::appendInternal    (src/client/OutputStreamImpl.cpp:298-359)
// with one launch over a whole batch of chunks.
//
// Mapping: one chunk per lane (chunks are independent, so no cross-lane fold is
// needed). Each lane walks its chunk in 16-byte loads and runs slice-by-4 table
// CRC: per 32-bit word, 4 LDS lookups. LDS is the co-bottleneck with HBM: a
// lookup per payload byte is 6-7e12 lookups/s at the HBM roofline, so the four
// 1 KiB slice tables are REPLICATED 32x across the LDS banks and lane l always
// reads copy l%32: every ds_read_b32 half-wave hits 32 distinct banks, i.e. it is
// conflict-free whatever the data. The image is 128 KiB, so one 1024-thread
// workgroup owns a CU.
//
// LDS image (byte address):  rowset*64K + entry*256 + half*128 + copy*4
//   slice 0 -> rowset 0 half 0,  slice 1 -> rowset 0 half 1,
//   slice 2 -> rowset 1 half 0,  slice 3 -> rowset 1 half 1.
// A 256-byte entry stride puts the table index in address byte 1, so ONE
// v_perm_b32 builds a lookup address from the CRC state and a per-lane base
// (bytes 0 and 2), and v_bitop3_b32 folds three lookups per instruction: a
// 32-bit word costs 4 v_perm + 2 v_bitop3 + 4 ds_read_b32.
#include <hip/hip_ext.h>

#include <type_traits>

#include "crc32c_kernels.h"
#include "crc32c_tables.h"

namespace hdfs3crc {
namespace {

constexpr int kCopies = 32;                                   // one per ds_read_b32 bank
constexpr int kLdsBytes = 128 * 1024;                         // 2 rowsets x 256 entries x 256 B
constexpr int kLdsSlots = kLdsBytes / 16;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Fill the replicated image from the 4 KiB global table image (slice-major,
// 256 words per slice). Consecutive lanes write consecutive 16-byte slots, so
// each ds_write_b128 lane group stores 128 contiguous bytes (conflict-free).
// Split in two so the caller can put its first data loads between the table
// fetch and the LDS stores (vmcnt is in-order: loads issued after the table
// words do not have to land before the stores).
constexpr int kFillPerThread = kLdsSlots / kBlockThreads;

__device__ __forceinline__ void fetch_tables(uint32_t (&v)[kFillPerThread],
                                             const uint32_t *__restrict__ g_tab) {
#pragma unroll
    for (int i = 0; i < kFillPerThread; ++i) {
        const int s = i * kBlockThreads + threadIdx.x;
        const int rowset = s >> 12, entry = (s >> 4) & 255, half = (s >> 3) & 1;
        v[i] = g_tab[(rowset * 2 + half) * kTableEntries + entry];
    }
}

__device__ __forceinline__ void store_tables(uint32_t *lds, const uint32_t (&v)[kFillPerThread]) {
    u32x4 *l4 = reinterpret_cast<u32x4 *>(lds);
#pragma unroll
    for (int i = 0; i < kFillPerThread; ++i) l4[i * kBlockThreads + threadIdx.x] = u32x4{v[i], v[i], v[i], v[i]};
}

__device__ __forceinline__ void fill_tables(uint32_t *lds, const uint32_t *__restrict__ g_tab) {
    uint32_t v[kFillPerThread];
    fetch_tables(v, g_tab);
    store_tables(lds, v);
}

// LDS writes visible to the whole workgroup. Written as asm so the compiler does
// not drain the data loads already in flight (a __syncthreads() would add vmcnt(0)).
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

struct Lut {
    const uint8_t *lds;
    uint32_t base[4];  // per-slice lane base: rowset<<16 | half<<7 | lane*4

    __device__ __forceinline__ explicit Lut(const uint32_t *l) : lds(reinterpret_cast<const uint8_t *>(l)) {
        const uint32_t lane4 = (threadIdx.x & (kCopies - 1)) * 4;
        base[0] = lane4;
        base[1] = lane4 | 0x80u;
        base[2] = lane4 | 0x10000u;
        base[3] = lane4 | 0x10080u;
    }
    // T[slice][byte k of x]: address = {0, base.byte2, x.byte k, base.byte0}.
    template <int K>
    __device__ __forceinline__ uint32_t at(int slice, uint32_t x) const {
        const uint32_t addr = __builtin_amdgcn_perm(x, base[slice], 0x0C020000u | ((4u + K) << 8));
        return *reinterpret_cast<const uint32_t *>(lds + addr);
    }
    // x = state ^ word; returns the state after the word, pre-xored with `next`.
    __device__ __forceinline__ uint32_t word(uint32_t x, uint32_t next) const {
        return xor3(xor3(at<0>(3, x), at<1>(2, x), at<2>(1, x)), at<3>(0, x), next);
    }
    // One byte (SWCrc32c.cpp:102): crc = T0[(crc ^ b) & 0xFF] ^ (crc >> 8).
    __device__ __forceinline__ uint32_t byte(uint32_t c, uint32_t b) const {
        return at<0>(0, c ^ b) ^ (c >> 8);
    }
    // Plain-state helpers for the irregular paths.
    __device__ __forceinline__ uint32_t word_state(uint32_t c, uint32_t w) const { return word(c ^ w, 0); }
    __device__ __forceinline__ uint32_t vec_state(uint32_t c, u32x4 v) const {
        uint32_t x = c ^ v.x;
        x = word(x, v.y);
        x = word(x, v.z);
        x = word(x, v.w);
        return word(x, 0);
    }
};

// Default cache policy: measured 2.4x faster than nontemporal (`nt`) loads for the
// chunk-per-lane pattern and no slower for coalesced rounds (tools/sweep.py).
__device__ __forceinline__ u32x4 ld16(const uint8_t *p) {
    return *reinterpret_cast<const u32x4 *>(p);
}

// Arbitrary pointer/length run, alignment dispatched per call (packet arenas put
// data at odd offsets; the short tail chunk of a block). `n` bytes from `p`.
__device__ uint32_t crc_run_any(const Lut &t, uint32_t c, const uint8_t *p, uint32_t n) {
    // bytes up to 4-byte alignment
    while (n && (reinterpret_cast<uintptr_t>(p) & 3u)) {
        c = t.byte(c, *p++);
        --n;
    }
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        for (; n >= 16; n -= 16, p += 16) c = t.vec_state(c, ld16(p));
    }
    for (; n >= 4; n -= 4, p += 4) c = t.word_state(c, *reinterpret_cast<const uint32_t *>(p));
    for (; n; --n) c = t.byte(c, *p++);
    return c;
}

// crc_run_any for a 16-byte aligned run: 128-byte lines whose 8 loads are issued
// together, then the remaining 16-byte pieces (again issued together), then words and
// bytes. One load latency per line instead of one per 16 bytes: the segmented kernel's
// slow pass runs it on one lane per chunk while the rest of the wave waits.
__device__ uint32_t crc_run_lines(const Lut &t, uint32_t c, const uint8_t *p, uint32_t n) {
    for (; n >= 128; n -= 128, p += 128) {
        u32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ld16(p + 16 * i);
#pragma unroll
        for (int i = 0; i < 8; ++i) c = t.vec_state(c, v[i]);
    }
    const uint32_t k = n / 16;
    u32x4 v[7];
#pragma unroll
    for (int i = 0; i < 7; ++i)
        if (uint32_t(i) < k) v[i] = ld16(p + 16 * i);
#pragma unroll
    for (int i = 0; i < 7; ++i)
        if (uint32_t(i) < k) c = t.vec_state(c, v[i]);
    p += 16 * k;
    n -= 16 * k;
    for (; n >= 4; n -= 4, p += 4) c = t.word_state(c, *reinterpret_cast<const uint32_t *>(p));
    for (; n; --n) c = t.byte(c, *p++);
    return c;
}

__device__ __forceinline__ uint32_t load_be32(const uint8_t *p, bool aligned4) {
    if (aligned4) return __builtin_bswap32(*reinterpret_cast<const uint32_t *>(p));
    return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3];
}
__device__ __forceinline__ void store_be32(uint8_t *p, uint32_t v, bool aligned4) {
    if (aligned4) {
        *reinterpret_cast<uint32_t *>(p) = __builtin_bswap32(v);
        return;
    }
    p[0] = uint8_t(v >> 24); p[1] = uint8_t(v >> 16); p[2] = uint8_t(v >> 8); p[3] = uint8_t(v);
}

// Chunk-per-lane kernel (crc_run_any): run-time bpc, any alignment, short blocks, a launch's short last chunk
template <bool VERIFY>
__global__ __launch_bounds__(kBlockThreads) void crc32c_chunks_kernel(ChunkLaunch a, const uint32_t *__restrict__ g_tab) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsBytes / 4];
    const uint32_t bpc = a.bpc;
    const uint64_t nfull = a.len / bpc;
    const uint64_t stride = uint64_t(gridDim.x) * kBlockThreads;
    uint64_t chunk = uint64_t(blockIdx.x) * kBlockThreads + threadIdx.x;
    const bool crc_al4 = (reinterpret_cast<uintptr_t>(VERIFY ? a.crc_be : a.out_be) & 3u) == 0;

    fill_tables(lds, g_tab);
    lds_barrier();
    const Lut t(lds);

    for (; chunk < nfull; chunk += stride) {
        const uint8_t *p = a.data + chunk * bpc;
        // Stored word requested first: it is older than the chunk's loads, so
        // waiting for it never drains them (vmcnt is in-order).
        uint32_t want = 0;
        if constexpr (VERIFY) want = load_be32(a.crc_be + 4 * chunk, crc_al4);
        const uint32_t c = ~crc_run_any(t, 0xFFFFFFFFu, p, bpc);
        if constexpr (VERIFY) {
            if (want != c)
                atomicMax(a.result, ~(unsigned long long)(a.chunk_base + chunk));
        } else {
            store_be32(a.out_be + 4 * chunk, c, crc_al4);
        }
    }
    // The lane whose stride sequence lands exactly on nfull owns the short tail chunk.
    const uint32_t tail = uint32_t(a.len - nfull * bpc);
    if (tail && chunk == nfull) {
        const uint32_t c = ~crc_run_any(t, 0xFFFFFFFFu, a.data + nfull * bpc, tail);
        if constexpr (VERIFY) {
            if (a.check_short_tail && load_be32(a.crc_be + 4 * nfull, crc_al4) != c)
                atomicMax(a.result, ~(unsigned long long)(a.chunk_base + nfull));
        } else {
            store_be32(a.out_be + 4 * nfull, c, crc_al4);
        }
    }
}

// ---- round kernel (the fast path) -------------------------------------------
//
// Work is cut into ROUNDS of 4 KiB of contiguous data, one round per wave at a
// time. A round is fetched with 4 perfectly coalesced global_load_dwordx4 (1 KiB
// each) and then regrouped in registers so that lane l owns the 64 contiguous bytes
// [64l, 64l+64) of the round:
//   instruction t gives lane (row r = l/16, c = l%16) the 16-byte piece 64t+4c+r;
//   lane (row s, c) needs pieces 64s+4c+q in register q  =>  a 4x4 transpose between
//   the wave's four 16-lane rows and the four load registers, done by one
//   v_permlane32_swap stage (rows {0,1} <-> {2,3}) and one v_permlane16_swap stage
//   (odd <-> even rows): 16 swaps per round, no LDS traffic.
// Each lane then runs slice-by-4 over its 16 words. A chunk of bpc <= 4096 bytes is
// G = bpc/64 consecutive lanes; lane j of a chunk advances its partial state over
// the (G-1-j)*64 bytes that follow its segment with a lane-specific 32x32 GF(2)
// matrix held in VGPRs (crc(A||B) = shift_|B|(crc(A)) ^ crc0(B)), the G states are
// xor-reduced with DPP / permlane swaps, and lane j == 0 finishes the chunk.
// For bpc a multiple of 4096 a wave walks the chunk's rounds in order and folds
// round results with the uniform 4096-byte advance.

constexpr int kWavesPerBlock = kBlockThreads / 64;

struct Round {
    uint32_t w[4][4];  // [load register][dword]
};

__device__ __forceinline__ void load_round(Round &r, const uint8_t *base, uint32_t lane_off) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const u32x4 v = ld16(base + 1024 * t + lane_off);
        r.w[t][0] = v.x;
        r.w[t][1] = v.y;
        r.w[t][2] = v.z;
        r.w[t][3] = v.w;
    }
}

// A wave-uniform 64-bit value made provably uniform (two v_readfirstlane): downstream
// arithmetic then stays in SGPRs/SALU instead of 64-bit VALU per use.
__device__ __forceinline__ uint64_t rfl64(uint64_t x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(x));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(x >> 32));
    return (uint64_t(hi) << 32) | lo;
}

// Same, through a buffer resource built from the wave-uniform round base (scalar
// registers, made provably uniform by readfirstlane: cdna_hip_programming.md T8/T20).
// The lane's constant byte offset is the only VGPR operand, so no 64-bit VGPR address
// temporaries exist that the allocator could alias with in-flight load destinations
// (which made the compiler drain the previous round's loads before each prefetch).
// nb: the round's valid bytes (the resource's range; a partial round's lanes past it load zeros
// without touching memory). Non-temporal loads (nt): a round is read once
__device__ __forceinline__ void load_round_buf(Round &r, const uint8_t *base, uint32_t lane_off, uint32_t nb = 4096) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(b));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(b >> 32));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>((uint64_t(hi) << 32) | lo), 0, __builtin_amdgcn_readfirstlane(nb), 0x00020000);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off + 1024 * t, 0, 2);
        r.w[t][0] = v.x;
        r.w[t][1] = v.y;
        r.w[t][2] = v.z;
        r.w[t][3] = v.w;
    }
}

__device__ __forceinline__ void swap32(uint32_t &a, uint32_t &b) {
    const auto p = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = p[0];
    b = p[1];
}
__device__ __forceinline__ void swap16(uint32_t &a, uint32_t &b) {
    const auto p = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = p[0];
    b = p[1];
}

// (row, register) 4x4 transpose, see above.
__device__ __forceinline__ void regroup(Round &r) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        swap32(r.w[0][k], r.w[2][k]);
        swap32(r.w[1][k], r.w[3][k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        swap16(r.w[0][k], r.w[1][k]);
        swap16(r.w[2][k], r.w[3][k]);
    }
}

// y = M x over GF(2), M given by its 32 columns.
__device__ __forceinline__ uint32_t gf2_apply(const uint32_t (&col)[32], uint32_t x) {
    uint32_t y = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const uint32_t m = uint32_t(int32_t(x << (31 - i)) >> 31);
        y ^= m & col[i];
    }
    return y;
}

// Same product, 4 independent accumulators and one v_bitop3 (y ^ (m & col), truth
// table 0x78 over {S0,S1,S2}) per bit: 64 VALU in chains of 8 instead of 96 in one chain.
__device__ __forceinline__ uint32_t gf2_apply4(const uint32_t (&col)[32], uint32_t x) {
    uint32_t y[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const uint32_t m = uint32_t(int32_t(x << (31 - i)) >> 31);
        y[i & 3] = __builtin_amdgcn_bitop3_b32(y[i & 3], m, col[i], 0x78);
    }
    return xor3(y[0], y[1], y[2]) ^ y[3];
}

template <int DPP>
__device__ __forceinline__ uint32_t dpp_xor(uint32_t v) {
    // bound_ctrl: every lane of these patterns has a source; it lets the DPP combiner fold the
    // move into the xor (v_xor_b32_dpp), row_half_mirror included
    return v ^ uint32_t(__builtin_amdgcn_update_dpp(0, int(v), DPP, 0xF, 0xF, true));
}

// XOR-reduce over aligned groups of G lanes; the group total lands in (at least) the
// group's first lane.
template <int G>
__device__ __forceinline__ uint32_t group_xor(uint32_t v) {
    v = dpp_xor<0xB1>(v);   // quad_perm [1,0,3,2]
    v = dpp_xor<0x4E>(v);   // quad_perm [2,3,0,1]
    v = dpp_xor<0x141>(v);  // row_half_mirror: 8-lane total
    if constexpr (G >= 16) v = dpp_xor<0x140>(v);  // row_mirror: 16-lane total
    if constexpr (G >= 32) {
        uint32_t a = v, b = v;
        swap16(a, b);  // b's even rows now hold the odd rows' totals
        v ^= b;
    }
    if constexpr (G >= 64) {
        uint32_t a = v, b = v;
        swap32(a, b);  // b's lower half now holds the upper half's total
        v ^= b;
    }
    return v;
}

// The multi-round kernel: chunks of R = BPC / 4096 whole rounds (8 / 16 / 64 KiB below kPiecesMinBytes per
// launch). A wave's unit is one chunk: its rounds in order, one in flight beside the one it consumes, each
// folded with the G = 64 lane-fold columns, the chunk's running state advanced by the 4096-byte matrix.
template <int BPC, bool VERIFY, bool PRIO = false>
__global__ __launch_bounds__(kBlockThreads) void crc32c_rounds_kernel(ChunkLaunch a,
                                                                      const uint32_t *__restrict__ g_tab,
                                                                      const uint32_t *__restrict__ g_fold) {
    static_assert(BPC > kRoundBytes && BPC % kRoundBytes == 0, "chunks of two or more whole rounds");
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsBytes / 4];
    constexpr int kUnit = BPC, kRoundsPerUnit = kUnit / kRoundBytes;  // a wave's work unit: one chunk
    constexpr int G = 64, kFoldOff = 56;  // lanes per chunk in a round; their columns (crc32c_tables.h: kFoldOffset[3])

    const uint32_t lane = threadIdx.x & 63, j = lane;
    const uint32_t lane_off = 64 * (lane & 15) + 16 * (lane >> 4);
    const uint64_t nunits = a.len / kUnit;
    const uint64_t nwaves = uint64_t(gridDim.x) * kWavesPerBlock;
    const uint64_t wave = uint64_t(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    // this wave's rounds: k = 0..K-1 -> unit wave + (k / RPU) * nwaves, sub-round k % RPU
    const uint64_t my_units = wave < nunits ? (nunits - wave + nwaves - 1) / nwaves : 0;
    const uint64_t K = my_units * kRoundsPerUnit;
    const bool crc_al4 = (reinterpret_cast<uintptr_t>(VERIFY ? a.crc_be : a.out_be) & 3u) == 0;
    // byte offset of round k; rounds past the end re-read the wave's last round
    // (cache-resident) so every prefetch stays unconditional
    auto round_ptr = [&](uint64_t k) -> const uint8_t * {
        if (K == 0) return a.data;  // host guarantees nunits >= 1; idle wave reads unit 0
        const uint64_t kk = k < K ? k : K - 1;
        return a.data + (wave + (kk / kRoundsPerUnit) * nwaves) * kUnit + (kk % kRoundsPerUnit) * kRoundBytes;
    };

    // small cache-resident reads first (tables, fold columns), then the first
    // round: the in-order vmcnt then lets the table fill proceed while rounds land
    uint32_t col[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) col[i] = g_fold[(kFoldOff + j) * 32 + i];
    uint32_t tv[kFillPerThread];
    fetch_tables(tv, g_tab);
    __builtin_amdgcn_sched_barrier(0);
    Round b0, b1;
    load_round(b0, round_ptr(0), lane_off);
    __builtin_amdgcn_sched_barrier(0);
    store_tables(lds, tv);
    lds_barrier();
    const Lut t(lds);

    uint32_t acc = 0;
    // One round: issue the stored CRC word and the prefetch of round k+1 into
    // `pf`, then consume `cur`.
    auto step = [&](Round &cur, Round &pf, uint64_t k) {
        const uint32_t r = uint32_t(k % kRoundsPerUnit);
        const uint64_t chunk = wave + (k / kRoundsPerUnit) * nwaves;  // the wave's unit is one chunk
        uint32_t want = 0;
        if constexpr (VERIFY) {
            // every lane of a chunk reads its word (one broadcast access), issued before
            // the prefetch so that waiting for it never drains the prefetch (vmcnt is in-order)
            want = *reinterpret_cast<const uint32_t *>(a.crc_be + 4 * chunk);
        }
        load_round(pf, round_ptr(k + 1), lane_off);
        __builtin_amdgcn_sched_barrier(0);
        regroup(cur);
        uint32_t x = ((j == 0 && r == 0) ? 0xFFFFFFFFu : 0u) ^ cur.w[0][0];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x = t.word(x, cur.w[q][1]);
            x = t.word(x, cur.w[q][2]);
            x = t.word(x, cur.w[q][3]);
            x = t.word(x, q < 3 ? cur.w[q < 3 ? q + 1 : 3][0] : 0u);
        }
        uint32_t y = group_xor<G>(gf2_apply4(col, x));
        if (r > 0) {
            uint32_t k4096[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) k4096[i] = g_fold[kFoldAdvance4096 + i];
            y ^= gf2_apply(k4096, acc);
        }
        acc = y;
        if (r == kRoundsPerUnit - 1 && j == 0) {
            const uint32_t c = ~acc;
            if constexpr (VERIFY) {
                if (__builtin_bswap32(want) != c)
                    atomicMax(a.result, ~(unsigned long long)(a.chunk_base + chunk));
            } else {
                *reinterpret_cast<uint32_t *>(a.out_be + 4 * chunk) = __builtin_bswap32(c);
            }
        }
    };
    // PRIO (lab 115): s_setprio by the quartile of rounds left for waves of >= 16 rounds, as the round
    // kernel does (crc32c_wave.h, kPrioMinRounds). Measured 1-2 us per GiB SLOWER here at bpc 8192 and
    // 65536 (profiles/r03/reentry/r3za_r8k_*.jsonl), so production leaves the arbiter's order.
    const bool use_prio = PRIO && K >= 16;
    auto prio = [&](uint64_t k) {
        if (use_prio && (k & 3) == 0) {
            const uint64_t left = K - k;
            if (left * 4 > 3 * K) __builtin_amdgcn_s_setprio(3);
            else if (left * 4 > 2 * K) __builtin_amdgcn_s_setprio(2);
            else if (left * 4 > K) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
    };
    // two buffers unrolled so they rotate by renaming (a loop-carried
    // register copy would make the compiler wait for the youngest prefetch)
    for (uint64_t k = 0; k < K; k += 2) {
        prio(k);
        step(b0, b1, k);
        if (k + 1 >= K) break;
        step(b1, b0, k + 1);
    }

    // Slow region: chunks after the last whole unit, plus the short tail chunk, one
    // lane per chunk (at most a unit's worth, so a handful of lanes).
    const uint64_t nfull = a.len / BPC;
    const uint64_t first_slow = nunits;
    const uint64_t nslow = nfull - first_slow + (a.len % BPC ? 1 : 0);
    const uint64_t gtid = uint64_t(blockIdx.x) * kBlockThreads + threadIdx.x;
    if (gtid < nslow) {
        const uint64_t chunk = first_slow + gtid;
        const uint32_t sz = chunk < nfull ? uint32_t(BPC) : uint32_t(a.len % BPC);
        const uint32_t c = ~crc_run_lines(t, 0xFFFFFFFFu, a.data + chunk * BPC, sz);
        if constexpr (VERIFY) {
            if ((sz == uint32_t(BPC) || a.check_short_tail) && load_be32(a.crc_be + 4 * chunk, crc_al4) != c)
                atomicMax(a.result, ~(unsigned long long)(a.chunk_base + chunk));
        } else {
            store_be32(a.out_be + 4 * chunk, c, crc_al4);
        }
    }
}

// ---- pieces of the production round kernel (crc32c_wave.h) -----------------------
//
// Same rounds/regroup as crc32c_rounds_kernel, two changes:
//  * the lane fold M_j (advance over (G-1-j)*64 bytes) reads lane-specific nibble
//    tables kept in LDS after the slice tables (word ((k*16+e)*64 + lane): each lane its
//    own bank): 8 lookups + ~19 VALU instead of a 32-column product in VGPRs; for G <= 32
//    the half-size image of fold_half below;
//  * a step consumes two rounds with their lookup chains software-pipelined
//    (sched_barrier-pinned phases: chain 1's 4 reads fly while chain 0 folds its
//    previous 4), so each lane keeps two LDS round trips in flight.
constexpr int kFoldLdsOff = kLdsBytes;                  // byte offset of the nibble tables
constexpr int kLdsBytesWave = kLdsBytes + 32 * 1024;    // 160 KiB: the whole CU LDS

struct NibFold {
    const uint8_t *f;  // lds + kFoldLdsOff + lane*4
    __device__ __forceinline__ explicit NibFold(const uint32_t *lds)
        : f(reinterpret_cast<const uint8_t *>(lds) + kFoldLdsOff + 4 * (threadIdx.x & 63)) {}
    __device__ __forceinline__ uint32_t ld(uint32_t off) const {
        return *reinterpret_cast<const uint32_t *>(f + off);
    }
    __device__ __forceinline__ uint32_t apply(uint32_t x) const {
        const uint32_t a0 = ld(((x << 8) & 0xF00u) + 0 * 4096);
        const uint32_t a1 = ld(((x << 4) & 0xF00u) + 1 * 4096);
        const uint32_t a2 = ld((x & 0xF00u) + 2 * 4096);
        const uint32_t a3 = ld(((x >> 4) & 0xF00u) + 3 * 4096);
        const uint32_t a4 = ld(((x >> 8) & 0xF00u) + 4 * 4096);
        const uint32_t a5 = ld(((x >> 12) & 0xF00u) + 5 * 4096);
        const uint32_t a6 = ld(((x >> 16) & 0xF00u) + 6 * 4096);
        const uint32_t a7 = ld(((x >> 20) & 0xF00u) + 7 * 4096);
        return xor3(xor3(a0, a1, a2), xor3(a3, a4, a5), a6 ^ a7);
    }
};

// The 4 table reads of one word step, and their fold into the next state.
struct Look {
    uint32_t v[4];
};
__device__ __forceinline__ Look lookups(const Lut &t, uint32_t x) {
    Look l;
    l.v[0] = t.at<0>(3, x);
    l.v[1] = t.at<1>(2, x);
    l.v[2] = t.at<2>(1, x);
    l.v[3] = t.at<3>(0, x);
    return l;
}
__device__ __forceinline__ uint32_t combine(const Look &l, uint32_t next) {
    return xor3(xor3(l.v[0], l.v[1], l.v[2]), l.v[3], next);
}

// The half-size lane-fold image (G <= 32: lanes l and l + 32 hold the same fold tables and
// never share a ds_read cycle, so 32 columns serve the wave), 16 KiB after the slice tables.
// Word (k >> 1) * 1024 + e * 64 + (k & 1) * 32 + (lane & 31) = M_j(e << 4k): the nibble sits in
// address byte 1, so ONE v_perm on the nibble-spread state builds each address, and
// (k >> 1) * 4096 + (k & 1) * 128 rides in the ds_read offset.
constexpr int kHalfFoldOff = kLdsBytes;  // 128 KiB

// OFF: byte offset of the image; its 64 KiB part rides in address byte 2 (the nibble owns
// byte 1), the rest in the ds_read immediate offset
template <int OFF = kHalfFoldOff>
__device__ __forceinline__ uint32_t fold_half(const uint8_t *lds, uint32_t x) {
    const uint32_t lo = x & 0x0F0F0F0Fu, hi = (x >> 4) & 0x0F0F0F0Fu;
    const uint32_t fb = (OFF & ~0xFFFF) + 4 * (threadIdx.x & 31);
    auto at = [&](uint32_t src, uint32_t byte, int off) {
        const uint32_t addr = __builtin_amdgcn_perm(src, fb, 0x0C020000u | ((4u + byte) << 8));
        return *reinterpret_cast<const uint32_t *>(lds + addr + (OFF & 0xFFFF) + off);
    };
    const uint32_t a0 = at(lo, 0, 0), a1 = at(hi, 0, 128), a2 = at(lo, 1, 4096), a3 = at(hi, 1, 4096 + 128);
    const uint32_t a4 = at(lo, 2, 8192), a5 = at(hi, 2, 8192 + 128), a6 = at(lo, 3, 12288);
    const uint32_t a7 = at(hi, 3, 12288 + 128);
    return xor3(xor3(a0, a1, a2), xor3(a3, a4, a5), a6 ^ a7);
}

// ---- segment lists (blocks of a batch, packets): crc32c_segments_kernel, crc32c_wave.h ----

struct SegLaunch {
    const DevSegment *seg;  // device array, or nullptr: use inl[] (nseg <= kInlineSegments)
    uint32_t nseg;
    uint64_t units;
    uint64_t uniform;
    unsigned long long *result;
    int check_short_tail;
    // stride != 0: packet i is {inl[0].data + i*stride, inl[0].crc + i*stride, inl[0].len,
    // key i << 32}, the last one with inl[1].len (uniform view only). Packets laid out at a
    // constant pitch in one arena need no descriptor array at all.
    uint64_t stride;
    uint32_t kq, kr;  // a wave's round count: kq + (wave < kr), split on the host (launch_segments)
    // non-null (bpc = R x 4096 descriptor lists, round 6): unit u's words go to dense_words + 4 * CPU * u
    // instead of the segment's own array (the 4096-byte piece CRCs a combine folds), and the segments'
    // short tails are left to the caller
    uint8_t *dense_words;
    // non-null (long descriptor lists, round 6): unit u lies in segment unit_seg[u] (one scalar load
    // instead of a binary search per round; crc32c_unit_map_kernel builds it)
    const uint32_t *unit_seg;
    DevSegment inl[kInlineSegments];
};

// Packet kernel: one wave per packet (grid-stride over packets), lanes over that
// packet's chunks. Result key = (packet << 32 | chunk), atomicMax of its complement
// keeps the lexicographically first bad (packet, chunk).
template <bool VERIFY>
__global__ __launch_bounds__(kBlockThreads) void crc32c_packets_kernel(
    const uint8_t *arena_c, uint8_t *arena_w, const DevPacket *__restrict__ pk,
    uint64_t n, uint32_t bpc, int check_short_tail, unsigned long long *result,
    const uint32_t *__restrict__ g_tab) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsBytes / 4];
    fill_tables(lds, g_tab);
    lds_barrier();
    const Lut t(lds);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = uint64_t(gridDim.x) * (kBlockThreads / 64);
    for (uint64_t w = uint64_t(blockIdx.x) * (kBlockThreads / 64) + (threadIdx.x >> 6); w < n;
         w += waves) {
        const DevPacket d = pk[w];
        const uint32_t chunks = (d.data_len + bpc - 1) / bpc;
        const uint8_t *data = arena_c + d.data_off;
        const bool al4 = (reinterpret_cast<uintptr_t>(arena_c + d.crc_off) & 3u) == 0;
        for (uint32_t k = lane; k < chunks; k += 64) {
            const uint32_t off = k * bpc;
            const uint32_t sz = d.data_len - off < bpc ? d.data_len - off : bpc;
            const uint32_t c = ~crc_run_any(t, 0xFFFFFFFFu, data + off, sz);
            if constexpr (VERIFY) {
                if ((sz == bpc || check_short_tail) &&
                    load_be32(arena_c + d.crc_off + 4ull * k, al4) != c)
                    atomicMax(result, ~((uint64_t(w) << 32) | k));
            } else {
                store_be32(arena_w + d.crc_off + 4ull * k, c, al4);
            }
        }
    }
}

template <bool V>
hipError_t launch_t(const ChunkLaunch &a, const uint32_t *tab, int grid, hipStream_t s) {
    hipLaunchKernelGGL((crc32c_chunks_kernel<V>), dim3(grid), dim3(kBlockThreads), 0, s, a, tab);
    return hipGetLastError();
}

template <int BPC, bool V, bool PRIO = false>
hipError_t launch_r3(const ChunkLaunch &a, const uint32_t *tab, const uint32_t *fold, int grid_cap, hipStream_t s) {
    const uint64_t units = a.len / BPC;
    const uint64_t need = (units + kWavesPerBlock - 1) / kWavesPerBlock;
    const int grid = int(need < uint64_t(grid_cap) ? need : uint64_t(grid_cap));
    hipLaunchKernelGGL((crc32c_rounds_kernel<BPC, V, PRIO>), dim3(grid), dim3(kBlockThreads), 0, s, a, tab, fold);
    return hipGetLastError();
}

}  // namespace
}  // namespace hdfs3crc
