// gfx950 (CDNA4) CRC32C kernels for libhdfs3's per-chunk checksum path: production launchers.
// The device code (kernels, design notes) is in crc32c_device.h and crc32c_wave.h; the kernel variants
// kept for A/B are in crc32c_experiments.hip; which launcher a batch takes is decided in launch_plan.cpp.
#include "crc32c_wave.h"

namespace hdfs3crc {

#if HDFS3_LAB
int g_variant = 0;  // measurement knob (hdfs3x_set_variant); 0 = production choice
#endif

namespace {

// a grid of `want` workgroups, at most `cap`
inline int clamped_grid(uint64_t want, uint64_t cap) { return int(want < cap ? want : cap); }

template <int BPC, bool V>
hipError_t launch_r(const LaunchEnv &env, const ChunkLaunch &a) {
    // Production path: the round kernel of crc32c_wave.h for bpc <= 4096, late prefetch, the solo
    // last step for overlapped launches up to 256 MiB (HDFS3_LAUNCH_OVERLAP_PREVIOUS: an AQL packet
    // without the barrier bit); the multi-round kernel above 4096. Non-zero variants select the designs kept
    // for in-process A/B (crc32c_experiments.hip, tools/ab.py).
#if HDFS3_LAB
    if (g_variant != 0) return launch_experiment(env, g_variant, a, V);
#endif
    if constexpr (BPC <= kRoundBytes)
        return launch_wave3<BPC, V, false, true>(a, env.tables, env.fold, env.grid_cap, env.stream);
    else
        return launch_r3<BPC, V>(a, env.tables, env.fold, env.grid_cap, env.stream);
}

// packet streams at a constant pitch: the production round kernel's pitch walk
template <int BPC, bool V>
hipError_t launch_p(const LaunchEnv &env, const ChunkLaunch &a) {
    const auto [tab, fold, grid_cap, s] = std::tie(env.tables, env.fold, env.grid_cap, env.stream);
#if HDFS3_LAB
    if (g_variant == 115) return launch_wave3<BPC, V, true, true, kLabPrio>(a, tab, fold, grid_cap, s);
    if (g_variant == 117) return launch_wave3<BPC, V, true, true, kLabNoPrio>(a, tab, fold, grid_cap, s);
    // without the solo last step (production before round 4)
    if (g_variant == 124) return launch_wave3<BPC, V, true, false>(a, tab, fold, grid_cap, s);
    // 256-thread workgroups (4 waves each): small launches spread over 4x the CUs
    if (g_variant == 132) return launch_wave3<BPC, V, true, true, 0, 256>(a, tab, fold, grid_cap, s);
    if (g_variant == 134) return launch_wave3<BPC, V, true, true, 0, 512>(a, tab, fold, grid_cap, s);
    if (g_variant == 137) return launch_wave3<BPC, V, true, true, kLabWg1024>(a, tab, fold, grid_cap, s);
    // compute: each round's words stored at once at every size (round 6, the writer's small batches)
    if (g_variant == 163) return launch_wave3<BPC, V, true, true, kLabNoHold>(a, tab, fold, grid_cap, s);
    // one round per wave for launches of <= 4096 units (round 6)
    if (g_variant == 162) return launch_wave3<BPC, V, true, true, kLabOneRound>(a, tab, fold, grid_cap, s);
#endif
    // the solo last step for overlapped launches up to 256 MiB, as the block walk (round 4): 128 MiB of
    // 64 KiB packets at the block reader's 66,048-byte pitch 22.53 -> 20.98 us overlapped against 20.97
    // for the same payload as one contiguous block (tools/pkt_ab.py, profiles/r04/r4c_pkt_ab*)
    return launch_wave3<BPC, V, true, true>(a, tab, fold, grid_cap, s);
}

hipError_t launch_stream_kernel(const LaunchEnv &env, const ChunkLaunch &a, bool verify) {
    return dispatch_bpc(a.bpc, [&](auto bpc) {
        return verify ? launch_p<bpc(), true>(env, a) : launch_p<bpc(), false>(env, a);
    });
}

// the verify (k_verify = k<true>) or the compute (k<false>) form of a kernel
template <class... P, class... A>
hipError_t launch_vc(bool verify, void (*k_verify)(P...), void (*k_compute)(P...), int grid, int block,
                     hipStream_t stream, A... args) {
    hipLaunchKernelGGL(verify ? k_verify : k_compute, dim3(grid), dim3(block), 0, stream, args...);
    return hipGetLastError();
}

// Makes *d a device buffer of at least `need` bytes (*cap) and *used an event: a buffer that has to
// grow is freed only after *used fired, since a launch in flight (on any stream) may still read it
hipError_t grow_scratch(uint8_t **d, uint64_t *cap, hipEvent_t *used, uint64_t need) {
    if (need > *cap) {
        if (*used) {
            hipError_t e = hipEventSynchronize(*used);
            if (e != hipSuccess) return e;
        }
        if (*d) (void)hipFree(*d);
        *d = nullptr;
        *cap = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(d), need);
        if (e != hipSuccess) return e;
        *cap = need;
    }
    return *used ? hipSuccess : hipEventCreateWithFlags(used, hipEventDisableTiming);
}

// packet p's `words` bytes (`last` for the last packet) from src + p * src_pitch to
// dst + p * dst_pitch: one wave per packet at a time, 64 consecutive words per store
__global__ __launch_bounds__(256) void crc32c_scatter_words_kernel(const uint8_t *__restrict__ src, uint8_t *dst,
                                                                   uint64_t src_pitch, uint64_t dst_pitch,
                                                                   uint64_t npk, uint32_t words, uint32_t last) {
    const uint64_t nwaves = uint64_t(gridDim.x) * 4;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t p = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); p < npk; p += nwaves) {
        const uint32_t nw = (p + 1 == npk ? last : words) / 4;
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src + p * src_pitch);
        uint32_t *d = reinterpret_cast<uint32_t *>(dst + p * dst_pitch);
        for (uint32_t i = lane; i < nw; i += 64) d[i] = s[i];
    }
}

}  // namespace

void PieceScratch::release() {
    for (int i = 0; i < 2; ++i) {
        if (d[i]) (void)hipFree(d[i]);
        if (used[i]) (void)hipEventDestroy(used[i]);
    }
    *this = PieceScratch();
}

namespace {

// Chunk c of R 4096-byte pieces from the pieces' CRCs y_i (standard init and final xor, BE words in
// `piece_be`): with A = the 4096-zero-byte advance (d_fold + kFoldAdvance4096) and crc0 the raw
// (init 0, no final xor) CRC, crc0(P_i) = y_i ^ K, K = A(~0) ^ ~0, and the chunk's state from init ~0
// is s = A(... A(A(~0) ^ crc0(P_0)) ...) ^ crc0(P_{R-1}); its CRC is ~s. One chunk per thread.
// cpp > 0 (packet streams, round 4): chunk k is chunk k % cpp of packet k / cpp, its word at
// crc + (k / cpp) * cpitch + 4 (k % cpp) and its key (packet << 32) | chunk; the pieces stay dense.
template <bool VERIFY>
__global__ __launch_bounds__(256) void crc32c_combine_pieces_kernel(const uint8_t *__restrict__ piece_be, uint64_t nchunks,
                                                                    uint32_t R, const uint32_t *__restrict__ g_fold,
                                                                    const uint8_t *crc_be, uint8_t *out_be,
                                                                    uint64_t chunk_base,
                                                                    unsigned long long *result, uint64_t cpp = 0,
                                                                    uint64_t cpitch = 0) {
    uint32_t col[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) col[i] = g_fold[kFoldAdvance4096 + i];
    const uint32_t K = gf2_apply4(col, 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
    const uint32_t *y = reinterpret_cast<const uint32_t *>(piece_be);
    for (uint64_t c = uint64_t(blockIdx.x) * 256 + threadIdx.x; c < nchunks; c += uint64_t(gridDim.x) * 256) {
        uint32_t st = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < R; ++i) st = gf2_apply4(col, st) ^ __builtin_bswap32(y[c * R + i]) ^ K;
        const uint32_t v = ~st;
        uint64_t woff = 4 * c, key = chunk_base + c;
        if (cpp) {
            const uint64_t pk = c / cpp, ch = c % cpp;
            woff = pk * cpitch + 4 * ch;
            key = (pk << 32) | ch;
        }
        if constexpr (VERIFY) {
            if (__builtin_bswap32(*reinterpret_cast<const uint32_t *>(crc_be + woff)) != v)
                atomicMax(result, ~(unsigned long long)key);
        } else {
            *reinterpret_cast<uint32_t *>(out_be + woff) = __builtin_bswap32(v);
        }
    }
}

// The next of the two piece buffers, at least `need` bytes, ordered after its previous reader.
hipError_t piece_buffer(PieceScratch *ps, uint64_t need, hipStream_t stream, unsigned *out) {
    const unsigned b = ps->next & 1u;
    const bool read_before = ps->used[b] != nullptr;
    if (hipError_t e = grow_scratch(&ps->d[b], &ps->cap[b], &ps->used[b], need); e != hipSuccess) return e;
    if (read_before && ps->on[b] != stream) {
        // the last reader of this buffer ran on another stream (the ctx's stream was switched):
        // order this launch after it; on one stream the launch order already does
        hipError_t e = hipStreamWaitEvent(stream, ps->used[b], 0);
        if (e != hipSuccess) return e;
    }
    ps->on[b] = stream;
    ps->next = b + 1;
    *out = b;
    return hipSuccess;
}

// The combine of nfull chunks of R pieces each out of piece buffer b (crc32c_combine_pieces_kernel; cpp > 0: a
// packet stream), then the event that lets the buffer be reused
hipError_t launch_combine(const LaunchEnv &env, const ChunkLaunch &a, bool verify, unsigned b, uint64_t nfull,
                          uint64_t chunk_base, uint64_t cpp, uint64_t cpitch) {
    hipError_t e = hipSuccess;
    if (nfull)
        e = launch_vc(verify, crc32c_combine_pieces_kernel<true>, crc32c_combine_pieces_kernel<false>,
                      clamped_grid((nfull + 255) / 256, 1024), 256, env.stream, env.pieces->d[b], nfull,
                      a.bpc / kRoundBytes, env.fold, verify ? a.crc_be : nullptr, verify ? nullptr : a.out_be,
                      chunk_base, a.result, cpp, cpitch);
    return e != hipSuccess ? e : hipEventRecord(env.pieces->used[b], env.stream);
}

// a's short last chunk, `tail` bytes at data, its word at byte `word` of a's words: one lane of the byte-exact kernel
hipError_t launch_tail_chunk(const LaunchEnv &env, const ChunkLaunch &a, bool verify, const uint8_t *data,
                             uint64_t tail, uint64_t word, uint64_t key) {
    if (tail == 0) return hipSuccess;
    ChunkLaunch t{};
    t.data = data;
    t.len = tail;
    t.bpc = a.bpc;
    t.chunk_base = key;
    t.check_short_tail = a.check_short_tail;
    t.result = a.result;
    if (verify) t.crc_be = a.crc_be + word;
    else t.out_be = a.out_be + word;
    return verify ? launch_t<true>(t, env.tables, 1, env.stream) : launch_t<false>(t, env.tables, 1, env.stream);
}

// Whole chunks of R = bpc / 4096 pieces: the round kernel's compute at bpc 4096 into the scratch,
// then the combine. The short tail chunk (if any) goes to the chunk-per-lane kernel.
hipError_t launch_pieces(const LaunchEnv &env, const ChunkLaunch &a, bool verify) {
    PieceScratch *ps = env.pieces;
    const uint32_t R = a.bpc / kRoundBytes;
    const uint64_t nfull = a.len / a.bpc;
    unsigned b = 0;
    if (hipError_t e = piece_buffer(ps, nfull * R * 4, env.stream, &b); e != hipSuccess) return e;
    ChunkLaunch p = a;  // the pieces: a compute at bpc 4096 over the whole chunks
    p.len = nfull * a.bpc;
    p.bpc = kRoundBytes;
    p.out_be = ps->d[b];
    p.crc_be = nullptr;
    p.chunk_base = 0;
    hipError_t e = launch_wave3<kRoundBytes, false, false, true>(p, env.tables, env.fold, env.grid_cap, env.stream);
    if (e != hipSuccess) return e;
    if ((e = launch_combine(env, a, verify, b, nfull, a.chunk_base, 0, 0)) != hipSuccess) return e;
    return launch_tail_chunk(env, a, verify, a.data + nfull * a.bpc, a.len - nfull * a.bpc, 4 * nfull,
                             a.chunk_base + nfull);
}

}  // namespace

// A packet stream whose chunks are R = bpc / 4096 whole rounds (64 KiB datanode packets at bpc 8192
// ... 65536; round 4). The pitch walk computes every 4096-byte piece's CRC densely into the piece
// scratch (packet p's pieces at 4 (p * upp + i)), the combine folds each chunk's R pieces and
// compares with (verify) or writes (compute) the word in the packet's own CRC region, key
// (packet << 32) | chunk; the last packet's short chunk, if any, takes the byte-exact kernel.
// Until round 4 these streams took the chunk-per-lane packet kernel.
hipError_t launch_stream_pieces(const LaunchEnv &env, const ChunkLaunch &a, bool verify) {
    PieceScratch *ps = env.pieces;
    const uint64_t upp = a.geom.upp;
    const uint64_t cpp = a.geom.pk_len / a.bpc;              // chunks per packet
    const uint64_t lfull = a.last_len / a.bpc;               // whole chunks of the last packet
    const uint64_t nfull = (a.npk - 1) * cpp + lfull;
    const uint64_t npieces = (a.npk - 1) * upp + (uint64_t(a.last_len) + kRoundBytes - 1) / kRoundBytes;
    const uint64_t cpitch = a.crc_pitch ? a.crc_pitch : a.pitch;
    unsigned b = 0;
    if (hipError_t e = piece_buffer(ps, npieces * 4, env.stream, &b); e != hipSuccess) return e;
    ChunkLaunch p = a;  // the pieces: a compute at bpc 4096 over the stream, words dense in the scratch
    p.bpc = kRoundBytes;
    p.out_be = ps->d[b];
    p.crc_be = ps->d[b];
    p.crc_pitch = upp * 4;
    p.check_short_tail = 1;
    hipError_t e = launch_stream_kernel(env, p, false);
    if (e != hipSuccess) return e;
    if ((e = launch_combine(env, a, verify, b, nfull, 0, cpp, cpitch)) != hipSuccess) return e;
    const uint64_t lp = a.npk - 1;  // the last packet's short chunk
    return launch_tail_chunk(env, a, verify, a.data + lp * a.pitch + lfull * a.bpc, a.last_len % a.bpc,
                             lp * cpitch + 4 * lfull, (lp << 32) | lfull);
}

void WordScratch::release() {
    if (d) (void)hipFree(d);
    if (used) (void)hipEventDestroy(used);
    *this = WordScratch();
}

hipError_t launch_packet_stream(const LaunchEnv &env, const ChunkLaunch &a, bool verify) {
    WordScratch *ws = env.words;
#if HDFS3_LAB
    if (g_variant == 55) ws = nullptr;  // A/B: words written in place (no dense scratch)
#endif
    // chunks of R whole rounds: pieces + combine (plan_packet_stream refuses them without a piece scratch)
    if (pieces_bpc(a.bpc)) return env.pieces ? launch_stream_pieces(env, a, verify) : hipErrorInvalidValue;
    if (!round_bpc(a.bpc)) return hipErrorInvalidValue;
    const uint64_t cpitch = a.crc_pitch ? a.crc_pitch : a.pitch;
    const uint64_t wpp = a.geom.pk_len / a.bpc * 4;  // word bytes per packet
    if (!verify && ws && a.npk > 1 && cpitch > wpp && wpp <= kDenseWordsMaxRegion) {
        const uint64_t last = (uint64_t(a.last_len) + a.bpc - 1) / a.bpc * 4;
        hipError_t e = grow_scratch(&ws->d, &ws->cap, &ws->used, (a.npk - 1) * wpp + last);
        if (e != hipSuccess) return e;
        ChunkLaunch b = a;
        b.out_be = ws->d;
        b.crc_be = ws->d;
        b.crc_pitch = wpp;
        e = launch_stream_kernel(env, b, false);
        if (e != hipSuccess) return e;
        const int grid = clamped_grid((a.npk + 3) / 4, 1024);  // a wave per packet, 4 per workgroup
        hipLaunchKernelGGL(crc32c_scatter_words_kernel, dim3(grid), dim3(256), 0, env.stream, ws->d, a.out_be, wpp,
                           cpitch, a.npk, uint32_t(wpp), uint32_t(last));
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        return hipEventRecord(ws->used, env.stream);
    }
    return launch_stream_kernel(env, a, verify);
}

hipError_t launch_chunks(const LaunchEnv &env, const ChunkLaunch &a, bool verify) {
    const uint64_t chunks = (a.len + a.bpc - 1) / a.bpc;
    if (chunks == 0) return hipSuccess;
    const bool aligned = (reinterpret_cast<uintptr_t>(a.data) & 15u) == 0 &&
                         (reinterpret_cast<uintptr_t>(verify ? a.crc_be : a.out_be) & 3u) == 0;
    const uint64_t unit = a.bpc <= uint32_t(kRoundBytes) ? uint64_t(kRoundBytes) : a.bpc;
    const PieceScratch *pieces = env.pieces;
#if HDFS3_LAB
    if (g_variant == 123) pieces = nullptr;  // A/B: the multi-round kernel (before r3zf)
#endif
    // pieces + combine from 256 MiB per launch: 1 GiB at bpc 8192 / 16384 / 65536 172.7 / 173.5 / 174.4 us
    // against 196.0 / 200.6 / 209.1 for the multi-round kernel, but the combine's own launch (~6 us,
    // latency-bound) loses 0.9 us at 128 MiB (profiles/r03/reentry/r3zf_*.jsonl); chunk sizes the
    // multi-round kernel does not cover (12 KiB, 32 KiB, ...) take the pieces at every length
    const bool multi_round = a.bpc == 8192 || a.bpc == 16384 || a.bpc == 65536;
    if (pieces && aligned && pieces_bpc(a.bpc) && a.len >= a.bpc && (!multi_round || a.len >= kPiecesMinBytes))
        return launch_pieces(env, a, verify);
    if (aligned && a.len >= unit && (round_bpc(a.bpc) || multi_round))
        return dispatch_bpc<true>(a.bpc, [&](auto bpc) {
            return verify ? launch_r<bpc(), true>(env, a) : launch_r<bpc(), false>(env, a);
        });
    const int grid = clamped_grid((chunks + kBlockThreads - 1) / kBlockThreads, uint64_t(env.grid_cap));
    return verify ? launch_t<true>(a, env.tables, grid, env.stream)
                  : launch_t<false>(a, env.tables, grid, env.stream);
}

hipError_t launch_packets(const LaunchEnv &env, const uint8_t *d_arena, const DevPacket *d_pk, uint64_t n,
                          uint32_t bpc, bool verify, int check_short_tail, unsigned long long *result) {
    if (n == 0) return hipSuccess;
    constexpr uint64_t kWaves = kBlockThreads / 64;
    return launch_vc(verify, crc32c_packets_kernel<true>, crc32c_packets_kernel<false>,
                     clamped_grid((n + kWaves - 1) / kWaves, uint64_t(env.grid_cap)), kBlockThreads, env.stream,
                     d_arena, verify ? nullptr : const_cast<uint8_t *>(d_arena), d_pk, n, bpc,
                     verify ? check_short_tail : 0, result, env.tables);
}

template <int BPC, bool V>
hipError_t launch_seg_t(const LaunchEnv &env, const SegLaunch &L) {
    const auto [tab, fold, grid_cap, s] = std::tie(env.tables, env.fold, env.grid_cap, env.stream);
#if HDFS3_LAB
    if (g_variant == 115) return launch_segments3<BPC, V, kLabPrio>(L, tab, fold, grid_cap, s);
    if (g_variant == 117) return launch_segments3<BPC, V, kLabNoPrio>(L, tab, fold, grid_cap, s);
    // 1024-thread workgroups at every size (production before round 6)
    if (g_variant == 161) return launch_segments3<BPC, V, 0, 1024>(L, tab, fold, grid_cap, s);
#endif
    return launch_segments3<BPC, V>(L, tab, fold, grid_cap, s);
}

hipError_t launch_segments(const LaunchEnv &env, const DevSegment *d_seg, uint32_t nseg, uint64_t units,
                           uint64_t uniform, uint32_t bpc, bool verify, int check_short_tail,
                           unsigned long long *result, const DevSegment *h_inline, uint64_t stride,
                           uint8_t *dense_words, const uint32_t *unit_seg) {
    if (nseg == 0) return hipSuccess;
    SegLaunch L{};
    L.dense_words = dense_words;
    L.unit_seg = unit_seg;
    L.seg = d_seg;
    L.nseg = nseg;
    L.units = units;
    L.uniform = uniform;
    L.result = result;
    L.check_short_tail = check_short_tail;
    if (stride) {  // h_inline = {first packet, last packet}; the rest follow by pitch
        if (!h_inline || !uniform) return hipErrorInvalidValue;
        L.seg = nullptr;
        L.stride = stride;
        L.inl[0] = h_inline[0];
        L.inl[1] = h_inline[1];
    } else if (h_inline) {
        if (nseg > kInlineSegments) return hipErrorInvalidValue;
        L.seg = nullptr;
        for (uint32_t i = 0; i < nseg; ++i) L.inl[i] = h_inline[i];
    }
    return dispatch_bpc(bpc, [&](auto b) {
        return verify ? launch_seg_t<b(), true>(env, L) : launch_seg_t<b(), false>(env, L);
    });
}

namespace {

// Descriptor lists at bpc = R x 4096 that are not one constant-pitch stream (round 6): the segmented
// kernel computes every 4096-byte piece of every segment densely (segment i's pieces from piece
// unit_begin_i, SegLaunch::dense_words), then this combine folds each chunk from its R pieces
// (crc32c_combine_pieces_kernel's fold) and compares with / writes the segment's own word c, key
// key_base + c. One wave per segment at a time (grid-stride), its lanes over the segment's chunks: a
// datanode packet holds few chunks at these sizes (5 of 12 KiB, 1 of 64 KiB).
template <bool VERIFY>
__global__ __launch_bounds__(256) void crc32c_combine_segment_pieces_kernel(const DevSegment *__restrict__ seg,
                                                                            uint32_t n,
                                                                            const uint8_t *__restrict__ piece_be,
                                                                            uint32_t bpc,
                                                                            const uint32_t *__restrict__ g_fold,
                                                                            unsigned long long *result) {
    uint32_t col[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) col[i] = g_fold[kFoldAdvance4096 + i];
    const uint32_t K = gf2_apply4(col, 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
    const uint32_t R = bpc / kRoundBytes;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = uint64_t(gridDim.x) * 4;
    for (uint64_t si = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); si < n; si += nwaves) {
        const DevSegment sd = seg[si];
        const uint64_t nfull = sd.len / bpc;
        for (uint64_t c = lane; c < nfull; c += 64) {
            const uint32_t *y = reinterpret_cast<const uint32_t *>(piece_be) + sd.unit_begin + c * R;
            uint32_t st = 0xFFFFFFFFu;
            for (uint32_t i = 0; i < R; ++i) st = gf2_apply4(col, st) ^ __builtin_bswap32(y[i]) ^ K;
            const uint32_t v = ~st;
            if constexpr (VERIFY) {
                if (__builtin_bswap32(*reinterpret_cast<const uint32_t *>(sd.crc + 4 * c)) != v)
                    atomicMax(result, ~(unsigned long long)(sd.key_base + c));
            } else {
                *reinterpret_cast<uint32_t *>(sd.crc + 4 * c) = __builtin_bswap32(v);
            }
        }
    }
}

// unit -> segment map of a long descriptor list (SegLaunch::unit_seg): one wave per segment at a time,
// its lanes over the segment's units (seg_units at ubpc: its whole chunks in 4 KiB units). A segmented
// kernel's wave steps nwaves units per round, past dozens of short segments, so without the map every
// round began with a binary search, a chain of ~15 dependent scalar loads (25k segments): 1 GiB of
// 12 KiB-chunk packets 327.3 -> 253.2 us verify, the pieces kernel 252 -> 166 us (profiles/r06/r6x_*,
// r6za_*). A 16-ary search (15 scalar loads per level) measured slower (430 us): the compiler issued
// them two at a time
__global__ __launch_bounds__(256) void crc32c_unit_map_kernel(const DevSegment *__restrict__ seg, uint32_t n,
                                                              uint32_t ubpc, uint32_t *__restrict__ map) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = uint64_t(gridDim.x) * 4;
    for (uint64_t si = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); si < n; si += nwaves) {
        const uint64_t ub = seg[si].unit_begin, len = seg[si].len;
        const uint64_t nu = (len / ubpc * ubpc + kRoundBytes - 1) / kRoundBytes;
        for (uint64_t t = lane; t < nu; t += 64) map[ub + t] = uint32_t(si);
    }
}

// the map of d_seg[0..n) at unit chunk size ubpc into unit_seg: a segment per wave, 4 waves per workgroup
hipError_t launch_unit_map(const LaunchEnv &env, const DevSegment *d_seg, size_t n, uint32_t ubpc, uint32_t *unit_seg) {
    hipLaunchKernelGGL(crc32c_unit_map_kernel, dim3(clamped_grid((n + 3) / 4, 2048)), dim3(256), 0, env.stream, d_seg,
                       uint32_t(n), ubpc, unit_seg);
    return hipGetLastError();
}

// the descriptors' H2D copy: in-stream, or for long lists on the side stream so it runs under the previous
// launch (1 GiB of 32-64 KiB packets: 872 KB of descriptors); *staged is set: h is read asynchronously
hipError_t copy_descs(const LaunchEnv &env, void *d, const void *h, size_t bytes, bool *staged) {
    const DescCopy *dc = env.desc_copy;
    const bool side = dc && dc->side && dc->copied && bytes >= kSideCopyMinBytes;
    hipError_t e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, side ? dc->side : env.stream);
    if (side && e == hipSuccess) e = hipEventRecord(dc->copied, dc->side);
    if (side && e == hipSuccess) e = hipStreamWaitEvent(env.stream, dc->copied, 0);
    if (e == hipSuccess && staged) *staged = true;
    return e;
}

// the segments' short last chunks (len % bpc bytes), one thread each
template <bool VERIFY>
__global__ __launch_bounds__(kBlockThreads) void crc32c_segment_tails_kernel(const DevSegment *__restrict__ seg,
                                                                             uint32_t n, uint32_t bpc,
                                                                             int check_short_tail,
                                                                             unsigned long long *result,
                                                                             const uint32_t *__restrict__ g_tab) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsBytes / 4];
    fill_tables(lds, g_tab);
    lds_barrier();
    const Lut t(lds);
    for (uint64_t i = uint64_t(blockIdx.x) * kBlockThreads + threadIdx.x; i < n;
         i += uint64_t(gridDim.x) * kBlockThreads) {
        const DevSegment sd = seg[i];
        const uint32_t tail = uint32_t(sd.len % bpc);
        if (!tail) continue;
        const uint64_t c = sd.len / bpc;
        const uint32_t v = ~crc_run_any(t, 0xFFFFFFFFu, sd.data + c * bpc, tail);
        const bool al = (reinterpret_cast<uintptr_t>(sd.crc) & 3u) == 0;
        if constexpr (VERIFY) {
            if (check_short_tail && load_be32(sd.crc + 4 * c, al) != v)
                atomicMax(result, ~(unsigned long long)(sd.key_base + c));
        } else {
            store_be32(sd.crc + 4 * c, v, al);
        }
    }
}

// kSegmentPieces: h_stage[0..n) planned at 4096-byte units (unit_begin = the segment's first piece); the
// descriptors go to d_stage (always: the combine and the tails read them), *staged is set
hipError_t launch_segment_pieces(const LaunchEnv &env, const BatchPlan &p, DevSegment *h_stage, DevSegment *d_stage,
                                 size_t n, uint32_t bpc, bool verify, int check_short_tail,
                                 unsigned long long *result, bool *staged) {
    PieceScratch *ps = env.pieces;
    unsigned b = 0;
    // the piece words, then (long lists) the unit -> segment map
    const bool map = n > kUnitMapMinSegments && p.pieces_total;
    if (hipError_t e = piece_buffer(ps, (p.pieces_total ? p.pieces_total : 1) * (map ? 8 : 4), env.stream, &b);
        e != hipSuccess)
        return e;
    hipError_t e = copy_descs(env, d_stage, h_stage, n * sizeof(DevSegment), staged);
    if (e != hipSuccess) return e;
    uint32_t *unit_seg = nullptr;
    if (map) {
        unit_seg = reinterpret_cast<uint32_t *>(ps->d[b] + p.pieces_total * 4);
        if ((e = launch_unit_map(env, d_stage, n, uint32_t(kRoundBytes), unit_seg)) != hipSuccess) return e;
    }
    if (p.pieces_total) {
        e = launch_segments(env, d_stage, uint32_t(n), p.pieces_total, 0, kRoundBytes, false, 1, nullptr, nullptr, 0,
                            ps->d[b], unit_seg);
        if (e != hipSuccess) return e;
    }
    if (p.max_chunks) {  // 4 waves per workgroup, a segment per wave
        e = launch_vc(verify, crc32c_combine_segment_pieces_kernel<true>, crc32c_combine_segment_pieces_kernel<false>,
                      clamped_grid((n + 3) / 4, 2048), 256, env.stream, d_stage, uint32_t(n), ps->d[b], bpc, env.fold,
                      result);
        if (e != hipSuccess) return e;
    }
    e = hipEventRecord(ps->used[b], env.stream);
    if (e != hipSuccess) return e;
    if (!p.any_tail) return hipSuccess;
    return launch_vc(verify, crc32c_segment_tails_kernel<true>, crc32c_segment_tails_kernel<false>,
                     clamped_grid((n + kBlockThreads - 1) / kBlockThreads, uint64_t(env.grid_cap)), kBlockThreads,
                     env.stream, d_stage, uint32_t(n), bpc, verify ? check_short_tail : 0, result, env.tables);
}

// kMappedSegments: the unit -> segment map in the piece scratch (4 B per 4 KiB unit), then the segmented kernel
hipError_t launch_mapped_segments(const LaunchEnv &env, const BatchPlan &p, const DevSegment *d_stage, size_t n,
                                  uint32_t bpc, bool verify, int check_short_tail, unsigned long long *result) {
    unsigned b = 0;
    if (hipError_t e = piece_buffer(env.pieces, p.units * 4, env.stream, &b); e != hipSuccess) return e;
    uint32_t *unit_seg = reinterpret_cast<uint32_t *>(env.pieces->d[b]);
    hipError_t e = launch_unit_map(env, d_stage, n, bpc, unit_seg);
    if (e == hipSuccess)
        e = launch_segments(env, d_stage, uint32_t(n), p.units, 0, bpc, verify, check_short_tail, result, nullptr, 0,
                            nullptr, unit_seg);
    if (e == hipSuccess) e = hipEventRecord(env.pieces->used[b], env.stream);
    return e;
}

}  // namespace

hipError_t launch_packet_batch(const LaunchEnv &env, const uint8_t *d_arena, const DevPacket *h_pk, size_t n,
                               uint32_t bpc, bool verify, int check_short_tail, unsigned long long *result,
                               DevSegment *h_stage, DevSegment *d_stage, uint64_t arena_len, size_t *bad_index,
                               bool overlap_previous, bool *staged) {
    if (staged) *staged = false;
    if (n == 0) return hipSuccess;
    const BatchPlan p = plan_packet_batch(reinterpret_cast<uintptr_t>(d_arena), h_pk, n, bpc,
                                          bad_index ? &arena_len : nullptr, env.pieces != nullptr, g_variant, h_stage);
    const uint32_t nseg = uint32_t(n);
    switch (p.route) {
    case Route::kOutOfBounds:
        *bad_index = p.bad_index;
        return hipErrorInvalidValue;
    case Route::kPitchStream: {
        ChunkLaunch a = pitch_stream_launch(p.stream, d_arena + h_pk[0].data_off,
                                            const_cast<uint8_t *>(d_arena) + h_pk[0].crc_off, bpc, check_short_tail,
                                            result);
        a.overlap_previous = overlap_previous && verify;
        return launch_packet_stream(env, a, verify);
    }
    case Route::kStridedSegments: {
        const DevSegment ends[2] = {
            DevSegment{d_arena + h_pk[0].data_off, const_cast<uint8_t *>(d_arena) + h_pk[0].crc_off,
                       h_pk[0].data_len, 0, 0},
            DevSegment{d_arena + h_pk[n - 1].data_off, const_cast<uint8_t *>(d_arena) + h_pk[n - 1].crc_off,
                       h_pk[n - 1].data_len, (n - 1) * p.uniform, uint64_t(n - 1) << 32}};
        return launch_segments(env, nullptr, nseg, p.units, p.uniform, bpc, verify, check_short_tail, result, ends,
                               p.stream.pitch);
    }
    case Route::kSegmentPieces:
        return launch_segment_pieces(env, p, h_stage, d_stage, n, bpc, verify, check_short_tail, result, staged);
    case Route::kInlineSegments:
        return launch_segments(env, nullptr, nseg, p.units, p.uniform, bpc, verify, check_short_tail, result, h_stage);
    case Route::kMappedSegments:
    case Route::kStagedSegments:
        if (hipError_t e = copy_descs(env, d_stage, h_stage, n * sizeof(DevSegment), staged); e != hipSuccess) return e;
        if (p.route == Route::kMappedSegments)
            return launch_mapped_segments(env, p, d_stage, n, bpc, verify, check_short_tail, result);
        return launch_segments(env, d_stage, nseg, p.units, p.uniform, bpc, verify, check_short_tail, result);
    case Route::kPackets:
        if (hipError_t e = copy_descs(env, d_stage, h_stage, n * sizeof(DevPacket), staged); e != hipSuccess) return e;
        return launch_packets(env, d_arena, reinterpret_cast<const DevPacket *>(d_stage), n, bpc, verify,
                              check_short_tail, result);
    }
    return hipErrorInvalidValue;
}

}  // namespace hdfs3crc
