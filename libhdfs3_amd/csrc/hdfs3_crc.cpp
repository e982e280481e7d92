// C-ABI of the MI355X CRC32C engine (include/hdfs3_crc.h): the entry points that launch. The ctx itself
// is ctx.cpp's, the pool of contexts ctx_pool.cpp's; errors follow ctx.cpp's convention (a negative
// errno code and hdfs3_crc_last_error).
#include "hdfs3_crc.h"
#include "md5.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstring>
#include <vector>

#include "copy_pool.h"
#include "crc32c_kernels.h"
#include "crc32c_tables.h"
#include "crc_compose.h"
#include "ctx.h"
#include "numa.h"

namespace hdfs3crc {
uint32_t host_update(uint32_t state, const void *p, size_t n);
}

using namespace hdfs3crc;

namespace {

int check_args(hdfs3_crc_ctx *ctx, uint32_t bpc) {
    if (!ctx) return fail(-EINVAL, "null hdfs3_crc_ctx");
    // any bytesPerChecksum > 0, as RemoteBlockReader::checkResponse accepts from a datanode
    // (RemoteBlockReader.cpp:150-156): sizes the whole-round kernels do not take (not 512..4096
    // or unaligned buffers) run on the byte-granular chunk-per-lane kernel
    if (bpc == 0) return fail(-EINVAL, "bytes per checksum must be positive");
    return 0;
}

int grow_slot(Slot &s, size_t data_bytes, size_t crc_bytes) {
    HIP_TRY(s.data.grow(data_bytes, pinned_host_flags()));
    HIP_TRY(s.crc.grow(crc_bytes, pinned_host_flags()));
    return 0;
}

int finish_pending(Slot &s) {
    if (s.pending_out) {
        HIP_TRY(hipEventSynchronize(s.done));
        std::memcpy(s.pending_out, s.crc.h, s.pending_bytes);
        s.pending_out = nullptr;
        s.pending_bytes = 0;
    }
    return 0;
}

int launch(hdfs3_crc_ctx *ctx, const ChunkLaunch &a, bool verify) {
    HIP_TRY(launch_chunks(launch_env(ctx), a, verify));
    ++ctx->launches;
    return 0;
}

// the block checksums compute their chunk words in pieces of this many chunks
constexpr uint64_t kMd5PieceChunks = 1ull << 20;  // 4 MiB of CRC words per piece

// the compute launch over piece i of [d_data, d_data + len): its words go to d_words
int launch_piece(hdfs3_crc_ctx *ctx, const void *d_data, size_t len, uint32_t bpc, uint64_t i, uint8_t *d_words) {
    const uint64_t off = i * kMd5PieceChunks * bpc;
    const uint64_t n = std::min<uint64_t>(kMd5PieceChunks * bpc, uint64_t(len) - off);
    const uint8_t *piece = static_cast<const uint8_t *>(d_data) + off;
    return launch(ctx, contiguous_launch(piece, n, bpc, nullptr, d_words, nullptr, 0, 0, false), false);
}

// true when [p, p+len) is page-locked host memory the DMA engine can read directly
// (hdfs3_host_malloc_pinned, hipHostRegister); pageable memory is staged instead
bool is_pinned_host(const void *p) {
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable pointers report an error; clear it
        return false;
    }
    return attr.type == hipMemoryTypeHost && attr.hostPointer != nullptr;
}

// The blocking verify calls' verdict: the ctx's result word is cleared before their launches ...
int clear_verdict(hdfs3_crc_ctx *ctx) {
    HIP_TRY(hipMemsetAsync(ctx->result.d, 0, sizeof(unsigned long long), ctx->stream));
    return 0;
}

// ... and read back behind them: the stream is drained, *raw is the word as the kernels left it
int read_verdict(hdfs3_crc_ctx *ctx, unsigned long long *raw) {
    HIP_TRY(hipMemcpyAsync(ctx->result.h, ctx->result.d, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *raw = *ctx->result.h;
    return 0;
}

// Host-buffer pipeline shared by compute and verify: segments of whole chunks
// alternate between two pinned/device slots, so the CPU copy into pinned memory
// of segment i+1 overlaps the DMA and kernel of segment i.
int host_pipeline_impl(hdfs3_crc_ctx *ctx, const void *data, size_t len, uint32_t bpc,
                       const void *crc_in, void *crc_out, int check_short_tail,
                       int64_t *first_bad) {
    const bool verify = crc_in != nullptr;
    const size_t seg = (kSegmentBytes / bpc > 0 ? kSegmentBytes / bpc : 1) * size_t(bpc);
    const size_t seg_crc = (seg / bpc) * 4;
    if (verify)
        if (int rc = clear_verdict(ctx)) return rc;
    const uint8_t *src = static_cast<const uint8_t *>(data);
    const bool direct = is_pinned_host(data);  // skip the staging copy for pinned callers
    size_t off = 0;
    for (int k = 0; off < len; ++k) {
        Slot &s = ctx->slot[k & 1];
        const size_t n = len - off < seg ? len - off : seg;
        const size_t nc = (n + bpc - 1) / bpc;
        const size_t chunk0 = off / bpc;
        if (s.done) HIP_TRY(hipEventSynchronize(s.done));
        if (int rc = finish_pending(s)) return rc;
        if (int rc = grow_slot(s, seg, seg_crc)) return rc;
        if (!direct) CopyPool::get().copy(s.data.h, src + off, n);  // pageable: staged, split over the pool
        HIP_TRY(hipMemcpyAsync(s.data.d, direct ? src + off : s.data.h, n, hipMemcpyHostToDevice, ctx->stream));
        if (verify) {
            std::memcpy(s.crc.h, static_cast<const uint8_t *>(crc_in) + 4 * chunk0, 4 * nc);
            HIP_TRY(hipMemcpyAsync(s.crc.d, s.crc.h, 4 * nc, hipMemcpyHostToDevice, ctx->stream));
        }
        const ChunkLaunch a = contiguous_launch(s.data.d, n, bpc, verify ? s.crc.d : nullptr, verify ? nullptr : s.crc.d,
                                                verify ? ctx->result.d : nullptr, chunk0, check_short_tail, false);
        if (int rc = launch(ctx, a, verify)) return rc;
        if (!verify) {
            HIP_TRY(hipMemcpyAsync(s.crc.h, s.crc.d, 4 * nc, hipMemcpyDeviceToHost, ctx->stream));
            s.pending_out = static_cast<uint8_t *>(crc_out) + 4 * chunk0;
            s.pending_bytes = 4 * nc;
        }
        if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s.done, ctx->stream));
        off += n;
    }
    unsigned long long raw = 0;
    if (verify) {
        if (int rc = read_verdict(ctx, &raw)) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    for (Slot &s : ctx->slot)
        if (int rc = finish_pending(s)) return rc;
    if (verify && first_bad) *first_bad = hdfs3_crc_decode_result(raw);
    return 0;
}

int host_pipeline(hdfs3_crc_ctx *ctx, const void *data, size_t len, uint32_t bpc,
                  const void *crc_in, void *crc_out, int check_short_tail,
                  int64_t *first_bad) {
    const int rc = host_pipeline_impl(ctx, data, len, bpc, crc_in, crc_out, check_short_tail, first_bad);
    if (rc != 0) {
        // a failed call must not leave CRC words queued for a caller buffer it no longer
        // owns: the next call would copy them out in finish_pending
        (void)hipStreamSynchronize(ctx->stream);
        for (Slot &sl : ctx->slot) sl.pending_out = nullptr;
    }
    return rc;
}

static_assert(sizeof(hdfs3_pkt_desc) == sizeof(DevPacket) && offsetof(hdfs3_pkt_desc, data_off) == offsetof(DevPacket, data_off) &&
                  offsetof(hdfs3_pkt_desc, crc_off) == offsetof(DevPacket, crc_off) &&
                  offsetof(hdfs3_pkt_desc, data_len) == offsetof(DevPacket, data_len),
              "the packets API hands descriptors to the kernels unconverted");

int stage_segments(hdfs3_crc_ctx *ctx, size_t n, hdfs3_crc_ctx::SegStage **out);

// One launch over n packets, nothing waited for: a single host pass over pk[] (bounds, layout
// detection, descriptors into a staging slot of the ctx's ring, which is reused only after its
// launch ran). Constant-pitch streams of whole-round packets take the wave kernel's pitch mode
// with no descriptor copy at all.
int packets_async(hdfs3_crc_ctx *ctx, const uint8_t *d_arena, size_t arena_len, const hdfs3_pkt_desc *pk, size_t n,
                  uint32_t bpc, bool verify, int check_short_tail, unsigned long long *d_result, bool overlap) {
    // the result key is (packet << 32 | chunk)
    if (n >= (size_t(1) << 31)) return fail(-EINVAL, "too many packets in one batch");
    hdfs3_crc_ctx::SegStage *st = nullptr;
    if (int rc = stage_segments(ctx, n, &st)) return rc;
    // hdfs3_pkt_desc and DevPacket share one layout (asserted above): no conversion copy
    const DevPacket *hp = reinterpret_cast<const DevPacket *>(pk);
    size_t bad = 0;
    bool staged = false;
    // a long list's descriptors copy on the ctx's side stream, under the launch before (the slot's
    // host and device halves are free: stage_segments waited for its last launch)
    DescCopy dc;
    LaunchEnv env = launch_env(ctx);
    if (n * sizeof(DevSegment) >= kSideCopyMinBytes) {
        if (!ctx->desc_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->desc_stream, hipStreamNonBlocking));
        if (!st->copied) HIP_TRY(hipEventCreateWithFlags(&st->copied, hipEventDisableTiming));
        dc.side = ctx->desc_stream;
        dc.copied = st->copied;
        env.desc_copy = &dc;
    }
    const hipError_t e = launch_packet_batch(env, d_arena, hp, n, bpc, verify, check_short_tail, d_result, st->seg.h, st->seg.d,
                                             arena_len, &bad, overlap, &staged);
    if (e == hipErrorInvalidValue) return fail(-EINVAL, "packet %zu lies outside the %zu-byte arena", bad, arena_len);
    HIP_TRY(e);
    ++ctx->launches;
    // the launch copied its descriptors out of st->seg.h asynchronously (the segmented kernel's array, the
    // chunk-per-lane kernel's DevPackets): the slot is reused only after that copy ran (round 5:
    // unarmed, a fifth async batch could overwrite a queued copy's source). A launch whose arguments
    // carried everything (the pitch walk: the writer's and the wire-layout batches) records nothing:
    // an event between barriered launches costs a marker packet, ~3 us of idle GPU (round 6)
    if (staged) {
        HIP_TRY(hipEventRecord(st->done, ctx->stream));
        st->armed = true;
    }
    return 0;
}

int packets_common(hdfs3_crc_ctx *ctx, const uint8_t *d_arena, size_t arena_len,
                   const hdfs3_pkt_desc *pk, size_t n, uint32_t bpc, bool verify,
                   int check_short_tail, int64_t *bad_packet, int64_t *bad_chunk) {
    if (verify)
        if (int rc = clear_verdict(ctx)) return rc;
    if (int rc = packets_async(ctx, d_arena, arena_len, pk, n, bpc, verify, check_short_tail, ctx->result.d, false))
        return rc;
    if (!verify) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return 0;
    }
    unsigned long long raw = 0;
    if (int rc = read_verdict(ctx, &raw)) return rc;
    split_result_key(raw, bad_packet, bad_chunk);
    return 0;
}

// hdfs3_pkt_stream: O(1) host work when the wave kernel's pitch mode takes the stream, else
// the descriptors are generated (once) and go through packets_async
int packet_stream_async(hdfs3_crc_ctx *ctx, const uint8_t *d_arena, size_t arena_len, const hdfs3_pkt_stream *ps,
                        uint32_t bpc, bool verify, int check_short_tail, unsigned long long *d_result, bool overlap) {
    if (ps->n == 0) return 0;
    if (ps->n >= (uint64_t(1) << 31)) return fail(-EINVAL, "too many packets in one stream");
    if (ps->last_len > ps->data_len) return fail(-EINVAL, "last_len above data_len");
    // bounds: the first and the last packet delimit the stream (pitch >= 0, offsets grow)
    const uint64_t last = ps->n - 1;
    const uint64_t lchunks = (uint64_t(ps->last_len) + bpc - 1) / bpc, chunks = (uint64_t(ps->data_len) + bpc - 1) / bpc;
    const unsigned __int128 ld = (unsigned __int128)ps->data_off + (unsigned __int128)last * ps->pitch;
    const unsigned __int128 lc = (unsigned __int128)ps->crc_off + (unsigned __int128)last * ps->pitch;
    if (ps->data_off + uint64_t(ps->n > 1 ? ps->data_len : ps->last_len) > arena_len || ld + ps->last_len > arena_len ||
        ps->crc_off + 4 * (ps->n > 1 ? chunks : lchunks) > arena_len || lc + 4 * lchunks > arena_len ||
        (ps->n > 1 && ps->pitch == 0))
        return fail(-EINVAL, "the packet stream does not fit the %zu-byte arena", arena_len);
    PitchStream s;
    if (plan_packet_stream(ps->data_len, ps->last_len, ps->n, bpc, d_arena + ps->data_off, d_arena + ps->crc_off,
                           ps->pitch, /*have_pieces=*/true, g_variant, &s)) {
        ChunkLaunch a = pitch_stream_launch(s, d_arena + ps->data_off, const_cast<uint8_t *>(d_arena) + ps->crc_off, bpc,
                                            check_short_tail, d_result);
        a.overlap_previous = overlap && verify;
        HIP_TRY(launch_packet_stream(launch_env(ctx), a, verify));
        ++ctx->launches;
        return 0;
    }
    std::vector<hdfs3_pkt_desc> pk(ps->n);
    for (uint64_t i = 0; i < ps->n; ++i)
        pk[i] = hdfs3_pkt_desc{ps->data_off + i * ps->pitch, ps->crc_off + i * ps->pitch,
                               i == last ? ps->last_len : ps->data_len, 0};
    return packets_async(ctx, d_arena, arena_len, pk.data(), pk.size(), bpc, verify, check_short_tail, d_result, false);
}

// a descriptor staging slot of the blocks API, reusable once its previous launch ran
int stage_segments(hdfs3_crc_ctx *ctx, size_t n, hdfs3_crc_ctx::SegStage **out) {
    hdfs3_crc_ctx::SegStage &st = ctx->seg_ring[ctx->seg_next++ & 3u];
    if (st.armed) HIP_TRY(hipEventSynchronize(st.done));
    st.armed = false;
    HIP_TRY(st.seg.grow(n * sizeof(DevSegment), hipHostMallocDefault));
    if (!st.done) HIP_TRY(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    *out = &st;
    return 0;
}

int blocks_common(hdfs3_crc_ctx *ctx, const hdfs3_dev_block *blocks, size_t n, uint32_t bpc, bool verify,
                  int check_short_tail, unsigned long long *d_result) {
    if (n > (size_t(1) << 31)) return fail(-EINVAL, "too many blocks in one batch");
    for (size_t i = 0; i < n; ++i) {
        if (blocks[i].len && (!blocks[i].data || !blocks[i].crc_be)) return fail(-EINVAL, "block %zu: null buffer", i);
        if ((blocks[i].len + bpc - 1) / bpc >= (uint64_t(1) << 32))
            return fail(-EINVAL, "block %zu: 2^32 chunks or more", i);
    }
    hdfs3_crc_ctx::SegStage *st = nullptr;
    if (int rc = stage_segments(ctx, n, &st)) return rc;
    for (size_t i = 0; i < n; ++i)
        st->seg.h[i] = DevSegment{static_cast<const uint8_t *>(blocks[i].data), static_cast<uint8_t *>(blocks[i].crc_be),
                              blocks[i].len, 0, uint64_t(i) << 32};
    // blocks of one 2-D tensor (constant data and word strides, equal whole-round blocks): the
    // wave kernel walks them directly (pitch mode); everything else: the segmented kernel
    const LaunchEnv env = launch_env(ctx);
    PitchStream s;
    if (plan_strided_blocks(st->seg.h, n, bpc, g_variant, &s)) {
        HIP_TRY(launch_packet_stream(
            env, pitch_stream_launch(s, st->seg.h[0].data, st->seg.h[0].crc, bpc, check_short_tail, d_result), verify));
        ++ctx->launches;
    } else if (segments_fast(st->seg.h, n, bpc)) {
        uint64_t uniform = 0;
        const uint64_t units = plan_segments(st->seg.h, n, bpc, &uniform);
        if (n <= kInlineSegments) {  // descriptors in the kernel arguments: no copy first
            HIP_TRY(launch_segments(env, nullptr, uint32_t(n), units, uniform, bpc, verify, check_short_tail, d_result,
                                    st->seg.h));
        } else {
            HIP_TRY(hipMemcpyAsync(st->seg.d, st->seg.h, n * sizeof(DevSegment), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(launch_segments(env, st->seg.d, uint32_t(n), units, uniform, bpc, verify, check_short_tail, d_result));
            // the pinned staging is read by the copy: reusable once it ran. The other paths read
            // it on the host only (the launch's arguments carry what the kernel needs), and an
            // event between launches costs a marker packet (~4 us of idle between barriered
            // launches in the kernel trace of the batch pass, profiles/r03/prof/)
            HIP_TRY(hipEventRecord(st->done, ctx->stream));
            st->armed = true;
        }
        ++ctx->launches;
    } else {  // other chunk sizes or unaligned buffers: one launch per block, same keys
        for (size_t i = 0; i < n; ++i) {
            if (!blocks[i].len) continue;
            const DevSegment &b = st->seg.h[i];
            const ChunkLaunch a =
                contiguous_launch(b.data, b.len, bpc, b.crc, b.crc, d_result, b.key_base, check_short_tail, false);
            if (int rc = launch(ctx, a, verify)) return rc;
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int hdfs3_crc32c_verify_blocks_dev_async(hdfs3_crc_ctx *ctx, const hdfs3_dev_block *blocks, size_t n,
                                         uint32_t bpc, int check_short_tail, uint64_t *d_result) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (n == 0) return 0;
    if (!blocks || !d_result) return fail(-EINVAL, "null argument");
    DeviceGuard g(ctx->device);
    return blocks_common(ctx, blocks, n, bpc, true, check_short_tail, reinterpret_cast<unsigned long long *>(d_result));
}

int hdfs3_crc32c_verify_blocks_dev(hdfs3_crc_ctx *ctx, const hdfs3_dev_block *blocks, size_t n, uint32_t bpc,
                                   int check_short_tail, int64_t *bad_block, int64_t *bad_chunk) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (bad_block) *bad_block = -1;
    if (bad_chunk) *bad_chunk = -1;
    if (n == 0) return 0;
    if (!blocks) return fail(-EINVAL, "null argument");
    DeviceGuard g(ctx->device);
    if (int rc = clear_verdict(ctx)) return rc;
    if (int rc = blocks_common(ctx, blocks, n, bpc, true, check_short_tail, ctx->result.d)) return rc;
    unsigned long long raw = 0;
    if (int rc = read_verdict(ctx, &raw)) return rc;
    split_result_key(raw, bad_block, bad_chunk);
    return 0;
}

int hdfs3_crc32c_compute_blocks_dev(hdfs3_crc_ctx *ctx, const hdfs3_dev_block *blocks, size_t n, uint32_t bpc) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (n == 0) return 0;
    if (!blocks) return fail(-EINVAL, "null argument");
    DeviceGuard g(ctx->device);
    return blocks_common(ctx, blocks, n, bpc, false, 0, nullptr);
}

int hdfs3_crc_abi_version(void) { return HDFS3_CRC_ABI_VERSION; }

int hdfs3_device_count(int *count) {
    if (!count) return fail(-EINVAL, "null count");
    HIP_TRY(hipGetDeviceCount(count));
    return 0;
}

}  // extern "C"

namespace hdfs3crc {
int gather_dev(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const void *d_src, size_t src_len, const CopyRange *r,
               size_t n, unsigned *launched) {
    const size_t bad = gather_first_bad(r, n, src_len, dst_len);
    if (bad != n)
        return fail(-EINVAL, "range %zu lies outside the %zu-byte source or the %zu-byte destination", bad, src_len,
                    dst_len);
    GatherLaunch g;
    for (size_t pos = 0; pos < n;) {
        pos = plan_gather_launch(reinterpret_cast<uintptr_t>(d_dst), r, n, pos, &g);
        if (g.n == 0) continue;  // nothing but empty ranges
        HIP_TRY(launch_gather(ctx->stream, d_dst, dst_len, d_src, src_len, g));
        ++ctx->launches;
        if (launched) ++*launched;
    }
    return 0;
}

int gather_sources_dev(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const CopyRange *r, size_t n, unsigned *launched) {
    const size_t bad = gather_sources_first_bad(r, n, dst_len);
    if (bad != n)
        return fail(-EINVAL, "range %zu lies outside the %zu-byte destination or its source wraps", bad, dst_len);
    for (size_t i = 0; i < n; ++i)
        if (r[i].len && (!d_dst || !r[i].src_off)) return fail(-EINVAL, "range %zu: null buffer", i);
    GatherLaunch g;
    for (size_t pos = 0; pos < n;) {
        pos = plan_gather_launch(reinterpret_cast<uintptr_t>(d_dst), r, n, pos, &g);
        if (g.n == 0) continue;  // nothing but empty ranges
        HIP_TRY(launch_gather_sources(ctx->stream, d_dst, dst_len, g));
        ++ctx->launches;
        if (launched) ++*launched;
    }
    return 0;
}

int deliver_dev(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const void *d_src, size_t src_len, const CopyRange *r,
                size_t n, const DeliverGuard &guard, unsigned *launched) {
    if (!guard.result) return fail(-EINVAL, "null result word");
    if (guard.granule == 0 || guard.bpc == 0) return fail(-EINVAL, "granule and bpc must be at least 1");
    if (guard.gate_out && (guard.gate_out == guard.gate_in || guard.gate_out == guard.result))
        return fail(-EINVAL, "gate_out aliases a word the same launch reads");
    const size_t bad = gather_first_bad(r, n, src_len, dst_len);
    if (bad != n)
        return fail(-EINVAL, "range %zu lies outside the %zu-byte source or the %zu-byte destination", bad, src_len,
                    dst_len);
    GatherLaunch g;
    bool any = false;
    for (size_t pos = 0; pos < n;) {
        pos = plan_gather_launch(reinterpret_cast<uintptr_t>(d_dst), r, n, pos, &g);
        if (g.n == 0) continue;  // nothing but empty ranges
        HIP_TRY(launch_deliver(ctx->stream, d_dst, dst_len, d_src, src_len, g, guard));
        any = true;
        ++ctx->launches;
        if (launched) ++*launched;
    }
    if (!any && guard.gate_out) {  // nothing to copy: the chain word is still passed on
        g.n = 0;
        HIP_TRY(launch_deliver(ctx->stream, d_dst, dst_len, d_src, src_len, g, guard));
        ++ctx->launches;
        if (launched) ++*launched;
    }
    return 0;
}
}  // namespace hdfs3crc

extern "C" {

int64_t hdfs3_crc_decode_result(uint64_t r) { return r ? int64_t(~r) : -1; }

int hdfs3_crc32c_compute(hdfs3_crc_ctx *ctx, const void *data, size_t len, uint32_t bpc,
                         void *crc_be_out) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (len == 0) return 0;
    if (!data || !crc_be_out) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return host_pipeline(ctx, data, len, bpc, nullptr, crc_be_out, 0, nullptr);
}

int hdfs3_crc32c_verify(hdfs3_crc_ctx *ctx, const void *data, size_t len, uint32_t bpc,
                        const void *crc_be, int check_short_tail, int64_t *first_bad_chunk) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (first_bad_chunk) *first_bad_chunk = -1;
    if (len == 0) return 0;
    if (!data || !crc_be) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return host_pipeline(ctx, data, len, bpc, crc_be, nullptr, check_short_tail, first_bad_chunk);
}

int hdfs3_crc32c_compute_dev(hdfs3_crc_ctx *ctx, const void *d_data, size_t len, uint32_t bpc,
                             void *d_crc_be_out) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (len == 0) return 0;
    if (!d_data || !d_crc_be_out) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return launch(ctx, contiguous_launch(d_data, len, bpc, nullptr, d_crc_be_out, nullptr, 0, 0, false), false);
}

int hdfs3_crc32c_compute_dev_async_ex(hdfs3_crc_ctx *ctx, const void *d_data, size_t len, uint32_t bpc,
                                      void *d_crc_be_out, uint32_t flags) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (flags & ~HDFS3_LAUNCH_OVERLAP_PREVIOUS) return fail(-EINVAL, "unknown launch flags 0x%x", flags);
    if (len == 0) return 0;
    if (!d_data || !d_crc_be_out) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    const bool overlap = (flags & HDFS3_LAUNCH_OVERLAP_PREVIOUS) != 0;
    return launch(ctx, contiguous_launch(d_data, len, bpc, nullptr, d_crc_be_out, nullptr, 0, 0, overlap), false);
}

int hdfs3_crc32c_verify_dev_async(hdfs3_crc_ctx *ctx, const void *d_data, size_t len,
                                  uint32_t bpc, const void *d_crc_be, int check_short_tail,
                                  uint64_t *d_result) {
    return hdfs3_crc32c_verify_dev_async_ex(ctx, d_data, len, bpc, d_crc_be, check_short_tail, d_result, 0);
}

int hdfs3_crc32c_verify_dev_async_ex(hdfs3_crc_ctx *ctx, const void *d_data, size_t len,
                                     uint32_t bpc, const void *d_crc_be, int check_short_tail,
                                     uint64_t *d_result, uint32_t flags) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (flags & ~HDFS3_LAUNCH_OVERLAP_PREVIOUS) return fail(-EINVAL, "unknown launch flags 0x%x", flags);
    if (len == 0) return 0;
    if (!d_data || !d_crc_be || !d_result) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    const bool overlap = (flags & HDFS3_LAUNCH_OVERLAP_PREVIOUS) != 0;
    return launch(ctx,
                  contiguous_launch(d_data, len, bpc, d_crc_be, nullptr, reinterpret_cast<unsigned long long *>(d_result), 0,
                                    check_short_tail, overlap),
                  true);
}

int hdfs3_crc32c_verify_dev(hdfs3_crc_ctx *ctx, const void *d_data, size_t len, uint32_t bpc,
                            const void *d_crc_be, int check_short_tail, int64_t *first_bad_chunk) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (first_bad_chunk) *first_bad_chunk = -1;
    if (len == 0) return 0;
    DeviceGuard g(ctx->device);
    if (int rc = clear_verdict(ctx)) return rc;
    if (int rc = hdfs3_crc32c_verify_dev_async(ctx, d_data, len, bpc, d_crc_be, check_short_tail,
                                               reinterpret_cast<uint64_t *>(ctx->result.d)))
        return rc;
    unsigned long long raw = 0;
    if (int rc = read_verdict(ctx, &raw)) return rc;
    if (first_bad_chunk) *first_bad_chunk = hdfs3_crc_decode_result(raw);
    return 0;
}

int hdfs3_crc32c_verify_packets(hdfs3_crc_ctx *ctx, const void *arena, size_t arena_len,
                                const hdfs3_pkt_desc *pk, size_t n, uint32_t bpc,
                                int check_short_tail, int64_t *bad_packet, int64_t *bad_chunk) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (bad_packet) *bad_packet = -1;
    if (bad_chunk) *bad_chunk = -1;
    if (n == 0) return 0;
    if (!arena || !pk) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    Slot &s = ctx->slot[0];
    if (s.done) HIP_TRY(hipEventSynchronize(s.done));
    if (int rc = finish_pending(s)) return rc;
    if (int rc = grow_slot(s, arena_len, 4)) return rc;
    CopyPool::get().copy(s.data.h, arena, arena_len);  // split over the pool from 2 MiB up
    HIP_TRY(hipMemcpyAsync(s.data.d, s.data.h, arena_len, hipMemcpyHostToDevice, ctx->stream));
    return packets_common(ctx, s.data.d, arena_len, pk, n, bpc, true, check_short_tail, bad_packet,
                          bad_chunk);
}

int hdfs3_crc32c_verify_packets_dev(hdfs3_crc_ctx *ctx, const void *d_arena, size_t arena_len,
                                    const hdfs3_pkt_desc *pk, size_t n, uint32_t bpc,
                                    int check_short_tail, int64_t *bad_packet,
                                    int64_t *bad_chunk) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (bad_packet) *bad_packet = -1;
    if (bad_chunk) *bad_chunk = -1;
    if (n == 0) return 0;
    if (!d_arena || !pk) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return packets_common(ctx, static_cast<const uint8_t *>(d_arena), arena_len, pk, n, bpc, true,
                          check_short_tail, bad_packet, bad_chunk);
}

int hdfs3_crc32c_compute_packets_dev(hdfs3_crc_ctx *ctx, void *d_arena, size_t arena_len,
                                     const hdfs3_pkt_desc *pk, size_t n, uint32_t bpc) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (n == 0) return 0;
    if (!d_arena || !pk) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return packets_common(ctx, static_cast<const uint8_t *>(d_arena), arena_len, pk, n, bpc, false,
                          0, nullptr, nullptr);
}

int hdfs3_crc32c_verify_packets_dev_async(hdfs3_crc_ctx *ctx, const void *d_arena, size_t arena_len,
                                          const hdfs3_pkt_desc *pk, size_t n, uint32_t bpc, int check_short_tail,
                                          uint64_t *d_result) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (n == 0) return 0;
    if (!d_arena || !pk || !d_result) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return packets_async(ctx, static_cast<const uint8_t *>(d_arena), arena_len, pk, n, bpc, true, check_short_tail,
                         reinterpret_cast<unsigned long long *>(d_result), false);
}

int hdfs3_crc32c_compute_packets_dev_async(hdfs3_crc_ctx *ctx, void *d_arena, size_t arena_len,
                                           const hdfs3_pkt_desc *pk, size_t n, uint32_t bpc) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (n == 0) return 0;
    if (!d_arena || !pk) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return packets_async(ctx, static_cast<const uint8_t *>(d_arena), arena_len, pk, n, bpc, false, 0, nullptr, false);
}

static_assert(sizeof(hdfs3_copy_range) == sizeof(CopyRange) && offsetof(hdfs3_copy_range, src_off) == offsetof(CopyRange, src_off) &&
                  offsetof(hdfs3_copy_range, dst_off) == offsetof(CopyRange, dst_off) &&
                  offsetof(hdfs3_copy_range, len) == offsetof(CopyRange, len),
              "the gather hands its ranges to the planner unconverted");

int hdfs3_gather_dev_async(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const void *d_src, size_t src_len,
                           const hdfs3_copy_range *ranges, size_t n) {
    if (!ctx) return fail(-EINVAL, "null hdfs3_crc_ctx");
    if (n == 0) return 0;
    if (!d_dst || !d_src || !ranges) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return gather_dev(ctx, d_dst, dst_len, d_src, src_len, reinterpret_cast<const CopyRange *>(ranges), n);
}

static_assert(sizeof(hdfs3_src_range) == sizeof(CopyRange) && sizeof(const void *) == sizeof(uint64_t) &&
                  offsetof(hdfs3_src_range, d_src) == offsetof(CopyRange, src_off) &&
                  offsetof(hdfs3_src_range, dst_off) == offsetof(CopyRange, dst_off) &&
                  offsetof(hdfs3_src_range, len) == offsetof(CopyRange, len),
              "a source range is a copy range whose src_off is the source address");

int hdfs3_gather_sources_dev_async(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const hdfs3_src_range *ranges,
                                   size_t n) {
    if (!ctx) return fail(-EINVAL, "null hdfs3_crc_ctx");
    if (n == 0) return 0;
    if (!ranges) return fail(-EINVAL, "null ranges");
    DeviceGuard g(ctx->device);
    return gather_sources_dev(ctx, d_dst, dst_len, reinterpret_cast<const CopyRange *>(ranges), n);
}

int hdfs3_deliver_verified_dev_async(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const void *d_src, size_t src_len,
                                     const hdfs3_copy_range *ranges, size_t n, const hdfs3_deliver_guard *guard) {
    if (!ctx) return fail(-EINVAL, "null hdfs3_crc_ctx");
    if (!guard) return fail(-EINVAL, "null guard");
    if (n && (!d_dst || !d_src || !ranges)) return fail(-EINVAL, "null buffer");
    const DeliverGuard dg{guard->d_result, guard->d_gate_in, guard->d_gate_out, guard->data_off,
                          guard->chunk_base, guard->granule,   guard->bpc};
    DeviceGuard g(ctx->device);
    return deliver_dev(ctx, d_dst, dst_len, d_src, src_len, reinterpret_cast<const CopyRange *>(ranges), n, dg);
}

int hdfs3_crc32c_verify_packets_gather_dev(hdfs3_crc_ctx *ctx, const void *d_arena, size_t arena_len,
                                           const hdfs3_pkt_desc *pk, size_t n, uint32_t bpc, int check_short_tail,
                                           void *d_dst, size_t dst_len, uint64_t dst_off,
                                           int64_t *bad_packet, int64_t *bad_chunk, uint64_t *delivered) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (bad_packet) *bad_packet = -1;
    if (bad_chunk) *bad_chunk = -1;
    if (delivered) *delivered = 0;
    if (n == 0) return 0;
    if (!d_arena || !pk) return fail(-EINVAL, "null buffer");
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += pk[i].data_len;
    if (dst_off > dst_len || total > dst_len - dst_off)
        return fail(-EINVAL, "%llu bytes of packet data do not fit the %zu-byte destination at offset %llu",
                    (unsigned long long)total, dst_len, (unsigned long long)dst_off);
    if (total && !d_dst) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    int64_t bp = -1, bc = -1;
    if (int rc = packets_common(ctx, static_cast<const uint8_t *>(d_arena), arena_len, pk, n, bpc, true,
                                check_short_tail, &bp, &bc))
        return rc;
    if (bad_packet) *bad_packet = bp;
    if (bad_chunk) *bad_chunk = bc;
    // the verify result is in hand: only now is anything copied, and only what lies before the bad packet
    const size_t good = bp >= 0 ? size_t(bp) : n;
    std::vector<CopyRange> r(good);
    uint64_t placed = 0;
    for (size_t i = 0; i < good; ++i) {
        r[i] = CopyRange{pk[i].data_off, dst_off + placed, pk[i].data_len};
        placed += pk[i].data_len;
    }
    if (placed) {
        if (int rc = gather_dev(ctx, d_dst, dst_len, d_arena, arena_len, r.data(), good)) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (delivered) *delivered = placed;
    return 0;
}

int hdfs3_crc32c_verify_packet_stream_dev_async(hdfs3_crc_ctx *ctx, const void *d_arena, size_t arena_len,
                                                const hdfs3_pkt_stream *ps, uint32_t bpc, int check_short_tail,
                                                uint64_t *d_result, uint32_t flags) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (flags & ~HDFS3_LAUNCH_OVERLAP_PREVIOUS) return fail(-EINVAL, "unknown launch flags 0x%x", flags);
    if (!ps) return fail(-EINVAL, "null stream");
    if (ps->n == 0) return 0;
    if (!d_arena || !d_result) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return packet_stream_async(ctx, static_cast<const uint8_t *>(d_arena), arena_len, ps, bpc, true, check_short_tail,
                               reinterpret_cast<unsigned long long *>(d_result),
                               (flags & HDFS3_LAUNCH_OVERLAP_PREVIOUS) != 0);
}

int hdfs3_crc32c_compute_packet_stream_dev_async(hdfs3_crc_ctx *ctx, void *d_arena, size_t arena_len,
                                                 const hdfs3_pkt_stream *ps, uint32_t bpc) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (!ps) return fail(-EINVAL, "null stream");
    if (ps->n == 0) return 0;
    if (!d_arena) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    return packet_stream_async(ctx, static_cast<const uint8_t *>(d_arena), arena_len, ps, bpc, false, 0, nullptr,
                               false);
}

uint32_t hdfs3_crc32c_update_host(uint32_t state, const void *p, size_t len) {
    return len ? host_update(state, p, len) : state;
}

// Block checksum (include/hdfs3_crc.h): the CRC words come from the compute kernel in
// pieces of up to kMd5PieceChunks chunks, alternating between the two slots, so the host
// digests piece i while the GPU computes and copies out piece i+1.
int hdfs3_block_checksum_dev(hdfs3_crc_ctx *ctx, const void *d_data, size_t len, uint32_t bpc,
                             uint8_t *md5_out, uint64_t *crc_per_block) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (!md5_out || (len && !d_data)) return fail(-EINVAL, "null buffer");
    const uint64_t n = (uint64_t(len) + bpc - 1) / bpc;
    if (crc_per_block) *crc_per_block = n;
    Md5 md5;
    if (n) {
        DeviceGuard g(ctx->device);
        const uint64_t per = kMd5PieceChunks;
        const uint64_t pieces = (n + per - 1) / per;
        for (Slot &s : ctx->slot) {
            if (int rc = finish_pending(s)) return rc;
            if (int rc = grow_slot(s, 0, size_t(std::min(n, per)) * 4)) return rc;
            if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        }
        auto issue = [&](uint64_t i) -> int {
            Slot &s = ctx->slot[i & 1];
            if (int rc = launch_piece(ctx, d_data, len, bpc, i, s.crc.d)) return rc;
            HIP_TRY(hipMemcpyAsync(s.crc.h, s.crc.d, size_t(std::min(per, n - i * per)) * 4, hipMemcpyDeviceToHost,
                                   ctx->stream));
            HIP_TRY(hipEventRecord(s.done, ctx->stream));
            return 0;
        };
        if (int rc = issue(0)) return rc;
        for (uint64_t i = 0; i < pieces; ++i) {
            if (i + 1 < pieces)
                if (int rc = issue(i + 1)) return rc;
            Slot &s = ctx->slot[i & 1];
            HIP_TRY(hipEventSynchronize(s.done));
            md5.update(s.crc.h, size_t(std::min(per, n - i * per)) * 4);
        }
    }
    md5.finish(md5_out);
    return 0;
}

int hdfs3_block_checksum_crcs(const void *crc_be, uint64_t n_crcs, uint8_t *md5_out) {
    if (!md5_out || (n_crcs && !crc_be)) return fail(-EINVAL, "null buffer");
    Md5 md5;
    md5.update(crc_be, size_t(n_crcs) * 4);
    md5.finish(md5_out);
    return 0;
}

int hdfs3_file_checksum_md5md5crc(const uint8_t *block_md5s, size_t n_blocks, uint8_t *md5_out) {
    if (!md5_out || (n_blocks && !block_md5s)) return fail(-EINVAL, "null buffer");
    Md5 md5;
    md5.update(block_md5s, n_blocks * 16);
    md5.finish(md5_out);
    return 0;
}

}  // extern "C"

// Composite CRC (include/hdfs3_crc.h): the host forms are crc_compose.cpp's arithmetic, the device
// forms reduce the words with crc32c_compose.hip.
namespace {

int poly_of_type(int type, uint32_t *poly) {
    if (type != HDFS3_CHECKSUM_TYPE_CRC32C && type != HDFS3_CHECKSUM_TYPE_CRC32)
        return fail(-EINVAL, "checksum type %d has no CRC polynomial", type);
    *poly = type == HDFS3_CHECKSUM_TYPE_CRC32C ? kPolyReflected : kPolyCrc32;
    return 0;
}

int check_words(uint64_t n_crcs, uint32_t bpc, uint32_t last_len) {
    if (bpc == 0) return fail(-EINVAL, "bytes per checksum must be positive");
    if (n_crcs && (last_len == 0 || last_len > bpc))
        return fail(-EINVAL, "the last chunk holds %u bytes, not 1..%u", last_len, bpc);
    return 0;
}

// the reduction of n >= 1 device words into *d_out on the ctx's stream
int compose_words(hdfs3_crc_ctx *ctx, const void *d_crc_be, uint64_t n, uint32_t bpc, uint32_t last_len,
                  uint32_t *d_out) {
    if (n > kComposeMaxWords) return fail(-EINVAL, "%llu words in one composite", (unsigned long long)n);
    if (reinterpret_cast<uintptr_t>(d_crc_be) & 3u) return fail(-EINVAL, "the words are not 4-byte aligned");
    unsigned launched = 0;
    const hipError_t e = launch_compose_words(launch_env(ctx), &ctx->compose, static_cast<const uint8_t *>(d_crc_be), n,
                                              bpc, last_len, ctx->poly, d_out, &launched);
    ctx->launches += launched;
    HIP_TRY(e);
    return 0;
}

}  // namespace

extern "C" {

int hdfs3_crc_compose(int type, uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t *crc_out) {
    uint32_t poly = 0;
    if (int rc = poly_of_type(type, &poly)) return rc;
    if (!crc_out) return fail(-EINVAL, "null out");
    *crc_out = compose(crc_a, crc_b, len_b, poly);
    return 0;
}

int hdfs3_block_composite_crc_crcs(int type, const void *crc_be, uint64_t n_crcs, uint32_t bpc, uint32_t last_len,
                                   uint32_t *crc_out) {
    uint32_t poly = 0;
    if (int rc = poly_of_type(type, &poly)) return rc;
    if (int rc = check_words(n_crcs, bpc, last_len)) return rc;
    if (!crc_out || (n_crcs && !crc_be)) return fail(-EINVAL, "null buffer");
    *crc_out = composite_of_words(crc_be, n_crcs, bpc, last_len, poly);
    return 0;
}

int hdfs3_file_checksum_composite_crc(int type, const uint32_t *block_crcs, const uint64_t *block_lens,
                                      size_t n_blocks, uint32_t *crc_out) {
    uint32_t poly = 0;
    if (int rc = poly_of_type(type, &poly)) return rc;
    if (!crc_out || (n_blocks && (!block_crcs || !block_lens))) return fail(-EINVAL, "null buffer");
    *crc_out = composite_of_blocks(block_crcs, block_lens, n_blocks, poly);
    return 0;
}

int hdfs3_block_composite_crc_words_dev_async(hdfs3_crc_ctx *ctx, const void *d_crc_be, uint64_t n_crcs,
                                              uint32_t bpc, uint32_t last_len, uint32_t *d_out) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (int rc = check_words(n_crcs, bpc, last_len)) return rc;
    if (!d_out || (n_crcs && !d_crc_be)) return fail(-EINVAL, "null buffer");
    DeviceGuard g(ctx->device);
    if (n_crcs == 0) {  // the empty block
        HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(uint32_t), ctx->stream));
        return 0;
    }
    return compose_words(ctx, d_crc_be, n_crcs, bpc, last_len, d_out);
}

int hdfs3_block_composite_crc_dev(hdfs3_crc_ctx *ctx, const void *d_data, size_t len, uint32_t bpc,
                                  uint32_t *crc_out) {
    if (int rc = check_args(ctx, bpc)) return rc;
    if (!crc_out || (len && !d_data)) return fail(-EINVAL, "null buffer");
    *crc_out = 0;
    if (len == 0) return 0;
    const uint64_t n = (uint64_t(len) + bpc - 1) / bpc;
    if (n > kComposeMaxWords) return fail(-EINVAL, "%llu chunks in one composite", (unsigned long long)n);
    DeviceGuard g(ctx->device);
    ComposeScratch &cs = ctx->compose;
    HIP_TRY(grow_compose_buffer(&cs.words, &cs.words_cap, n * 4, ctx->stream));
    // the chunk words into the scratch, one compute launch per 4 Mi chunks as hdfs3_block_checksum_dev
    for (uint64_t i = 0; i * kMd5PieceChunks < n; ++i)
        if (int rc = launch_piece(ctx, d_data, len, bpc, i, cs.words + 4 * i * kMd5PieceChunks)) return rc;
    // the result word shares the verify calls' slot: a ctx serves one call at a time
    uint32_t *d_out = reinterpret_cast<uint32_t *>(ctx->result.d);
    const uint32_t last_len = uint32_t(uint64_t(len) - (n - 1) * bpc);
    if (int rc = compose_words(ctx, cs.words, n, bpc, last_len, d_out)) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->result.h, d_out, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *crc_out = *reinterpret_cast<const uint32_t *>(ctx->result.h);
    return 0;
}

}  // extern "C"
