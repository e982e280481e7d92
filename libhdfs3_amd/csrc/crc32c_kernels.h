// Internal launch interface of the gfx950 CRC32C kernels (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <tuple>
#include <type_traits>

#include "launch_plan.h"

namespace hdfs3crc {

// Workgroup geometry: the bank-replicated slice-table image takes 128 KiB of
// the CU's 160 KiB LDS, so one workgroup owns a CU; 1024 threads = 16 waves
// (4 per SIMD) keep the CU's memory pipe and LDS busy.
constexpr int kBlockThreads = 1024;

struct ChunkLaunch {
    const uint8_t *data;      // device pointer to the first chunk
    uint64_t len;             // bytes
    uint32_t bpc;             // bytes per checksum
    const uint8_t *crc_be;    // verify: stored BE32 words (device)
    uint8_t *out_be;          // compute: BE32 words written here (device)
    unsigned long long *result;  // verify: atomicMax(~first_bad) target (device)
    uint64_t chunk_base;      // added to chunk indices reported in *result
    int check_short_tail;     // 1: tail chunk checked (LocalBlockReader semantics)
    bool overlap_previous = false;  // HDFS3_LAUNCH_OVERLAP_PREVIOUS: AQL packet without barrier bit
    // Packet stream at a constant pitch (PitchWalk, launch_packet_stream): packet i's data at
    // data + i*pitch, its BE32 words at crc_be/out_be + i*pitch; every packet but the last holds
    // geom.pk_len bytes of whole chunks (geom.upp units), the last one last_len <= that many bytes.
    // len is unused; result keys are (packet << 32) | chunk.
    uint64_t pitch = 0;
    uint64_t npk = 0;
    PacketGeom geom;
    uint32_t last_len = 0;
    // pitch mode over independent blocks at constant strides (a [blocks, bytes] tensor and its
    // [blocks, words] tensor): the words' own pitch; 0 = `pitch` (the wire layout of packets)
    uint64_t crc_pitch = 0;
    // Round kernel (launch_wave3 fills these): a wave's round count is kq + (wave < kr), the units of
    // the launch split over its waves on the host, so no wave divides 64-bit values in its prologue.
    uint32_t kq = 0, kr = 0;
    uint32_t lab_seq = 0;  // lab clock stamps only (LabClock): the launch's number
};

// lab clock stamps: launches numbered by the host (kernel argument), see LabClock
inline std::atomic<uint32_t> g_lab_seq{0};

// The launch over one contiguous run of chunks: verify reads crc_in and reports into *result with
// chunk_base added to its chunk indices, compute writes crc_out
inline ChunkLaunch contiguous_launch(const void *data, uint64_t len, uint32_t bpc, const void *crc_in, void *crc_out,
                                     unsigned long long *result, uint64_t chunk_base, int check_short_tail,
                                     bool overlap) {
    ChunkLaunch a{};
    a.data = static_cast<const uint8_t *>(data);
    a.len = len;
    a.bpc = bpc;
    a.crc_be = static_cast<const uint8_t *>(crc_in);
    a.out_be = static_cast<uint8_t *>(crc_out);
    a.result = result;
    a.chunk_base = chunk_base;
    a.check_short_tail = check_short_tail;
    a.overlap_previous = overlap;
    return a;
}

// The launch of a planned pitch stream whose first packet's data and words are at data / crc
inline ChunkLaunch pitch_stream_launch(const PitchStream &s, const uint8_t *data, uint8_t *crc, uint32_t bpc,
                                       int check_short_tail, unsigned long long *result) {
    ChunkLaunch a{};
    a.data = data;
    a.crc_be = a.out_be = crc;
    a.bpc = bpc;
    a.result = result;
    a.check_short_tail = check_short_tail;
    a.pitch = s.pitch;
    a.crc_pitch = s.crc_pitch;
    a.npk = s.npk;
    a.geom = s.geom;
    a.last_len = s.last_len;
    return a;
}

// Compute mode over a stream whose CRC words sit inside each packet (the wire layout: 512 B of
// words per 64 KiB packet, 66 KiB apart) writes 8 MiB per GiB as small regions scattered over
// the arena, interleaved with the read stream: 1 GiB took 213 us against 186 us with the words
// written densely (tools/compute_layout_probe.py, docs/DESIGN_HISTORY.md §4.3). With a WordScratch the words
// go densely into it and one copy kernel scatters them to the packets afterwards.
struct WordScratch {
    uint8_t *d = nullptr;
    uint64_t cap = 0;
    hipEvent_t used = nullptr;  // recorded after the last launch that read the scratch
    void release();
};
// Chunks of R * 4096 bytes (R >= 2; 8 KiB ... 64 KiB and any other multiple of 4096): the round
// kernel computes the CRC of every 4096-byte piece into a ctx-owned scratch (two buffers used in
// turn, so a launch that overlaps its predecessor never writes the words that predecessor's combine
// still reads), then a combine kernel folds each chunk's R piece CRCs (launch_chunks, pieces != null).
struct PieceScratch {
    uint8_t *d[2] = {nullptr, nullptr};
    uint64_t cap[2] = {0, 0};
    hipEvent_t used[2] = {nullptr, nullptr};  // recorded after the combine that read buffer i
    hipStream_t on[2] = {nullptr, nullptr};   // the stream that combine ran on
    unsigned next = 0;
    void release();
};
// Where a long descriptor list's host-to-device copy runs (round 6): on `side`, beside the launch before
// it, with `stream` waiting for `copied`; in `stream` itself when null or below kSideCopyMinBytes
struct DescCopy {
    hipStream_t side = nullptr;
    hipEvent_t copied = nullptr;
};

// What every launcher needs beyond its work (launch_env, ctx.h)
struct LaunchEnv {
    const uint32_t *tables = nullptr, *fold = nullptr;  // slice-table image, lane-fold GF(2) matrices (device)
    int grid_cap = 0;
    hipStream_t stream = nullptr;
    WordScratch *words = nullptr;          // null: compute writes its words in place
    PieceScratch *pieces = nullptr;        // null: no pieces + combine, no unit map
    const DescCopy *desc_copy = nullptr;   // null: descriptors copy in `stream`
};

// f(std::integral_constant<int, BPC>) for the chunk sizes that have a kernel of their own: the round
// kernel's, and with kMultiRound the multi-round kernel's; hipErrorInvalidValue for every other bpc
template <bool kMultiRound = false, class F>
hipError_t dispatch_bpc(uint32_t bpc, F &&f) {
    switch (bpc) {
    case 512: return f(std::integral_constant<int, 512>());
    case 1024: return f(std::integral_constant<int, 1024>());
    case 2048: return f(std::integral_constant<int, 2048>());
    case 4096: return f(std::integral_constant<int, 4096>());
    default: break;
    }
    if constexpr (kMultiRound) {
        if (bpc == 8192) return f(std::integral_constant<int, 8192>());
        if (bpc == 16384) return f(std::integral_constant<int, 16384>());
        if (bpc == 65536) return f(std::integral_constant<int, 65536>());
    }
    return hipErrorInvalidValue;
}

// One contiguous block: the round, the multi-round or (unaligned, short, other bpc) the chunk-per-lane kernel
hipError_t launch_chunks(const LaunchEnv &env, const ChunkLaunch &a, bool verify);

// A planned constant-pitch packet stream (pitch_stream_launch): the pitch walk; compute goes through
// env.words when the words sit inside the packets; bpc = R x 4096: pieces in env.pieces + the combine
hipError_t launch_packet_stream(const LaunchEnv &env, const ChunkLaunch &a, bool verify);

// Launches over d_seg (a device copy of a planned h_seg array), or, with h_inline and
// nseg <= kInlineSegments, over descriptors carried in the kernel arguments (no copy before the
// kernel); stride != 0: h_inline = {first, last} and the kernel derives the rest (SegLaunch::stride)
hipError_t launch_segments(const LaunchEnv &env, const DevSegment *d_seg, uint32_t nseg, uint64_t units,
                           uint64_t uniform, uint32_t bpc, bool verify, int check_short_tail,
                           unsigned long long *result, const DevSegment *h_inline = nullptr, uint64_t stride = 0,
                           uint8_t *dense_words = nullptr, const uint32_t *unit_seg = nullptr);

// The chunk-per-lane packet kernel over a device array of descriptors: one wave per packet
hipError_t launch_packets(const LaunchEnv &env, const uint8_t *d_arena, const DevPacket *d_pk, uint64_t n,
                          uint32_t bpc, bool verify, int check_short_tail, unsigned long long *result);

// Packet batch (packets API, block reader, output stream): descriptors in host memory; h_stage/d_stage are pinned/
// device staging for n DevSegments. plan_packet_batch picks the route, this launches it. Keys: packet << 32 | chunk.
// bad_index != null: every packet is first checked against [0, arena_len) (hipErrorInvalidValue
// and *bad_index = the first one outside). staged != null: set when the launch copies h_stage to the
// device asynchronously (the caller may reuse h_stage only after that copy ran); false when the
// kernel's arguments carried everything (the pitch walk, inline descriptors).
hipError_t launch_packet_batch(const LaunchEnv &env, const uint8_t *d_arena, const DevPacket *h_pk, size_t n,
                               uint32_t bpc, bool verify, int check_short_tail, unsigned long long *result,
                               DevSegment *h_stage, DevSegment *d_stage, uint64_t arena_len = 0,
                               size_t *bad_index = nullptr, bool overlap_previous = false, bool *staged = nullptr);

// Composite CRC of a block from its chunk words (crc32c_compose.hip). A lane runs Horner over
// kComposeLaneWords consecutive words, a workgroup of kComposeThreads lanes reduces kComposeSpan words to
// one partial, and the partials are reduced by the same kernel until one is left.
constexpr int kComposeLaneWords = 4;
constexpr int kComposeThreads = 256;
constexpr uint64_t kComposeSpan = uint64_t(kComposeLaneWords) * kComposeThreads;
constexpr uint64_t kComposeMaxWords = uint64_t(1) << 40;  // the first level's grid stays below 2^31
// ctx-owned buffers of the composite calls, apart from the word and piece scratch of the compute paths:
// the chunk words of a composite from data, and the workgroups' partials of every level
struct ComposeScratch {
    uint8_t *words = nullptr, *partials = nullptr;
    uint64_t words_cap = 0, partials_cap = 0;
    void release();
};
// Makes *d at least `need` bytes. The buffers serve launches of one stream at a time (a ctx's stream is
// drained before it is switched), so a buffer that has to grow is freed after `stream` drained.
hipError_t grow_compose_buffer(uint8_t **d, uint64_t *cap, uint64_t need, hipStream_t stream);
// n >= 1 big-endian words at d_crc_be (4-byte aligned, n <= kComposeMaxWords), `unit` bytes each but the last
// (`tail` bytes, 1..unit), polynomial `poly` -> the composite in *d_out (host order). Nothing waits;
// *launched (if given) receives the number of kernel launches.
hipError_t launch_compose_words(const LaunchEnv &env, ComposeScratch *scratch, const uint8_t *d_crc_be, uint64_t n,
                                uint32_t unit, uint32_t tail, uint32_t poly, uint32_t *d_out,
                                unsigned *launched = nullptr);

// One planned gather launch (crc32c_gather.hip; plan_gather_launch, launch_plan.h): g's ranges from d_src to
// d_dst, its descriptors in the kernel arguments, so nothing of g is read after the call returns and no
// staging buffer is involved (any thread may launch on `stream`). g.n == 0 launches nothing.
hipError_t launch_gather(hipStream_t stream, void *d_dst, uint64_t dst_len, const void *d_src, uint64_t src_len,
                         const GatherLaunch &g);
// The same launch as a guarded delivery (launch_plan.h: DeliverGuard): every range clipped on the device to
// the limit the guard's words give, *guard.gate_out written by one lane. g.n == 0 launches one workgroup
// that only passes the gate on.
hipError_t launch_deliver(hipStream_t stream, void *d_dst, uint64_t dst_len, const void *d_src, uint64_t src_len,
                          const GatherLaunch &g, const DeliverGuard &guard);
// The same launch with a source per range (plan_gather_launch over ranges whose src_off is a device ADDRESS,
// checked by gather_sources_first_bad): a range's loads stay inside [src_off, src_off + len).
hipError_t launch_gather_sources(hipStream_t stream, void *d_dst, uint64_t dst_len, const GatherLaunch &g);

// HDFS3_LAB=1 builds the measurement library (libhdfs3_crc_lab.so: tools/, the A/B tests):
// the same production launchers plus a process-wide kernel-variant knob, the kernel
// variants of crc32c_experiments.hip and the read-ceiling kernels. The product library
// (libhdfs3_crc.so) is built with HDFS3_LAB=0: g_variant is the constant 0, so no
// variant, diagnostic or wrong-on-purpose kernel is reachable from it.
#ifndef HDFS3_LAB
#define HDFS3_LAB 0
#endif
#if HDFS3_LAB
void set_variant(int v);
extern int g_variant;
// clock stamps (LabClock): install a device buffer of cap x 4 words; *n_out = stamps in the previous one
hipError_t lab_clock_buffer(unsigned long long *d, unsigned int cap, unsigned int *n_out);
// every wave's stamps (LabClock with a wave buffer): cap x 4 words; *n_out = launches stamped into the
// previous one
hipError_t lab_wave_buffer(unsigned long long *d, unsigned int cap, unsigned int *n_out);
// The A/B variants (crc32c_experiments.hip): variant != 0, bpc with a whole-round kernel.
hipError_t launch_experiment(const LaunchEnv &env, int variant, const ChunkLaunch &a, bool verify);

// Measurement-only kernels (bench/profiling): HBM read ceiling and the CRC
// kernel's access pattern without the table arithmetic.
hipError_t launch_stream_read(const uint8_t *d, uint64_t len, uint32_t *sink, int grid,
                              hipStream_t stream, bool overlap_previous = false);
hipError_t launch_lane_read(const uint8_t *d, uint64_t len, uint32_t bpc, uint32_t *sink,
                            int grid_cap, hipStream_t stream);
#else
constexpr int g_variant = 0;
#endif

}  // namespace hdfs3crc
