// Launch planning of the CRC kernels' host layer: which kernel a packet stream, a block batch or a
// packet batch takes, and that launch's geometry. Plain host arithmetic, no GPU runtime
// (tests/native/launch_plan_check.cpp); crc32c_kernels.hip turns a plan into launches.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hdfs3crc {

constexpr int kRoundBytes = 4096;         // a wave's round: 64 lanes x 64 bytes
constexpr uint32_t kInlineSegments = 16;  // small segment lists travel in the kernel arguments
// Lists longer than this take the unit map (below it the search is a few loads and the map's launch
// is not worth it)
constexpr size_t kUnitMapMinSegments = 256;
// word regions at most this long (per packet) take the dense path: 64 KiB = 8 MiB packets at bpc 512
constexpr uint64_t kDenseWordsMaxRegion = 64 * 1024;
constexpr uint64_t kPiecesMinBytes = uint64_t(256) << 20;  // launch_chunks: pieces + combine at 8 / 16 / 64 KiB
constexpr size_t kSideCopyMinBytes = size_t(256) << 10;    // descriptor lists that copy on the side stream (DescCopy)

// the round kernel's chunk sizes (a chunk is G = bpc / 64 lanes of one round)
constexpr bool round_bpc(uint32_t bpc) { return bpc == 512 || bpc == 1024 || bpc == 2048 || bpc == 4096; }
// chunks of R >= 2 whole rounds: 4096-byte piece CRCs + a combine
constexpr bool pieces_bpc(uint32_t bpc) { return bpc > uint32_t(kRoundBytes) && bpc % kRoundBytes == 0; }

// ---- the round kernel's word output (crc32c_wave.h: RoundWords) -----------------------------------
// What becomes of the CRC words a round finishes; each policy's code and measurements are one RoundWords unit.
enum class Words {
    kCompare,   // verify
    kPerRound,  // each round's words stored as the round finishes
    kHold8,     // bpc 512: 8 rounds' words per VGPR, up to 8 such VGPRs stored in one burst
    kHold64,    // bpc 4096: 64 rounds' words in one VGPR, one store per 64 rounds
    kStaged,    // a window of rounds staged in LDS, written by the workgroup as whole lines
};
enum class WalkKind { kBlock, kPitch, kSeg };  // BlockWalk, PitchWalk, SegWalk (crc32c_wave.h)
// 16 waves x R rounds x (4096 / bpc) words = the 4096 words (16 KiB) the half fold image leaves:
// 32 rounds at bpc 512, 64 at 1024, 128 at 2048
constexpr uint32_t kStageMaxRounds(int bpc) { return uint32_t(bpc / 16); }
constexpr uint64_t kAnyUnits = ~uint64_t(0);  // words_policy: a launch of no known size
// The policy of one launch of the round kernel: `units` rounds over workgroups of `tpb` threads, every wave
// kq rounds and the first kr waves one more (ChunkLaunch::kq/kr). The only place that decides it.
constexpr Words words_policy(bool verify, WalkKind walk, int bpc, int tpb, uint64_t units, uint32_t kq, uint32_t kr) {
    if (verify) return Words::kCompare;
    if (walk == WalkKind::kBlock) {
        if (bpc == 4096) return Words::kHold64;
        // staged words need the whole LDS of a 1024-thread workgroup and a 31-bit store offset (words below
        // 2 GiB); at bpc 512 only while they fit one window (beyond it the held stores measured faster at
        // 1 GiB: 160.4 against 163.1 us in windows)
        const bool fit = tpb == 1024 && units * uint64_t(4 * (kRoundBytes / bpc)) < (uint64_t(1) << 31);
        if (fit && (bpc != 512 || uint64_t(kq) + (kr ? 1u : 0u) <= kStageMaxRounds(512))) return Words::kStaged;
        return bpc == 512 ? Words::kHold8 : Words::kPerRound;
    }
    // compute over a packet stream of <= 16 MiB (the writer's batches, 256-thread workgroups): each round's
    // words stored at once. With two rounds per wave the held stores only delay the words to the wave's end:
    // the writer's 64-packet batch 5.32 -> 4.47 us against 4.41 for its verify (lab 163, round 6,
    // profiles/r06/r6n_partial_rate.jsonl)
    if (walk == WalkKind::kPitch && units <= 4096) return Words::kPerRound;
    return bpc == 512 ? Words::kHold8 : Words::kPerRound;  // a segment walk holds with per-lane addresses
}

// The 4 KiB units of a packet stream (PitchWalk, crc32c_wave.h). A packet of whole chunks is
// ceil(bytes / 4096) units; its last unit may be PARTIAL (the writer's 127-chunk packets at bpc
// 512: 65,024 B = 15 whole rounds + 3,584 B, OutputStreamImpl.cpp:161-170): its loads are bounded by
// a buffer resource of ptail bytes, so the lanes past the last whole chunk read zeros and their
// results are dropped. Unit u -> packet u / upp by a multiply-shift (u < 2^31: q = (u * magic) >>
// shift, Granlund-Montgomery with N = 31), so upp need not be a power of two.
struct PacketGeom {
    uint64_t pk_len = 0;  // data bytes of every packet but the last (whole chunks)
    uint32_t upp = 0;     // units per packet but the last
    uint32_t magic = 0, shift = 0;
    uint32_t ptail = 0;   // valid bytes of such a packet's last unit (4096: whole)
    uint32_t lunits = 0;  // units of the last packet (its whole chunks only)
    uint32_t ltail = 0;   // valid bytes of the last packet's last unit
};
// Fills g for npk packets of data_len bytes (the last last_len) with chunks of unit_bpc bytes
// (<= 4096; callers at bpc = R x 4096 pass 4096). False when it does not fit the walk: a non-last
// packet that ends in a short chunk, no unit at all, or 2^31 units or more. One packet (npk == 1) is
// its own last packet: upp = lunits, ptail = ltail and pk_len = 0, so every unit is a round of packet 0.
bool packet_geom(uint64_t data_len, uint64_t last_len, uint64_t npk, uint32_t unit_bpc, PacketGeom *g);

// Packet-descriptor as seen by the device (mirrors hdfs3_pkt_desc).
struct DevPacket {
    uint64_t data_off;
    uint64_t crc_off;
    uint32_t data_len;
    uint32_t reserved;
};

// One independent byte range of a segmented launch (a block of a batch, or one packet's
// data region): device pointers, its 4 KiB units start at global unit unit_begin,
// chunk c of it is reported as key_base + c (packets: packet << 32).
struct DevSegment {
    const uint8_t *data;
    uint8_t *crc;            // verify: stored BE32 words; compute: written here
    uint64_t len;
    uint64_t unit_begin;
    uint64_t key_base;
};

// A verify result word whose key has two halves (key_base above: index << 32 | chunk; the word holds ~key,
// 0 while nothing was bad): *hi / *lo (either may be null) receive the halves, -1 / -1 for 0.
// hdfs3_crc_decode_result is the one-part form for chunk keys.
inline void split_result_key(unsigned long long raw, int64_t *hi, int64_t *lo) {
    const uint64_t key = ~uint64_t(raw);
    if (hi) *hi = raw ? int64_t(key >> 32) : -1;
    if (lo) *lo = raw ? int64_t(key & 0xFFFFFFFFu) : -1;
}

// Units of a segment of len bytes at bpc <= 4096: its whole chunks cut into 4 KiB units, the
// last one partial when the whole chunks end inside a round (PacketGeom); a short last chunk is
// the kernel's one-lane tail
constexpr uint64_t seg_units(uint64_t len, uint32_t bpc) { return (len / bpc * bpc + 4095) / 4096; }

// Fills h_seg for n segments (data/crc/len/key_base already set) and returns the total
// unit count (seg_units); *uniform = units per segment when every segment but the last has
// the same count (direct unit -> segment mapping), else 0 (binary search).
uint64_t plan_segments(DevSegment *h_seg, size_t n, uint32_t bpc, uint64_t *uniform);
// True when the segmented wave kernel can take these segments: bpc in {512..4096},
// every data pointer 16-byte aligned and every CRC pointer 4-byte aligned.
bool segments_fast(const DevSegment *h_seg, size_t n, uint32_t bpc);

// constant-pitch packet streams (ChunkLaunch::pitch): whether the wave kernel's pitch mode
// takes them (bpc 512..4096 or R x 4096, aligned, every packet but the last whole chunks)
bool packet_stream_ok(uint64_t data_len, uint64_t last_len, uint64_t npk, uint32_t bpc, const void *data,
                      const void *crc, uint64_t pitch, PacketGeom *geom);

// A packet stream the pitch walk takes (pitch_stream_launch, crc32c_kernels.h): crc_pitch 0 = pitch
struct PitchStream {
    uint64_t pitch = 0, crc_pitch = 0, npk = 0;
    uint32_t last_len = 0;
    PacketGeom geom;
};
// packet_stream_ok, and a piece scratch at bpc = R x 4096; lab variants 52 / 53 refuse every stream
bool plan_packet_stream(uint64_t data_len, uint64_t last_len, uint64_t npk, uint32_t bpc, const void *data,
                        const void *crc, uint64_t pitch, bool have_pieces, int variant, PitchStream *s);
// equal blocks (the last may be shorter) whose data and words sit at two constant strides (blocks of one
// 2-D tensor): the pitch mode with crc_pitch, at bpc <= 4096; false (lab variant 54): the segmented kernel
bool plan_strided_blocks(const DevSegment *h_seg, size_t n, uint32_t bpc, int variant, PitchStream *s);

enum class Route {
    kPitchStream,      // one constant-pitch stream: the round kernel's pitch walk (plan.stream)
    kStridedSegments,  // constant pitch, partial rounds: the segmented kernel derives every descriptor
    kSegmentPieces,    // bpc = R x 4096 over a descriptor list: piece CRCs + the segments' combine
    kInlineSegments,   // up to kInlineSegments descriptors in the kernel arguments
    kMappedSegments,   // a long ragged list: descriptor array + the unit -> segment map
    kStagedSegments,   // descriptor array copied to the device
    kPackets,          // unaligned / other chunk sizes: the chunk-per-lane packet kernel
    kOutOfBounds,      // packet bad_index lies outside [0, arena_len)
};

struct BatchPlan {
    Route route = Route::kPackets;
    PitchStream stream;    // kPitchStream; .pitch also kStridedSegments
    uint64_t units = 0, uniform = 0;  // segment routes at bpc <= 4096: 4 KiB units; per segment when all agree
    uint64_t pieces_total = 0, max_chunks = 0;  // kSegmentPieces: 4096-byte pieces; the most whole chunks in a segment
    bool any_tail = false;    // kSegmentPieces: some segment ends in a short chunk
    size_t bad_index = 0;     // kOutOfBounds
};
// Routes n >= 1 packets (offsets into an arena at device address `arena`) in one pass over h_pk with no
// allocation (16K packets per GiB: on the call's critical path). arena_len != null: each packet is first
// checked against [0, *arena_len). have_pieces: a PieceScratch is at hand. variant: the lab's knob (product:
// 0); 17 forces kPackets, 52 descriptor arrays, 53 only refuses the pitch walk. h_stage[0..n) is filled for
// the routes that read it: planned DevSegments (kSegmentPieces ... kStagedSegments), kPackets: the DevPackets.
BatchPlan plan_packet_batch(uint64_t arena, const DevPacket *h_pk, size_t n, uint32_t bpc, const uint64_t *arena_len,
                            bool have_pieces, int variant, DevSegment *h_stage);

// ---- range gather (crc32c_gather.hip) -------------------------------------------------------------
// One byte range of a gather: len bytes from src + src_off to dst + dst_off (mirrors hdfs3_copy_range).
struct CopyRange {
    uint64_t src_off, dst_off, len;
};
// A gather launch carries its ranges in the kernel arguments: at most this many (a default reader batch
// of 64 packets is one launch); longer lists take more launches
constexpr uint32_t kGatherMaxRanges = 64;
// A workgroup's tile: kGatherThreads lanes x kGatherLinesPerLane destination lines of 16 bytes. A range's
// lines are the aligned 16-byte lines of the destination that hold any of its bytes, so its first and
// last line may be partial (the kernel writes those with byte stores)
constexpr uint32_t kGatherThreads = 256;
constexpr uint32_t kGatherLinesPerLane = 4;
constexpr uint64_t kGatherTileBytes = uint64_t(kGatherThreads) * kGatherLinesPerLane * 16;
constexpr uint64_t kGatherMaxTiles = (uint64_t(1) << 31) - 1;  // a launch's grid
struct GatherLaunch {
    CopyRange r[kGatherMaxRanges];
    uint32_t tile_end[kGatherMaxRanges];  // tiles of ranges 0 .. i: workgroup w copies range i, tile_end[i-1] <= w < tile_end[i]
    uint32_t n;
};
// tiles of a range whose first destination byte is at address dst_addr
constexpr uint64_t gather_tiles(uint64_t dst_addr, uint64_t len) {
    return len ? (((dst_addr & 15) + len + 15) / 16 * 16 + kGatherTileBytes - 1) / kGatherTileBytes : 0;
}
// Index of the first range that leaves [0, src_len) or [0, dst_len) or has more than kGatherMaxTiles
// tiles, n when every range is inside (empty ranges are checked like the others)
size_t gather_first_bad(const CopyRange *in, size_t n, uint64_t src_len, uint64_t dst_len);
// Fills *g from in[pos ..) for a destination at address dst_addr and returns the position it stopped at
// (n: this was the last launch): empty ranges dropped, a range that continues its predecessor on both
// sides merged into it, closed at kGatherMaxRanges ranges or kGatherMaxTiles tiles. g->n may be 0 (nothing
// but empty ranges were left). The ranges were checked by gather_first_bad.
size_t plan_gather_launch(uint64_t dst_addr, const CopyRange *in, size_t n, size_t pos, GatherLaunch *g);
// The gather with a source per range (mirrors hdfs3_src_range): src_off is the range's source ADDRESS and the
// range its own source buffer. plan_gather_launch plans such a list as it stands (a range merges into a
// predecessor it continues in address and destination; the merged range is again its own source). Index of
// the first range that leaves [0, dst_len), whose src_off + len wraps, or that has more than kGatherMaxTiles
// tiles; n when there is none.
size_t gather_sources_first_bad(const CopyRange *in, size_t n, uint64_t dst_len);

// ---- guarded delivery (crc32c_gather.hip: the gather behind a verify's result word) -----------------
// A delivery copies ranges as the gather does, each clipped to a LIMIT (a source offset) that the kernel
// derives from two device words: the result word of the verify that covered the source data (0, or
// ~first_bad_chunk; chunk 0 is the source byte data_off) and a chain word gate_in (non-zero: an earlier
// delivery of the chain stopped, nothing is copied). The kernel and the host (which needs the same number
// to know how many bytes arrived) share the arithmetic below.
constexpr uint64_t kDeliverNoLimit = ~uint64_t(0);
// The limit: 0 behind a closed gate, none behind a clean result, else the start of the granule (counted
// from data_off) that holds the bad chunk. granule, bpc >= 1. Saturates instead of wrapping: a bad chunk
// whose offset does not fit 64 bits lies past every buffer, as no limit does.
constexpr uint64_t deliver_limit(uint64_t result, uint64_t gate_in, uint64_t data_off, uint64_t granule, uint32_t bpc) {
    if (gate_in) return 0;
    if (!result) return kDeliverNoLimit;
    const uint64_t bad = ~result;
    if (bad > kDeliverNoLimit / bpc) return kDeliverNoLimit;
    const uint64_t off = bad * bpc / granule * granule;
    return off > kDeliverNoLimit - data_off ? kDeliverNoLimit : data_off + off;
}
// bytes of a range {src_off, len} below the limit: its first clamp(limit - src_off, 0, len)
constexpr uint64_t deliver_clip(uint64_t limit, uint64_t src_off, uint64_t len) {
    return limit <= src_off ? 0 : limit - src_off < len ? limit - src_off : len;
}
// The chain word a delivery leaves: a closed gate stays as it is, a bad result closes it with the bad
// chunk's index plus chunk_base in the result words' own encoding, a clean one leaves it open (0)
constexpr uint64_t deliver_gate(uint64_t result, uint64_t gate_in, uint64_t chunk_base) {
    return gate_in ? gate_in : result ? ~(chunk_base + ~result) : 0;
}
// The guard as the kernel receives it (mirrors hdfs3_deliver_guard)
struct DeliverGuard {
    const uint64_t *result;
    const uint64_t *gate_in;  // may be null: read as 0
    uint64_t *gate_out;       // may be null
    uint64_t data_off, chunk_base, granule;
    uint32_t bpc;
};

}  // namespace hdfs3crc
