// CPU check of the launch planner (libhdfs3_amd/csrc/launch_plan.cpp), built with the host compiler
// under ASan + UBSan by tests/test_launch_plan.py. Four parts: the unit -> packet multiply-shift of
// PacketGeom, the pitch walk's coverage of a stream's bytes (a host model of PitchWalk::view,
// crc32c_wave.h), the route plan_packet_batch picks for small descriptor lists, and the word policy
// words_policy gives a launch of the round kernel. The expected
// routes are read off the branch conditions of launch_packet_batch as it stood before the planner
// was split out of it ("before:" = that function's line in crc32c_kernels.hip at commit 023ec6b).
#include <cstdio>
#include <cstring>
#include <vector>

#include "launch_plan.h"

using namespace hdfs3crc;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_failed <= 20) {                       \
                std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

// ---- a. the unit -> packet divide ---------------------------------------------------------------
void check_divide_at(const PacketGeom &g, uint64_t u) {
    if (u >= (uint64_t(1) << 31)) return;
    const uint64_t q = (u * g.magic) >> g.shift;
    CHECK(q == u / g.upp, "upp %u u %llu: %llu", g.upp, (unsigned long long)u, (unsigned long long)q);
}

void check_divide() {
    std::vector<uint32_t> upps;
    for (uint32_t upp = 1; upp <= 600; ++upp) upps.push_back(upp);
    for (uint32_t upp : {(1u << 20) - 1, 1u << 20, (1u << 20) + 1}) upps.push_back(upp);
    for (uint32_t upp : upps) {
        PacketGeom g;
        const uint64_t len = uint64_t(upp) * kRoundBytes;
        CHECK(packet_geom(len, len, 2, 4096, &g), "upp %u", upp);
        CHECK(g.upp == upp, "upp %u: %u", upp, g.upp);
        for (uint64_t u : {uint64_t(0), uint64_t(upp) - 1, uint64_t(upp)}) check_divide_at(g, u);
        for (uint64_t k : {2, 3, 5, 64, 1000, 4097, 65535, 1 << 20})
            for (uint64_t u : {k * upp - 1, k * upp, k * upp + 1}) check_divide_at(g, u);
        const uint64_t top = (uint64_t(1) << 31) - 1;  // the largest unit index, and the multiples around it
        check_divide_at(g, top);
        check_divide_at(g, top / upp * upp);
        if (top / upp * upp) check_divide_at(g, top / upp * upp - 1);
    }
}

// ---- b. walk coverage ---------------------------------------------------------------------------
// PitchWalk::view on the host: unit u -> packet, round, valid bytes
struct Unit {
    uint32_t pk, r, nb;
};
Unit walk_view(const PacketGeom &g, uint64_t npk, uint32_t u) {
    const uint32_t pk = uint32_t((uint64_t(u) * g.magic) >> g.shift), r = u - pk * g.upp;
    const bool lastp = pk == uint32_t(npk - 1);
    const uint32_t nb = r + 1 == (lastp ? g.lunits : g.upp) ? (lastp ? g.ltail : g.ptail) : uint32_t(kRoundBytes);
    return Unit{pk, r, nb};
}

void check_walk(uint32_t bpc, uint64_t npk, uint64_t data_len, uint64_t last_len) {
    PacketGeom g;
    const bool ok = packet_geom(data_len, last_len, npk, bpc, &g);
    if (npk == 1 && last_len < bpc) {  // no whole chunk: no unit at all
        CHECK(!ok, "bpc %u one packet of %llu", bpc, (unsigned long long)last_len);
        return;
    }
    CHECK(ok, "bpc %u npk %llu len %llu last %llu", bpc, (unsigned long long)npk, (unsigned long long)data_len,
          (unsigned long long)last_len);
    if (!ok) return;
    const uint64_t units = (npk - 1) * uint64_t(g.upp) + g.lunits;
    std::vector<uint64_t> end(npk, 0);  // per packet: the bytes covered so far, contiguous from 0
    for (uint64_t u = 0; u < units; ++u) {
        const Unit v = walk_view(g, npk, uint32_t(u));
        if (v.pk >= npk) {
            CHECK(false, "unit %llu -> packet %u of %llu", (unsigned long long)u, v.pk, (unsigned long long)npk);
            return;
        }
        const uint64_t len = v.pk + 1 == npk ? last_len : data_len;
        // each byte once: a unit starts where the packet's previous one ended
        CHECK(uint64_t(v.r) * kRoundBytes == end[v.pk] && v.nb >= 1 && v.nb <= uint32_t(kRoundBytes),
              "bpc %u npk %llu len %llu last %llu: unit %llu = packet %u round %u, %u bytes after %llu", bpc,
              (unsigned long long)npk, (unsigned long long)data_len, (unsigned long long)last_len,
              (unsigned long long)u, v.pk, v.r, v.nb, (unsigned long long)end[v.pk]);
        end[v.pk] += v.nb;
        CHECK(end[v.pk] <= len, "bpc %u npk %llu len %llu last %llu: packet %u read to %llu", bpc,
              (unsigned long long)npk, (unsigned long long)data_len, (unsigned long long)last_len, v.pk,
              (unsigned long long)end[v.pk]);
    }
    for (uint64_t pk = 0; pk < npk; ++pk) {  // exactly the whole chunks
        const uint64_t len = pk + 1 == npk ? last_len : data_len;
        CHECK(end[pk] == len / bpc * bpc, "bpc %u npk %llu len %llu last %llu: packet %llu covered to %llu", bpc,
              (unsigned long long)npk, (unsigned long long)data_len, (unsigned long long)last_len,
              (unsigned long long)pk, (unsigned long long)end[pk]);
    }
}

void check_walks() {
    for (uint32_t bpc : {512u, 1024u, 2048u, 4096u}) {
        const uint64_t lens[] = {bpc, 4096, 4096 + bpc, 127 * 512, 65536, 17 * 4096 + 512};
        for (uint64_t data_len : lens) {
            if (data_len % bpc) continue;
            std::vector<uint64_t> lasts = {0, 100, bpc, data_len};
            if (data_len >= bpc) lasts.push_back(data_len - bpc);
            if (data_len >= 300) lasts.push_back(data_len - 300);
            for (uint64_t last_len : lasts) {
                if (last_len > data_len) continue;
                // one packet: every unit is a round of packet 0, whatever its length
                for (uint64_t npk : {1, 2, 3, 64, 4097}) check_walk(bpc, npk, data_len, last_len);
            }
        }
        // one packet of many rounds that ends inside a chunk (a non-last packet could not)
        check_walk(bpc, 1, 131072, 131072 - 7);
        check_walk(bpc, 1, 65536, 65024 - 11);
    }
    // chunks of R x 4096: the pieces path plans its 4096-byte pieces with unit_bpc 4096 whatever R is,
    // so a one-packet stream's pieces are the whole rounds of last_len
    for (uint64_t last_len : {uint64_t(4096), uint64_t(4096 + 8192), uint64_t(4096 * 5 + 100), uint64_t(65024 - 11),
                              uint64_t(65536 - 300), uint64_t(65536)})
        check_walk(4096, 1, 65536, last_len);
    check_walk(4096, 1, 131072, 131072 - 7);
    PacketGeom g;
    // a one-packet stream has the last packet's geometry: no unit can map past packet 0
    CHECK(packet_geom(65536, 65536 - 300, 1, 512, &g) && g.upp == 16 && g.lunits == 16 && g.ptail == g.ltail &&
              g.ltail == 4096 - 512 && g.pk_len == 0,
          "one packet: upp %u lunits %u ptail %u ltail %u", g.upp, g.lunits, g.ptail, g.ltail);
    CHECK(!packet_geom(65536 - 300, 100, 2, 512, &g), "a non-last packet that is not whole chunks");
    CHECK(!packet_geom(65536, 65536, 0, 512, &g), "npk = 0");
    CHECK(!packet_geom(65536, 65537, 2, 512, &g), "last_len > data_len");
    // 16 units per packet: 2^27 packets are 2^31 units, one round less is the largest launch
    CHECK(!packet_geom(65536, 65536, uint64_t(1) << 27, 512, &g), "2^31 units");
    CHECK(!packet_geom(65536, 0, (uint64_t(1) << 27) + 1, 512, &g), "2^31 units before an empty last packet");
    CHECK(packet_geom(65536, 65536 - 4096, uint64_t(1) << 27, 512, &g), "2^31 - 1 units");
}

// ---- c. the route table -------------------------------------------------------------------------
constexpr uint64_t kArena = uint64_t(0x7f12) << 32;  // a device address, never dereferenced
constexpr uint64_t kSlot = 66048;                    // the block reader's packet pitch: 512 B of words + 64 KiB
const char *name(Route r) {
    static const char *const n[] = {"pitch stream", "strided segments", "segment pieces", "inline segments",
                                    "mapped segments", "staged segments", "packets", "out of bounds"};
    return n[int(r)];
}

// n packets in slots kSlot apart, words at the slot's start, data 512 B in; len(i) bytes each
template <class Len>
std::vector<DevPacket> slots(size_t n, Len len) {
    std::vector<DevPacket> pk(n);
    for (size_t i = 0; i < n; ++i) pk[i] = DevPacket{i * kSlot + 512, i * kSlot, uint32_t(len(i)), 0};
    return pk;
}
std::vector<DevPacket> stream(size_t n, uint32_t len) {
    return slots(n, [=](size_t) { return len; });
}
// lengths that differ in bytes and in 4 KiB units, all multiples of 512
std::vector<DevPacket> ragged(size_t n) {
    return slots(n, [](size_t i) { return 32768 + (i % 5) * 4096 + (i % 3) * 512; });
}

struct Planned {
    BatchPlan p;
    std::vector<DevSegment> stage;
};
Planned plan(const std::vector<DevPacket> &pk, uint32_t bpc, bool have_pieces, int variant = 0,
             const uint64_t *arena_len = nullptr) {
    Planned r;
    r.stage.resize(pk.size());
    std::memset(static_cast<void *>(r.stage.data()), 0xEE, pk.size() * sizeof(DevSegment));
    r.p = plan_packet_batch(kArena, pk.data(), pk.size(), bpc, arena_len, have_pieces, variant, r.stage.data());
    return r;
}
#define EXPECT_ROUTE(planned, want) CHECK((planned).p.route == (want), "got %s", name((planned).p.route))

bool untouched(const Planned &r) {
    for (const DevSegment &s : r.stage)
        if (s.len != 0xEEEEEEEEEEEEEEEEull) return false;
    return true;
}

void check_routes() {
    // before: 743-760, strided (709): one pitch for data and words
    const std::vector<DevPacket> wire = stream(64, 65536);
    Planned r = plan(wire, 512, true);
    EXPECT_ROUTE(r, Route::kPitchStream);
    CHECK(r.p.stream.pitch == kSlot && r.p.stream.crc_pitch == 0 && r.p.stream.npk == 64 &&
              r.p.stream.last_len == 65536 && r.p.stream.geom.upp == 16,
          "pitch %llu crc_pitch %llu", (unsigned long long)r.p.stream.pitch, (unsigned long long)r.p.stream.crc_pitch);
    CHECK(untouched(r), "the pitch stream reads no staged descriptor");
    // before: 716, 754: the words dense at a pitch of their own (the writer's batches)
    std::vector<DevPacket> dense = wire;
    for (size_t i = 0; i < dense.size(); ++i) dense[i].crc_off = 64 * kSlot + i * 512;
    r = plan(dense, 512, true);
    EXPECT_ROUTE(r, Route::kPitchStream);
    CHECK(r.p.stream.pitch == kSlot && r.p.stream.crc_pitch == 512, "crc_pitch %llu",
          (unsigned long long)r.p.stream.crc_pitch);
    // before: 702 (aligned needs the piece scratch above 4096), 185; without it 822-829
    EXPECT_ROUTE(plan(wire, 8192, true), Route::kPitchStream);
    r = plan(wire, 8192, false);
    EXPECT_ROUTE(r, Route::kPackets);
    CHECK(std::memcmp(r.stage.data(), wire.data(), wire.size() * sizeof(DevPacket)) == 0, "DevPackets staged");
    // before: 762: packets that end inside a chunk are no stream (packet_geom), but one stride
    r = plan(stream(17, 65536 - 300), 512, true);
    EXPECT_ROUTE(r, Route::kStridedSegments);
    CHECK(r.p.stream.pitch == kSlot && r.p.uniform == 16 && r.p.units == 17 * 16 && untouched(r), "units %llu",
          (unsigned long long)r.p.units);
    // before: 762 (n > 16), 799
    r = plan(stream(16, 65536 - 300), 512, true);
    EXPECT_ROUTE(r, Route::kInlineSegments);
    CHECK(r.p.uniform == 16 && r.p.units == 256 && r.stage[15].unit_begin == 240 &&
              r.stage[15].key_base == uint64_t(15) << 32 &&
              r.stage[15].data == reinterpret_cast<const uint8_t *>(uintptr_t(kArena + 15 * kSlot + 512)) &&
              r.stage[15].crc == reinterpret_cast<uint8_t *>(uintptr_t(kArena + 15 * kSlot)) &&
              r.stage[15].len == 65536 - 300,
          "inline descriptors");
    // before: 799, 802 (n > 256 and a piece scratch), 819
    r = plan(ragged(16), 512, true);
    EXPECT_ROUTE(r, Route::kInlineSegments);
    CHECK(r.p.uniform == 0 && r.stage[1].unit_begin == 8 && r.stage[2].unit_begin == 8 + 10, "ragged units");
    EXPECT_ROUTE(plan(ragged(17), 512, true), Route::kStagedSegments);
    EXPECT_ROUTE(plan(ragged(256), 512, true), Route::kStagedSegments);
    r = plan(ragged(257), 512, true);
    EXPECT_ROUTE(r, Route::kMappedSegments);
    CHECK(r.p.uniform == 0 && r.p.units == r.stage[256].unit_begin + seg_units(r.stage[256].len, 512), "map units");
    EXPECT_ROUTE(plan(ragged(257), 512, false), Route::kStagedSegments);
    // before: 779-790. Three packets of 61,440 / 28,672 / 12,388 B at 12 KiB chunks: 15 + 7 + 3 pieces
    // of 4096, 5 / 2 / 1 whole chunks, the second ends 4096 B into a chunk and the third 100 B
    const uint32_t lens[3] = {61440, 28672, 12388};
    r = plan(slots(3, [&](size_t i) { return lens[i]; }), 12288, true);
    EXPECT_ROUTE(r, Route::kSegmentPieces);
    CHECK(r.p.pieces_total == 25 && r.p.max_chunks == 5 && r.p.any_tail, "pieces %llu chunks %llu tail %d",
          (unsigned long long)r.p.pieces_total, (unsigned long long)r.p.max_chunks, int(r.p.any_tail));
    CHECK(r.stage[0].unit_begin == 0 && r.stage[1].unit_begin == 15 && r.stage[2].unit_begin == 22, "piece offsets");
    r = plan(slots(3, [](size_t i) { return i == 1 ? 24576 : 12288; }), 12288, true);
    CHECK(r.p.route == Route::kSegmentPieces && r.p.pieces_total == 12 && r.p.max_chunks == 2 && !r.p.any_tail,
          "whole chunks only");
    // before: 730-732, 822: one unaligned packet sends the batch to the chunk-per-lane kernel
    std::vector<DevPacket> odd = ragged(17);
    odd[3].data_off += 8;
    EXPECT_ROUTE(plan(odd, 512, true), Route::kPackets);
    // before: 700, 702: no wave kernel for this chunk size
    EXPECT_ROUTE(plan(wire, 768, true), Route::kPackets);
    // before: 709, 716 (variant 52: no stride at all), 181 (53: the walk refuses, the stride stays)
    r = plan(wire, 512, true, 52);
    CHECK(r.p.route != Route::kPitchStream, "variant 52");
    EXPECT_ROUTE(r, Route::kStagedSegments);
    EXPECT_ROUTE(plan(wire, 512, true, 53), Route::kStridedSegments);
    // before: 700, 702
    EXPECT_ROUTE(plan(wire, 512, true, 17), Route::kPackets);
    EXPECT_ROUTE(plan(ragged(5), 512, true, 17), Route::kPackets);
    // before: 718-726: packet 39 ends at 40 slots, packet 40's data begins past the arena's end
    const uint64_t arena_len = 40 * kSlot + 100;
    r = plan(wire, 512, true, 0, &arena_len);
    EXPECT_ROUTE(r, Route::kOutOfBounds);
    CHECK(r.p.bad_index == 40, "bad index %zu", r.p.bad_index);
    const uint64_t whole = 64 * kSlot;
    EXPECT_ROUTE(plan(wire, 512, true, 0, &whole), Route::kPitchStream);
    // before: 718 (bad_index == null): no check at all
    EXPECT_ROUTE(plan(wire, 512, true, 0, nullptr), Route::kPitchStream);
    // the stream API's one-packet streams: the walk takes them at any 16-byte pitch, 0 included, with the
    // last packet's geometry (at R x 4096: its 4096-byte pieces); an unaligned pitch goes to descriptors
    const void *const data = reinterpret_cast<const void *>(uintptr_t(kArena + 512));
    const void *const words = reinterpret_cast<const void *>(uintptr_t(kArena));
    for (uint64_t pitch : {uint64_t(0), uint64_t(16), kSlot}) {
        PitchStream s;
        CHECK(plan_packet_stream(65536, 65536 - 300, 1, 512, data, words, pitch, true, 0, &s) && s.npk == 1 &&
                  s.last_len == 65536 - 300 && s.geom.upp == 16 && s.geom.lunits == 16 && s.geom.pk_len == 0,
              "one packet at pitch %llu: upp %u", (unsigned long long)pitch, s.geom.upp);
        CHECK(plan_packet_stream(65536, 65536 - 300, 1, 12288, data, words, pitch, true, 0, &s) && s.geom.upp == 15 &&
                  s.geom.lunits == 15 && s.geom.ltail == 4096 && s.geom.pk_len == 0,
              "one packet of 12 KiB chunks at pitch %llu: upp %u", (unsigned long long)pitch, s.geom.upp);
    }
    PitchStream s;
    CHECK(!plan_packet_stream(65536, 65536 - 300, 1, 512, data, words, 7, true, 0, &s), "one packet at pitch 7");
    CHECK(!plan_packet_stream(65536, 100, 1, 512, data, words, 0, true, 0, &s), "one packet without a whole chunk");
}

// ---- d. the round kernel's word policy ------------------------------------------------------------
// words_policy against the table of launches it has to reproduce (what launch_wave3 and the two kernels
// chose before the rule was written once), with the edges of its three run-time conditions
void check_words() {
    using W = Words;
    using K = WalkKind;
    constexpr uint64_t kGiB2 = uint64_t(1) << 31;
    struct Row {
        bool verify;
        K walk;
        int bpc, tpb;
        uint64_t units;
        uint32_t kq, kr;
        W want;
    };
    const Row rows[] = {
        // verify compares, whatever the walk, chunk size and launch size
        {true, K::kBlock, 512, 256, 8, 2, 0, W::kCompare},
        {true, K::kBlock, 4096, 1024, 1 << 20, 256, 0, W::kCompare},
        {true, K::kPitch, 1024, 512, 8192, 8, 0, W::kCompare},
        {true, K::kSeg, 512, 1024, 100000, 24, 1696, W::kCompare},
        // compute over a contiguous block
        {false, K::kBlock, 4096, 1024, 32768, 8, 0, W::kHold64},
        {false, K::kBlock, 4096, 1024, 1, 0, 1, W::kHold64},
        {false, K::kBlock, 1024, 1024, 32768, 8, 0, W::kStaged},
        {false, K::kBlock, 2048, 1024, 1 << 20, 256, 0, W::kStaged},  // past one window: in windows
        {false, K::kBlock, 512, 1024, 32768, 8, 0, W::kStaged},
        {false, K::kBlock, 512, 1024, 4096 * 32, 32, 0, W::kStaged},       // the longest wave has 32 rounds
        {false, K::kBlock, 512, 1024, 4096 * 31 + 5, 31, 5, W::kStaged},   // 31 + 1
        {false, K::kBlock, 512, 1024, 4096 * 32 + 1, 32, 1, W::kHold8},    // 32 + 1 = 33
        {false, K::kBlock, 512, 1024, 4096 * 33, 33, 0, W::kHold8},
        {false, K::kBlock, 1024, 1024, kGiB2 / 16 - 1, 131071, 4095, W::kStaged},  // words: 2^31 - 16 bytes
        {false, K::kBlock, 1024, 1024, kGiB2 / 16, 131072, 0, W::kPerRound},       // words: 2^31 bytes
        {false, K::kBlock, 2048, 1024, kGiB2 / 8 - 1, 262143, 4095, W::kStaged},
        {false, K::kBlock, 2048, 1024, kGiB2 / 8, 262144, 0, W::kPerRound},
        {false, K::kBlock, 512, 1024, kGiB2 / 32, 65536, 0, W::kHold8},
        {false, K::kBlock, 512, 256, 64, 1, 0, W::kHold8},       // smaller workgroups (lab only) cannot stage
        {false, K::kBlock, 1024, 512, 64, 1, 0, W::kPerRound},
        {false, K::kBlock, 2048, 256, 64, 1, 0, W::kPerRound},
        // compute over a packet stream
        {false, K::kPitch, 512, 256, 4096, 4, 0, W::kPerRound},
        {false, K::kPitch, 512, 512, 4097, 2, 1, W::kHold8},
        {false, K::kPitch, 512, 1024, 1 << 20, 256, 0, W::kHold8},
        {false, K::kPitch, 512, 256, 1, 0, 1, W::kPerRound},
        {false, K::kPitch, 1024, 256, 4096, 4, 0, W::kPerRound},
        {false, K::kPitch, 4096, 256, 16, 0, 16, W::kPerRound},
        {false, K::kPitch, 1024, 512, 4097, 2, 1, W::kPerRound},
        {false, K::kPitch, 2048, 1024, 1 << 20, 256, 0, W::kPerRound},
        {false, K::kPitch, 4096, 1024, 1 << 20, 256, 0, W::kPerRound},
        // compute over a segment list: held with per-lane addresses at bpc 512, at every launch size
        {false, K::kSeg, 512, 256, 16, 0, 16, W::kHold8},
        {false, K::kSeg, 512, 1024, 1 << 20, 256, 0, W::kHold8},
        {false, K::kSeg, 1024, 256, 16, 0, 16, W::kPerRound},
        {false, K::kSeg, 2048, 512, 8192, 8, 0, W::kPerRound},
        {false, K::kSeg, 4096, 1024, 1 << 20, 256, 0, W::kPerRound},
    };
    for (const Row &r : rows) {
        const W got = words_policy(r.verify, r.walk, r.bpc, r.tpb, r.units, r.kq, r.kr);
        CHECK(got == r.want, "verify %d walk %d bpc %d tpb %d units %llu kq %u kr %u: policy %d, want %d", int(r.verify),
              int(r.walk), r.bpc, r.tpb, (unsigned long long)r.units, r.kq, r.kr, int(got), int(r.want));
    }
    // the words of bpc 1024 at exactly 2^31 - 4 bytes: no whole number of rounds gives them (4 words per round),
    // so the condition itself at the byte: units * 16 < 2^31 holds up to the last round below and not at 2^31
    static_assert((kGiB2 / 16 - 1) * 16 + 12 == kGiB2 - 4, "the last round's last word ends 4 bytes below 2 GiB");
    static_assert(kStageMaxRounds(512) == 32 && kStageMaxRounds(1024) == 64 && kStageMaxRounds(2048) == 128, "windows");
    // what a launch of no known size gets (launch_wave3's other kernel, the segment kernel's only one)
    static_assert(words_policy(false, K::kBlock, 512, 1024, kAnyUnits, ~0u, 0) == W::kHold8, "");
    static_assert(words_policy(false, K::kBlock, 1024, 1024, kAnyUnits, ~0u, 0) == W::kPerRound, "");
    static_assert(words_policy(false, K::kSeg, 512, 1024, kAnyUnits, 0, 0) == W::kHold8, "");
}

}  // namespace

int main() {
    check_divide();
    check_walks();
    check_routes();
    check_words();
    if (g_failed) {
        std::printf("launch plan: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("launch plan ok\n");
    return 0;
}
