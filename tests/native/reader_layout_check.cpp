// CPU check of the block reader's batch geometry (libhdfs3_amd/csrc/client/reader_layout.h), built with
// the host compiler under ASan + UBSan by tests/test_reader_layout.py against that header alone: no GPU
// runtime, no socket, no receiver thread. The expected figures are derived from the reader's rules
// (dense: words from 0, data from a 4 KiB-rounded d0; wire: [words][data] with 16-byte aligned data),
// not measured.
#include <cstdio>
#include <vector>

#include "client/reader_layout.h"

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

constexpr uint64_t kKiB = 1024, kMiB = 1024 * 1024;

uint64_t crc_len_of(uint64_t data_len, uint32_t bpc) { return (data_len + bpc - 1) / bpc * 4; }

// What receive() does with one packet: open an empty batch, place, commit unless the batch closes.
// Returns false when the batch closed. *grown: the capacity the reader would have grown the arena to.
bool feed(BatchLayout &l, uint32_t data_len, uint32_t bpc, int batch_packets, bool dense, uint64_t *cap,
          Placement *out = nullptr, uint64_t *grown = nullptr) {
    const uint64_t crc_len = crc_len_of(data_len, bpc);
    if (l.pk.empty()) l.open(data_len, bpc, 4, batch_packets, dense);
    const Placement p = l.place(data_len, crc_len, *cap);
    if (out) *out = p;
    if (p.close) return false;
    if (p.need > *cap) {
        CHECK(l.pk.empty(), "only a batch's first packet may grow the arena (need %llu, cap %llu)",
              (unsigned long long)p.need, (unsigned long long)*cap);
        *cap = p.need;
        if (grown) *grown = p.need;
    }
    CHECK(p.crc_off + crc_len <= *cap && p.data_off + data_len <= *cap, "placement outside the arena");
    l.commit(p, data_len, 0, data_len);
    return true;
}

void dense_cases() {
    {  // default ring: 64 packets of 64 KiB at bpc 512 in 64 x 66,064 bytes
        BatchLayout l;
        uint64_t cap = ring_arena_bytes(64);
        CHECK(cap == 4228096, "ring arena %llu", (unsigned long long)cap);
        for (int i = 0; i < 64; ++i) {
            Placement p;
            CHECK(feed(l, 64 * kKiB, 512, 64, true, &cap, &p), "packet %d closed the batch", i);
            CHECK(p.crc_off == 512u * i && p.data_off == 32768 + 65536u * i, "packet %d at %llu / %llu", i,
                  (unsigned long long)p.crc_off, (unsigned long long)p.data_off);
        }
        CHECK(l.d0 == 32768 && l.used == 4227072 && cap == 4228096 && !l.sealed, "d0 %llu used %llu",
              (unsigned long long)l.d0, (unsigned long long)l.used);
        CHECK(l.chunk0.size() == 64 && l.chunk0[63] == 63 * 128, "chunk0");
    }
    {  // 256 KiB packets in the same arena: 15 fit, the 16th closes the batch, the arena stays
        BatchLayout l;
        uint64_t cap = ring_arena_bytes(64);
        int placed = 0;
        while (feed(l, 256 * kKiB, 512, 64, true, &cap)) ++placed;
        CHECK(l.d0 == 131072 && placed == 15 && cap == ring_arena_bytes(64), "d0 %llu placed %d",
              (unsigned long long)l.d0, placed);
    }
    {  // a short first packet keeps the word region, seals the batch; the next packet closes it
        BatchLayout l;
        uint64_t cap = ring_arena_bytes(64);
        CHECK(feed(l, 100, 512, 64, true, &cap), "first packet");
        CHECK(l.d0 == 32768 && l.sealed && l.words_used == 4 && l.used == 32768 + 100, "d0 %llu",
              (unsigned long long)l.d0);
        CHECK(!feed(l, 64 * kKiB, 512, 64, true, &cap), "a sealed batch took another packet");
    }
    for (uint32_t bpc : {4096u, 65536u}) {  // large chunk sizes: the word region is one 4 KiB page
        BatchLayout l;
        uint64_t cap = ring_arena_bytes(64);
        CHECK(feed(l, 64 * kKiB, bpc, 64, true, &cap), "first packet");
        CHECK(l.d0 == 4096, "bpc %u d0 %llu", bpc, (unsigned long long)l.d0);
    }
    {  // the word-region bound: one 64 KiB packet, then 128 KiB packets in 16 MiB
        BatchLayout l;
        uint64_t cap = 16 * kMiB;
        CHECK(feed(l, 64 * kKiB, 512, 64, true, &cap), "first packet");
        int placed = 1;
        Placement p{};
        while (feed(l, 128 * kKiB, 512, 64, true, &cap, &p)) ++placed;
        CHECK(l.d0 == 32768 && placed == 32 && l.words_used == 32256, "placed %d words %llu", placed,
              (unsigned long long)l.words_used);
        CHECK(p.close && p.need <= cap && l.words_used + 1024 > l.d0, "closed by something else than the word region");
    }
    {  // growth: one 16 MiB packet in a one-packet batch
        BatchLayout l;
        uint64_t cap = ring_arena_bytes(1), grown = 0;
        CHECK(feed(l, 16 * kMiB, 512, 1, true, &cap, nullptr, &grown), "first packet");
        CHECK(l.d0 == 131072 && grown == 131072 + 16777216, "grown to %llu", (unsigned long long)grown);
    }
}

void wire_cases() {
    const uint32_t bpc = 3, len = 4096;
    const uint64_t crc_len = crc_len_of(len, bpc);
    CHECK(crc_len == 5464, "crc_len %llu", (unsigned long long)crc_len);
    {
        BatchLayout l;
        uint64_t cap = ring_arena_bytes(64);
        Placement p;
        CHECK(feed(l, len, bpc, 64, false, &cap, &p) && p.crc_off == 8 && p.data_off == 5472, "first packet");
        CHECK(feed(l, len, bpc, 64, false, &cap, &p) && p.crc_off == 9576 && p.data_off == 15040, "second packet");
        for (int i = 2; i < 64; ++i) CHECK(feed(l, len + i, bpc, 64, false, &cap, &p), "packet %d", i);
        for (const PacketRef &r : l.pk)
            CHECK(r.data_off % 16 == 0 && r.crc_off + crc_len_of(r.data_len, bpc) == r.data_off, "alignment");
        CHECK(l.used == l.pk.back().data_off + l.pk.back().data_len && !l.sealed && l.chunk0.empty(), "used");
    }
    {  // a packet that does not fit a non-empty batch closes it; the arena stays
        BatchLayout l;
        uint64_t cap = 20000;
        CHECK(feed(l, len, bpc, 64, false, &cap) && feed(l, len, bpc, 64, false, &cap), "two packets fit");
        Placement p;
        CHECK(!feed(l, len, bpc, 64, false, &cap, &p) && p.close && cap == 20000 && l.pk.size() == 2, "third packet");
    }
    {  // a packet that does not fit an empty batch grows the arena to size + 64 and is placed first
        BatchLayout l;
        uint64_t cap = 1000, grown = 0;
        Placement p;
        CHECK(feed(l, len, bpc, 64, false, &cap, &p, &grown), "first packet");
        CHECK(grown == crc_len + len + 64 && p.crc_off == 8 && p.data_off == 5472, "grown to %llu",
              (unsigned long long)grown);
    }
}

void result_mapping() {
    BatchLayout d;
    uint64_t cap = ring_arena_bytes(64);
    for (int i = 0; i < 3; ++i) feed(d, 64 * kKiB, 512, 64, true, &cap);
    CHECK(d.chunk0 == (std::vector<uint64_t>{0, 128, 256}), "chunk0");
    CHECK(d.bad_packet(~127ull) == 0 && d.bad_packet(~128ull) == 1 && d.bad_packet(~300ull) == 2, "dense mapping");
    BatchLayout w;
    w.open(4096, 3, 4, 64, false);
    CHECK(w.bad_packet(~((5ull << 32) | 3)) == 5, "wire mapping");
}

// split_result_key (launch_plan.h): the word holds ~key, and 0 means nothing bad
void result_key_cases() {
    int64_t hi = 7, lo = 7;
    split_result_key(0, &hi, &lo);
    CHECK(hi == -1 && lo == -1, "raw 0: %lld / %lld", (long long)hi, (long long)lo);
    split_result_key(~0ull, &hi, &lo);  // key 0: the first chunk of the first packet
    CHECK(hi == 0 && lo == 0, "key 0: %lld / %lld", (long long)hi, (long long)lo);
    split_result_key(~((5ull << 32) | 3), &hi, &lo);
    CHECK(hi == 5 && lo == 3, "both halves: %lld / %lld", (long long)hi, (long long)lo);
    // the largest key a non-zero word can hold (~1); the key of all ones would read as raw 0
    split_result_key(1, &hi, &lo);
    CHECK(hi == 0xFFFFFFFFll && lo == 0xFFFFFFFEll, "largest key: %lld / %lld", (long long)hi, (long long)lo);
    hi = lo = 7;
    split_result_key(~(9ull << 32), &hi, nullptr);
    split_result_key(~4ull, nullptr, &lo);
    CHECK(hi == 9 && lo == 4, "one half at a time: %lld / %lld", (long long)hi, (long long)lo);
}

void cursor_cases() {
    BatchLayout l;
    l.open(512, 512, 4, 8, true);
    const uint32_t skip[3] = {17, 0, 0}, deliver[3] = {495, 512, 100}, data_len[3] = {512, 512, 100};
    for (int i = 0; i < 3; ++i)
        l.commit(l.place(data_len[i], crc_len_of(data_len[i], 512), 1 << 20), data_len[i], skip[i], deliver[i]);
    // byte k of the delivery is at this arena offset
    std::vector<uint64_t> want;
    for (const PacketRef &p : l.pk)
        for (uint32_t k = 0; k < p.deliver; ++k) want.push_back(p.data_off + p.skip + k);
    CHECK(want.size() == 1107, "%zu bytes", want.size());
    for (size_t step : {size_t(1), size_t(600), size_t(7), size_t(4096)})
        for (size_t limit : {size_t(3), size_t(2), size_t(0)}) {
            const size_t total = limit == 3 ? 1107 : limit == 2 ? 1007 : 0;
            DeliveryCursor c;
            size_t got = 0;
            while (!c.done(limit)) {
                CHECK(c.remaining(l.pk, limit) == int64_t(total - got), "remaining at %zu (step %zu)", got, step);
                const DeliveryCursor::Piece pc = c.take(l.pk, step);
                CHECK(pc.n > 0 && pc.n <= step && got + pc.n <= total, "piece of %zu at %zu", pc.n, got);
                if (got + pc.n > total) break;
                CHECK(pc.src == want[got] && pc.src + pc.n - 1 == want[got + pc.n - 1], "piece at %zu (step %zu)", got, step);
                got += pc.n;
            }
            CHECK(got == total && c.remaining(l.pk, limit) == 0, "walked %zu of %zu (step %zu)", got, total, step);
        }
}

}  // namespace

int main() {
    CHECK(kPacketGuess == 66064 && batch_payload_bytes(64) == 4 * int64_t(kMiB), "sizing");
    CHECK(arena_pinned_bytes(64) == 64 * int64_t(66064 + sizeof(DevSegment)) + 8, "pinned bytes");
    dense_cases();
    wire_cases();
    result_mapping();
    result_key_cases();
    cursor_cases();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("reader layout ok\n");
    return 0;
}
