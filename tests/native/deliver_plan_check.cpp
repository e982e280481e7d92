// CPU check of the guarded delivery's arithmetic (libhdfs3_amd/csrc/launch_plan.h: deliver_limit,
// deliver_clip, deliver_gate, shared by the kernel and the host) and of the planner as the delivery uses
// it, built with the host compiler under ASan + UBSan by tests/test_deliver_plan.py. A host model of the
// kernel (every planned range clipped to the limit) must write exactly the bytes below the limit.
#include <cstdio>
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

constexpr uint64_t bad(uint64_t chunk) { return ~chunk; }  // a verify's result word

// the arithmetic is usable in constant expressions (it is compiled into the kernel as is)
static_assert(deliver_limit(0, 0, 512, 2048, 512) == kDeliverNoLimit, "clean");
static_assert(deliver_limit(bad(5), 0, 512, 2048, 512) == 512 + 2048, "chunk 5 of 512 in granules of 2048");
static_assert(deliver_clip(100, 40, 100) == 60 && deliver_clip(100, 100, 5) == 0 && deliver_clip(100, 0, 7) == 7, "clip");

void check_limit() {
    // result 0: no limit, whatever the rest
    CHECK(deliver_limit(0, 0, 0, 1, 1) == kDeliverNoLimit, "clean");
    CHECK(deliver_limit(0, 0, ~uint64_t(0), ~uint64_t(0), ~uint32_t(0)) == kDeliverNoLimit, "clean, extreme guard");
    // a closed gate: nothing, whatever the result
    CHECK(deliver_limit(0, 1, 512, 2048, 512) == 0, "gate closed, clean result");
    CHECK(deliver_limit(bad(9), bad(3), 512, 2048, 512) == 0, "gate closed, bad result");
    CHECK(deliver_limit(0, ~uint64_t(0), 0, 1, 1) == 0, "gate of all ones");
    // bad chunk 0: the limit is data_off itself
    CHECK(deliver_limit(bad(0), 0, 0, 2048, 512) == 0, "chunk 0");
    CHECK(deliver_limit(bad(0), 0, 512, 2048, 512) == 512, "chunk 0 behind data_off");
    // the middle of a granule and a granule's start (granule 2048 = 4 chunks of 512)
    CHECK(deliver_limit(bad(3), 0, 0, 2048, 512) == 0, "chunk 3: granule 0");
    CHECK(deliver_limit(bad(4), 0, 0, 2048, 512) == 2048, "chunk 4: start of granule 1");
    CHECK(deliver_limit(bad(6), 0, 0, 2048, 512) == 2048, "chunk 6: middle of granule 1");
    CHECK(deliver_limit(bad(16), 0, 512, 2048, 512) == 512 + 8192, "chunk 16 behind data_off");
    // granule = bpc: chunk granularity
    for (uint64_t k : {uint64_t(0), uint64_t(1), uint64_t(7), uint64_t(1000003)})
        CHECK(deliver_limit(bad(k), 0, 40, 512, 512) == 40 + k * 512, "chunk granularity, chunk %llu", (unsigned long long)k);
    // a granule that is no multiple of bpc: the granule holding the bad chunk's FIRST byte is withheld
    CHECK(deliver_limit(bad(1), 0, 0, 1000, 512) == 0, "chunk 1 starts at 512: granule 0");
    CHECK(deliver_limit(bad(2), 0, 0, 1000, 512) == 1000, "chunk 2 starts at 1024: granule 1");
    CHECK(deliver_limit(bad(4), 0, 7, 1000, 512) == 7 + 2000, "chunk 4 starts at 2048: granule 2, behind data_off");
    CHECK(deliver_limit(bad(5), 0, 0, 3, 7) == 33, "bpc 7, granule 3: chunk 5 starts at 35");
    // a granule larger than everything before the bad chunk
    CHECK(deliver_limit(bad(100), 0, 64, uint64_t(1) << 40, 4096) == 64, "huge granule");
    // near 2^63 and beyond: exact while it fits 64 bits, saturated (never wrapped) when it does not
    const uint64_t two62 = uint64_t(1) << 62, two63 = uint64_t(1) << 63;
    CHECK(deliver_limit(bad(two62), 0, 0, 2, 2) == two63, "2^62 chunks of 2");
    CHECK(deliver_limit(bad(two63 - 1), 0, 0, 1, 1) == two63 - 1, "2^63 - 1 chunks of 1");
    CHECK(deliver_limit(bad(two63 - 1), 0, two63, 1, 1) == ~uint64_t(0), "2^63 - 1 behind 2^63");
    CHECK(deliver_limit(bad(two63), 0, two63, 1, 1) == kDeliverNoLimit, "sum wraps: saturated");
    CHECK(deliver_limit(bad(two63), 0, 0, 1, 2) == kDeliverNoLimit, "product wraps: saturated");
    CHECK(deliver_limit(bad((uint64_t(1) << 53) + 3), 0, 1, 1 << 20, 1 << 10) == 1 + ((uint64_t(1) << 63) + 3072) / (1 << 20) * (1 << 20),
          "2^53 + 3 chunks of 1024");
    CHECK(deliver_limit(bad(~uint64_t(0) - 1), 0, 0, 1, 1) == ~uint64_t(0) - 1, "the largest chunk index a word holds");
    CHECK(deliver_limit(bad(~uint64_t(0) - 1), 0, 0, 4096, ~uint32_t(0)) == kDeliverNoLimit, "and with the largest bpc");
    // the largest granule
    CHECK(deliver_limit(bad(two62), 0, 9, ~uint64_t(0), 2) == 9, "granule 2^64 - 1");
}

void check_clip_and_gate() {
    CHECK(deliver_clip(kDeliverNoLimit, 0, 10) == 10, "no limit");
    CHECK(deliver_clip(kDeliverNoLimit, kDeliverNoLimit - 1, 1) == 1, "no limit, last byte");
    CHECK(deliver_clip(0, 0, 10) == 0, "limit 0");
    CHECK(deliver_clip(2560, 2000, 1000) == 560, "straddling");
    CHECK(deliver_clip(2560, 2560, 1000) == 0, "starts at the limit");
    CHECK(deliver_clip(2560, 3000, 1000) == 0, "past the limit");
    CHECK(deliver_clip(2560, 1000, 1560) == 1560, "ends at the limit");
    CHECK(deliver_clip(2560, 1000, 0) == 0, "empty");
    CHECK(deliver_clip(uint64_t(1) << 63, (uint64_t(1) << 63) - 5, ~uint64_t(0)) == 5, "huge length");

    CHECK(deliver_gate(0, 0, 1000) == 0, "clean: open");
    CHECK(deliver_gate(bad(3), 0, 1000) == bad(1003), "bad: closed with chunk_base + chunk");
    CHECK(deliver_gate(bad(0), 0, 0) == bad(0) && bad(0) != 0, "chunk 0 closes the gate");
    CHECK(deliver_gate(0, bad(77), 1000) == bad(77), "closed stays closed");
    CHECK(deliver_gate(bad(3), bad(77), 1000) == bad(77), "closed stays closed over a bad result");
    CHECK(deliver_gate(bad((uint64_t(1) << 62)), 0, uint64_t(1) << 62) == bad(uint64_t(1) << 63), "2^62 + 2^62");
}

// the kernel on the host: every planned range clipped, its bytes counted
void check_planned_delivery() {
    const uint64_t dst_addr = 0x7f0000000003ull, src_len = 9000, dst_len = 20000;
    std::vector<CopyRange> in;
    for (uint64_t i = 0; i < 70; ++i) in.push_back({100 * i + 7, 200 * i + 1, 1});  // two launches, none merges
    in.push_back({0, 15000, 4096});      // contiguous with the next on both sides: merged by the planner,
    in.push_back({4096, 19096, 800});    // and clipped as one range
    in.push_back({8000, 14500, 0});
    CHECK(gather_first_bad(in.data(), in.size(), src_len, dst_len) == in.size(), "ranges are valid");
    for (uint64_t limit : {uint64_t(0), uint64_t(8), uint64_t(3508), uint64_t(4096), uint64_t(4500), uint64_t(6907), kDeliverNoLimit}) {
        std::vector<int> want(dst_len, 0), hit(dst_len, 0);
        for (const CopyRange &c : in)
            for (uint64_t b = 0; b < c.len; ++b)
                if (c.src_off + b < limit) ++want[c.dst_off + b];
        size_t launches = 0;
        for (size_t pos = 0; pos < in.size();) {
            GatherLaunch g;
            pos = plan_gather_launch(dst_addr, in.data(), in.size(), pos, &g);
            if (!g.n) continue;
            ++launches;
            for (uint32_t i = 0; i < g.n; ++i) {
                const uint64_t n = deliver_clip(limit, g.r[i].src_off, g.r[i].len);
                CHECK(n <= g.r[i].len, "clip grows a range");
                for (uint64_t b = 0; b < n; ++b) ++hit[g.r[i].dst_off + b];
            }
        }
        CHECK(launches == 2, "%zu launches", launches);
        CHECK(hit == want, "limit %llu: the clipped ranges are not the bytes below the limit", (unsigned long long)limit);
    }
}

}  // namespace

int main() {
    check_limit();
    check_clip_and_gate();
    check_planned_delivery();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("deliver plan ok\n");
    return 0;
}
