// CPU check of the gather planner (libhdfs3_amd/csrc/launch_plan.cpp: gather_first_bad,
// plan_gather_launch), built with the host compiler under ASan + UBSan by tests/test_gather_plan.py.
// The planner's launches are replayed by a host model of the kernel's work split (workgroup -> range by
// the tile prefix sums, lane -> 16-byte destination line), which must write every byte of every range
// exactly once and nothing else.
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

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

std::vector<GatherLaunch> plan_all(uint64_t dst_addr, const std::vector<CopyRange> &in) {
    std::vector<GatherLaunch> out;
    for (size_t pos = 0; pos < in.size();) {
        GatherLaunch g;
        const size_t next = plan_gather_launch(dst_addr, in.data(), in.size(), pos, &g);
        CHECK(next > pos, "no progress at %zu", pos);
        if (next <= pos) break;
        pos = next;
        if (g.n) out.push_back(g);
    }
    return out;
}

// ---- a. bounds -----------------------------------------------------------------------------------
void check_bounds() {
    const uint64_t S = 1000, D = 500;
    const CopyRange ok[] = {{0, 0, 500}, {999, 499, 1}, {1000, 500, 0}, {0, 0, 0}, {500, 0, 500}};
    CHECK(gather_first_bad(ok, 5, S, D) == 5, "all inside");
    CHECK(gather_first_bad(ok, 0, S, D) == 0, "empty list");
    const CopyRange bad_src[] = {{0, 0, 10}, {999, 0, 2}};
    CHECK(gather_first_bad(bad_src, 2, S, D) == 1, "source end");
    const CopyRange bad_dst[] = {{0, 499, 2}};
    CHECK(gather_first_bad(bad_dst, 1, S, D) == 0, "destination end");
    const CopyRange off_src[] = {{0, 0, 1}, {0, 0, 1}, {1001, 0, 0}};
    CHECK(gather_first_bad(off_src, 3, S, D) == 2, "empty range past the source");
    const CopyRange off_dst[] = {{0, 501, 0}};
    CHECK(gather_first_bad(off_dst, 1, S, D) == 0, "empty range past the destination");
    const CopyRange wrap[] = {{~uint64_t(0) - 3, 0, 8}, {0, ~uint64_t(0) - 3, 8}, {8, 0, ~uint64_t(0)}};
    for (int i = 0; i < 3; ++i) CHECK(gather_first_bad(wrap + i, 1, S, D) == 0, "wrapping range %d", i);
    CHECK(gather_first_bad(wrap, 1, ~uint64_t(0), ~uint64_t(0)) == 0, "offset + len wraps in a huge buffer");
    // a range of more tiles than a grid holds
    const CopyRange huge[] = {{0, 0, kGatherMaxTiles * kGatherTileBytes}};
    CHECK(gather_first_bad(huge, 1, ~uint64_t(0), ~uint64_t(0)) == 0, "too many tiles");
}

// ---- b. empty ranges, merging --------------------------------------------------------------------
void check_merge() {
    {
        const std::vector<CopyRange> in = {{0, 0, 0}, {5, 7, 0}};
        CHECK(plan_all(0x1000, in).empty(), "only empty ranges");
    }
    {
        // 0+1 contiguous on both sides; 2 continues the source only; 3 the destination only; an empty range
        // between two halves does not keep them apart; 5 runs backwards
        const std::vector<CopyRange> in = {{100, 10, 20}, {120, 30, 5}, {125, 40, 5},  {300, 45, 5},
                                           {305, 50, 3},  {0, 0, 0},    {308, 53, 2}, {290, 55, 10}};
        const auto L = plan_all(0x1003, in);
        CHECK(L.size() == 1, "%zu launches", L.size());
        if (L.size() == 1) {
            const GatherLaunch &g = L[0];
            CHECK(g.n == 4, "%u ranges", g.n);
            const CopyRange want[] = {{100, 10, 25}, {125, 40, 5}, {300, 45, 10}, {290, 55, 10}};
            for (uint32_t i = 0; i < g.n && i < 4; ++i)
                CHECK(g.r[i].src_off == want[i].src_off && g.r[i].dst_off == want[i].dst_off && g.r[i].len == want[i].len,
                      "range %u: %llu %llu %llu", i, (unsigned long long)g.r[i].src_off,
                      (unsigned long long)g.r[i].dst_off, (unsigned long long)g.r[i].len);
        }
    }
    {
        // a dense reader batch: 64 packets back to back on both sides -> one range, tiles by bytes
        std::vector<CopyRange> in;
        for (uint64_t i = 0; i < 64; ++i) in.push_back({4096 + i * 65536, i * 65536, 65536});
        const auto L = plan_all(0x7f0000000000ull, in);
        CHECK(L.size() == 1 && L[0].n == 1 && L[0].r[0].len == 64 * 65536, "dense batch");
        if (L.size() == 1) CHECK(L[0].tile_end[0] == 64 * 65536 / kGatherTileBytes, "%u tiles", L[0].tile_end[0]);
    }
}

// ---- c. the kernel's work split on the host -------------------------------------------------------
// every byte of every range written exactly once, by the workgroup the prefix sums assign
void replay(uint64_t dst_addr, uint64_t dst_len, const std::vector<CopyRange> &in, const char *what) {
    uint64_t want_bytes = 0;
    for (const CopyRange &c : in) want_bytes += c.len;
    std::vector<uint8_t> hit(dst_len, 0);
    uint64_t planned = 0, ranges = 0;
    for (const GatherLaunch &g : plan_all(dst_addr, in)) {
        CHECK(g.n >= 1 && g.n <= kGatherMaxRanges, "%s: %u ranges", what, g.n);
        ranges += g.n;
        uint32_t prev = 0;
        for (uint32_t i = 0; i < g.n; ++i) {
            CHECK(g.r[i].len > 0, "%s: empty range kept", what);
            CHECK(g.tile_end[i] - prev == gather_tiles(dst_addr + g.r[i].dst_off, g.r[i].len), "%s: tiles of range %u", what, i);
            CHECK(g.tile_end[i] > prev, "%s: prefix sums not increasing", what);
            prev = g.tile_end[i];
            planned += g.r[i].len;
        }
        for (uint32_t w = 0; w < g.tile_end[g.n - 1]; ++w) {
            uint32_t lo = 0, hi = g.n - 1;  // the kernel's search
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (g.tile_end[mid] > w) hi = mid;
                else lo = mid + 1;
            }
            const CopyRange &c = g.r[lo];
            const uint64_t lt = w - (lo ? g.tile_end[lo - 1] : 0);
            const uint64_t D = dst_addr + c.dst_off, line0 = D & ~uint64_t(15);
            const uint64_t t0 = line0 + lt * kGatherTileBytes, t1 = t0 + kGatherTileBytes;
            const uint64_t a0 = t0 > D ? t0 : D, a1 = t1 < D + c.len ? t1 : D + c.len;
            CHECK(a0 < a1, "%s: workgroup %u has no byte", what, w);
            for (uint64_t a = a0; a < a1; ++a) ++hit[a - dst_addr];
        }
    }
    CHECK(planned == want_bytes, "%s: %llu bytes planned of %llu", what, (unsigned long long)planned,
          (unsigned long long)want_bytes);
    std::vector<uint8_t> want(dst_len, 0);
    for (const CopyRange &c : in)
        for (uint64_t k = 0; k < c.len; ++k) ++want[c.dst_off + k];
    CHECK(hit == want, "%s: the workgroups' bytes are not the ranges' bytes", what);
    (void)ranges;
}

void check_split() {
    // more ranges than one launch carries, none mergeable (gaps in the destination), mixed with empties
    for (uint64_t align : {0, 1, 7, 15}) {
        std::vector<CopyRange> in;
        uint64_t d = 0;
        for (int i = 0; i < 3 * int(kGatherMaxRanges) + 5; ++i) {
            const uint64_t len = i % 11 == 3 ? 0 : 1 + rnd() % 40000;
            in.push_back({rnd() % 100000, d, len});
            d += len + 1 + rnd() % 3;
        }
        replay(0x10000 + align, d, in, "long list");
        uint64_t nonempty = 0;
        for (const CopyRange &c : in) nonempty += c.len != 0;
        const auto L = plan_all(0x10000 + align, in);
        uint64_t got = 0;
        for (const GatherLaunch &g : L) got += g.n;
        CHECK(got == nonempty, "%llu ranges planned of %llu", (unsigned long long)got, (unsigned long long)nonempty);
        CHECK(L.size() == (nonempty + kGatherMaxRanges - 1) / kGatherMaxRanges, "%zu launches", L.size());
    }
    // ranges abutting inside destination lines, every alignment, around the tile size
    for (uint64_t align = 0; align < 16; ++align)
        for (uint64_t len : {uint64_t(1), uint64_t(15), uint64_t(16), uint64_t(17), kGatherTileBytes - 1, kGatherTileBytes,
                             kGatherTileBytes + 1, 3 * kGatherTileBytes + 5}) {
            std::vector<CopyRange> in = {{7, 0, len}, {9000, len, len}, {3, 2 * len, 1}};
            replay(0x20000 + align, 2 * len + 1, in, "abutting");
        }
    // a launch closes at the grid limit: two ranges of more than half a grid's tiles
    {
        const uint64_t big = (kGatherMaxTiles / 2 + 10) * kGatherTileBytes;
        const std::vector<CopyRange> in = {{0, 0, big}, {0, big + 1, big}};
        CHECK(gather_first_bad(in.data(), 2, big, 2 * big + 1) == 2, "big ranges are valid");
        const auto L = plan_all(0, in);
        CHECK(L.size() == 2 && L[0].n == 1 && L[1].n == 1, "grid limit: %zu launches", L.size());
        // contiguous on both sides, but the merged range would not fit a grid: kept apart
        const std::vector<CopyRange> in2 = {{0, 0, big}, {big, big, big}};
        const auto L2 = plan_all(0, in2);
        CHECK(L2.size() == 2, "merge across the grid limit: %zu launches", L2.size());
    }
}

}  // namespace

int main() {
    check_bounds();
    check_merge();
    check_split();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("gather plan ok\n");
    return 0;
}
