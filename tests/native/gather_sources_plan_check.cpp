// CPU check of the planner for the gather with a source per range (libhdfs3_amd/csrc/launch_plan.cpp:
// gather_sources_first_bad, and plan_gather_launch over ranges whose src_off is an address), built with the
// host compiler under ASan + UBSan by tests/test_gather_sources_plan.py. Beside the destination-side checks
// of gather_plan_check.cpp, the launches are replayed by a host model of the kernel's LOADS: a workgroup's
// aligned 16-byte quads are taken only inside its own (planned) range, every other byte singly, and every
// address read must lie inside one of the caller's ranges.
#include <algorithm>
#include <cstdio>
#include <utility>
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

uint64_t rng_state = 0xD1B54A32D192ED03ull;
uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr uint64_t kMax = ~uint64_t(0);

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

// ---- a. bounds, wrap-around ----------------------------------------------------------------------
void check_bounds() {
    const uint64_t D = 500, A = 0x7f1200000000ull;
    const CopyRange ok[] = {{A, 0, 500}, {A + 7, 499, 1}, {0, 500, 0}, {0, 0, 0}, {kMax - 8, 0, 8}, {kMax, 3, 0}};
    CHECK(gather_sources_first_bad(ok, 6, D) == 6, "all inside");
    CHECK(gather_sources_first_bad(ok, 0, D) == 0, "empty list");
    const CopyRange bad_dst[] = {{A, 0, 10}, {A, 499, 2}};
    CHECK(gather_sources_first_bad(bad_dst, 2, D) == 1, "destination end");
    const CopyRange off_dst[] = {{A, 501, 0}};
    CHECK(gather_sources_first_bad(off_dst, 1, D) == 0, "empty range past the destination");
    const CopyRange wrap[] = {{kMax - 3, 0, 8}, {A, kMax - 3, 8}, {8, 0, kMax}, {kMax, 0, 2}};
    for (int i = 0; i < 4; ++i) CHECK(gather_sources_first_bad(wrap + i, 1, kMax) == 0, "wrapping range %d", i);
    const CopyRange third[] = {{A, 0, 1}, {A, 1, 1}, {kMax - 3, 2, 8}};
    CHECK(gather_sources_first_bad(third, 3, D) == 2, "the wrapping source is the third range");
    const CopyRange huge[] = {{A, 0, kGatherMaxTiles * kGatherTileBytes}};
    CHECK(gather_sources_first_bad(huge, 1, kMax) == 0, "too many tiles");
    const CopyRange fits[] = {{A, 0, (kGatherMaxTiles - 1) * kGatherTileBytes}};
    CHECK(gather_sources_first_bad(fits, 1, kMax) == 1, "the longest range a grid holds");
}

// ---- b. empty ranges, merging of address-adjacent ranges -----------------------------------------
void check_merge() {
    const uint64_t A = 0x7f1200000100ull, B = 0x7f5500000000ull;
    {
        const std::vector<CopyRange> in = {{0, 0, 0}, {A, 7, 0}};
        CHECK(plan_all(0x1000, in).empty(), "only empty ranges");
    }
    {
        // 0+1 adjacent in address and destination; 2 continues the address only; 3 the destination only (another
        // allocation); 4 and 6 adjacent around an empty entry with a null address; 7 runs backwards
        const std::vector<CopyRange> in = {{A, 10, 20},    {A + 20, 30, 5}, {A + 25, 40, 5}, {B, 45, 5},
                                           {B + 5, 50, 3}, {0, 0, 0},       {B + 8, 53, 2},  {A - 10, 55, 10}};
        const auto L = plan_all(0x1003, in);
        CHECK(L.size() == 1, "%zu launches", L.size());
        if (L.size() == 1) {
            const GatherLaunch &g = L[0];
            CHECK(g.n == 4, "%u ranges", g.n);
            const CopyRange want[] = {{A, 10, 25}, {A + 25, 40, 5}, {B, 45, 10}, {A - 10, 55, 10}};
            for (uint32_t i = 0; i < g.n && i < 4; ++i)
                CHECK(g.r[i].src_off == want[i].src_off && g.r[i].dst_off == want[i].dst_off && g.r[i].len == want[i].len,
                      "range %u: %llx %llu %llu", i, (unsigned long long)g.r[i].src_off,
                      (unsigned long long)g.r[i].dst_off, (unsigned long long)g.r[i].len);
        }
    }
    {
        // 200 entries of 100 bytes back to back in memory and in the destination: one range, one launch
        std::vector<CopyRange> in;
        for (uint64_t i = 0; i < 200; ++i) in.push_back({A + 3 + i * 100, 48 + i * 100, 100});
        const auto L = plan_all(0x7f0000000000ull, in);
        CHECK(L.size() == 1 && L[0].n == 1 && L[0].r[0].len == 20000 && L[0].r[0].src_off == A + 3, "adjacent entries");
        if (L.size() == 1) CHECK(L[0].tile_end[0] == gather_tiles(0x7f0000000000ull + 48, 20000), "%u tiles", L[0].tile_end[0]);
        // the same with a byte between them in memory: 200 ranges, 4 launches
        for (uint64_t i = 0; i < 200; ++i) in[i].src_off += i;
        const auto L2 = plan_all(0x7f0000000000ull, in);
        CHECK(L2.size() == 4 && L2[0].n == 64 && L2[3].n == 8, "entries with gaps: %zu launches", L2.size());
    }
}

// ---- c. the kernel's work split and its loads on the host -----------------------------------------
// every destination byte of every range written exactly once and from the right address, and every address the
// model loads lies inside the workgroup's own planned range (so inside the caller's ranges it was merged from)
void replay(uint64_t dst_addr, uint64_t dst_len, const std::vector<CopyRange> &in, const char *what) {
    std::vector<std::pair<uint64_t, uint64_t>> spans, allowed;  // the union of the caller's source bytes: [first, end)
    for (const CopyRange &c : in)
        if (c.len) spans.push_back({c.src_off, c.src_off + c.len});
    std::sort(spans.begin(), spans.end());
    for (const auto &sp : spans) {
        if (!allowed.empty() && sp.first <= allowed.back().second) allowed.back().second = std::max(allowed.back().second, sp.second);
        else allowed.push_back(sp);
    }
    auto readable = [&](uint64_t a, uint64_t n) {
        auto it = std::upper_bound(allowed.begin(), allowed.end(), std::make_pair(a, ~uint64_t(0)));
        return it != allowed.begin() && (--it)->first <= a && a + n <= it->second;
    };
    std::vector<uint8_t> hit(dst_len, 0);
    std::vector<uint64_t> from(dst_len, 0);
    uint64_t planned = 0, want_bytes = 0;
    for (const CopyRange &c : in) want_bytes += c.len;
    for (const GatherLaunch &g : plan_all(dst_addr, in)) {
        CHECK(g.n >= 1 && g.n <= kGatherMaxRanges, "%s: %u ranges", what, g.n);
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
            const uint64_t D = dst_addr + c.dst_off, S = c.src_off, src_e = S + c.len, line0 = D & ~uint64_t(15);
            const uint64_t delta = S - D, k = delta & 15;
            bool any = false;
            for (uint64_t idx = 0; idx < kGatherTileBytes / 16; ++idx) {
                const uint64_t line = line0 + (lt * (kGatherTileBytes / 16) + idx) * 16;
                const uint64_t q = line + delta - k;
                const bool fast = line >= D && line + 16 <= D + c.len && q >= S && q + (k ? 32 : 16) <= src_e;
                if (fast) CHECK(readable(q, k ? 32 : 16), "%s: a quad load leaves the caller's ranges", what);
                const uint64_t a0 = line > D ? line : D, a1 = line + 16 < D + c.len ? line + 16 : D + c.len;
                for (uint64_t a = a0; a < a1; ++a) {
                    any = true;
                    if (!fast) CHECK(readable(a + delta, 1), "%s: a byte load leaves the caller's ranges", what);
                    ++hit[a - dst_addr];
                    from[a - dst_addr] = a + delta;
                }
            }
            CHECK(any, "%s: workgroup %u has no byte", what, w);
        }
    }
    CHECK(planned == want_bytes, "%s: %llu bytes planned of %llu", what, (unsigned long long)planned,
          (unsigned long long)want_bytes);
    std::vector<uint8_t> want(dst_len, 0);
    std::vector<uint64_t> want_from(dst_len, 0);
    for (const CopyRange &c : in)
        for (uint64_t i = 0; i < c.len; ++i) ++want[c.dst_off + i], want_from[c.dst_off + i] = c.src_off + i;
    CHECK(hit == want, "%s: the workgroups' bytes are not the ranges' bytes", what);
    CHECK(from == want_from, "%s: a byte comes from the wrong address", what);
}

void check_split() {
    // more ranges than one launch carries, sources in three "allocations" in turn at every misalignment, none
    // mergeable (gaps in the destination), mixed with empties
    const uint64_t base[3] = {0x7f1200000000ull, 0x7f3400001000ull, 0x7f5600002000ull};
    for (uint64_t align : {0, 1, 7, 15}) {
        std::vector<CopyRange> in;
        uint64_t d = 0;
        for (int i = 0; i < 3 * int(kGatherMaxRanges) + 7; ++i) {
            const uint64_t len = i % 11 == 3 ? 0 : 1 + rnd() % 40000;
            in.push_back({len ? base[i % 3] + rnd() % 100000 : 0, d, len});
            d += len + 1 + rnd() % 3;
        }
        CHECK(gather_sources_first_bad(in.data(), in.size(), d) == in.size(), "long list is valid");
        replay(0x10000 + align, d, in, "long list");
        uint64_t nonempty = 0;
        for (const CopyRange &c : in) nonempty += c.len != 0;
        const auto L = plan_all(0x10000 + align, in);
        uint64_t got = 0;
        for (const GatherLaunch &g : L) got += g.n;
        CHECK(got == nonempty, "%llu ranges planned of %llu", (unsigned long long)got, (unsigned long long)nonempty);
        CHECK(L.size() == (nonempty + kGatherMaxRanges - 1) / kGatherMaxRanges, "%zu launches", L.size());
    }
    // all 16 x 16 misalignments, short ranges and ranges around the tile size, abutting in the destination
    for (uint64_t sa = 0; sa < 16; ++sa)
        for (uint64_t da = 0; da < 16; ++da)
            for (uint64_t len : {uint64_t(1), uint64_t(15), uint64_t(16), uint64_t(17), uint64_t(33), kGatherTileBytes - 1,
                                 kGatherTileBytes, kGatherTileBytes + 1}) {
                std::vector<CopyRange> in = {{base[0] + sa, 0, len}, {base[1] + 9000 + sa, len, len}, {base[2] + 3, 2 * len, 1}};
                replay(0x20000 + da, 2 * len + 1, in, "abutting");
            }
    // adjacent entries merge and the merged range is its own source: still no load outside the entries
    {
        std::vector<CopyRange> in;
        uint64_t d = 5;
        for (uint64_t i = 0; i < 40; ++i) {
            in.push_back({base[0] + 11 + i * 100, d, 100});
            d += 100;
        }
        replay(0x30000 + 9, d, in, "merged");
    }
    // a launch closes at the grid limit
    {
        const uint64_t big = (kGatherMaxTiles / 2 + 10) * kGatherTileBytes;
        const std::vector<CopyRange> in = {{base[0], 0, big}, {base[1], big + 1, big}};
        CHECK(gather_sources_first_bad(in.data(), 2, 2 * big + 1) == 2, "big ranges are valid");
        const auto L = plan_all(0, in);
        CHECK(L.size() == 2 && L[0].n == 1 && L[1].n == 1, "grid limit: %zu launches", L.size());
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
    std::printf("gather sources plan ok\n");
    return 0;
}
