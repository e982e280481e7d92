// CPU check of the output stream's batch ledger (libhdfs3_amd/csrc/client/batch_ledger.cpp), built with
// the host compiler under ASan + UBSan by tests/test_write_ledger.py; links the ledger alone.
// A scenario records host-written and device-placed ranges of an arena. A byte model then replays what
// dispatch does with the ledger's answers: the device arena starts stale and holds the placed bytes, the
// host arena holds the host's bytes and is stale elsewhere; the uploads are applied, then the downloads.
// Afterwards both arenas must hold every recorded byte, so no upload may cross a placed byte and no
// download a host byte that was not uploaded. The lists must also be ascending, disjoint and as short as
// the interleaving allows (one copy per run of one kind).
#include <cstdio>
#include <cstring>
#include <vector>

#include "client/batch_ledger.h"

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

enum : uint8_t { kNone = 0, kHost = 1, kDev = 2 };
constexpr uint8_t kStaleHost = 0xEE, kStaleDev = 0xDD;

struct Op {
    uint8_t kind;  // kHost / kDev
    uint64_t off, len;
};

uint8_t value_at(uint64_t off, uint8_t kind) { return uint8_t(1 + (off * 7 + kind * 101) % 200); }

// Feeds ops to a ledger, then checks its answers against the byte model. Returns the number of uploads.
size_t run(const char *name, BatchLedger &lg, const std::vector<Op> &ops, uint64_t arena, size_t *n_down = nullptr) {
    std::vector<uint8_t> owner(arena, kNone), h(arena, kStaleHost), d(arena, kStaleDev);
    for (const Op &o : ops) {
        if (o.kind == kHost) lg.host(o.off, o.len);
        else lg.device(o.off, o.len);
        for (uint64_t i = o.off; i < o.off + o.len; ++i) {
            owner[i] = o.kind;
            (o.kind == kHost ? h : d)[i] = value_at(i, o.kind);
        }
    }
    bool any_h = false, any_d = false;
    size_t runs[3] = {0, 0, 0};  // maximal runs of one kind, bytes nobody wrote skipped
    uint8_t last = kNone;
    for (uint64_t i = 0; i < arena; ++i) {
        if (owner[i] == kNone) continue;
        any_h |= owner[i] == kHost;
        any_d |= owner[i] == kDev;
        if (owner[i] != last) ++runs[owner[i]];
        last = owner[i];
    }
    CHECK(lg.any_host() == any_h, "%s: any_host", name);
    CHECK(lg.any_device() == any_d, "%s: any_device (the D2H decision)", name);

    std::vector<ByteRange> up, down;
    lg.uploads(&up);
    lg.downloads(&down);
    const std::vector<ByteRange> *lists[2] = {&up, &down};
    for (int k = 0; k < 2; ++k) {
        uint64_t prev_end = 0;
        for (size_t i = 0; i < lists[k]->size(); ++i) {
            const ByteRange &r = (*lists[k])[i];
            CHECK(r.len > 0, "%s: list %d range %zu is empty", name, k, i);
            CHECK(r.off + r.len <= arena, "%s: list %d range %zu leaves the arena", name, k, i);
            CHECK(i == 0 || r.off > prev_end, "%s: list %d range %zu not ascending / abuts", name, k, i);
            prev_end = r.off + r.len;
            // begins and ends on a byte of its own kind: no copy is longer than it has to be
            if (r.len && r.off + r.len <= arena) {
                const uint8_t want = k == 0 ? kHost : kDev;
                CHECK(owner[r.off] == want && owner[r.off + r.len - 1] == want, "%s: list %d range %zu ends", name, k, i);
            }
        }
    }
    CHECK(up.size() == runs[kHost], "%s: %zu uploads for %zu host runs", name, up.size(), runs[kHost]);
    CHECK(down.size() == runs[kDev], "%s: %zu downloads for %zu device runs", name, down.size(), runs[kDev]);
    if (!any_d && any_h) {  // the pure-host batch: the one upload from its first byte to its last
        uint64_t lo = 0, hi = arena;
        while (owner[lo] != kHost) ++lo;
        while (owner[hi - 1] != kHost) --hi;
        CHECK(up.size() == 1 && up[0].off == lo && up[0].len == hi - lo, "%s: the host-only upload", name);
        CHECK(down.empty(), "%s: a host-only batch copies nothing back", name);
    }

    for (const ByteRange &r : up)
        if (r.off + r.len <= arena) std::memcpy(d.data() + r.off, h.data() + r.off, r.len);
    for (uint64_t i = 0; i < arena; ++i)
        if (owner[i] != kNone && d[i] != value_at(i, owner[i])) {
            CHECK(false, "%s: device arena byte %llu (kind %d) wrong after the uploads", name, (unsigned long long)i,
                  owner[i]);
            break;
        }
    for (const ByteRange &r : down)
        if (r.off + r.len <= arena) std::memcpy(h.data() + r.off, d.data() + r.off, r.len);
    for (uint64_t i = 0; i < arena; ++i)
        if (owner[i] != kNone && h[i] != value_at(i, owner[i])) {
            CHECK(false, "%s: host arena byte %llu (kind %d) wrong after the downloads", name, (unsigned long long)i,
                  owner[i]);
            break;
        }
    if (n_down) *n_down = down.size();
    return up.size();
}

// the stream's geometry: slots of [lead][data], the data regions filled from their start
struct Geom {
    uint64_t lead, stride;
    uint64_t data(size_t slot) const { return lead + stride * slot; }
};

void check_small() {
    {
        BatchLedger lg;
        std::vector<ByteRange> v{{1, 1}};
        lg.uploads(&v);
        CHECK(v.empty(), "an empty ledger uploads nothing");
        v.push_back({1, 1});
        lg.downloads(&v);
        CHECK(v.empty() && !lg.any_device() && !lg.any_host(), "an empty ledger downloads nothing");
    }
    {  // empty ranges are dropped, wherever they point
        BatchLedger lg;
        CHECK(run("empty ranges", lg, {{kHost, 10, 0}, {kDev, 999, 0}, {kHost, 0, 0}}, 1000) == 0, "no uploads");
        CHECK(!lg.any_device() && !lg.any_host(), "empty ranges leave the ledger empty");
    }
    {  // abutting writes of one kind are one range; of two kinds two, split exactly at the seam
        BatchLedger lg;
        size_t down = 0;
        CHECK(run("abutting", lg, {{kHost, 48, 100}, {kHost, 148, 1}, {kDev, 149, 300}, {kDev, 449, 5}, {kHost, 454, 10}},
                  1000, &down) == 2, "two host runs");
        CHECK(down == 1, "one device run");
        std::vector<ByteRange> up;
        lg.uploads(&up);
        CHECK(up.size() == 2 && up[0].off == 48 && up[0].len == 101 && up[1].off == 454 && up[1].len == 10, "seams");
    }
    {  // host ranges in neighbouring slots with only a lead between them join; a placed range between does not
        BatchLedger lg;
        const Geom g{48, 48 + 2048};
        size_t down = 0;
        CHECK(run("joined across leads", lg,
                  {{kHost, g.data(0), 2048}, {kHost, g.data(1), 2048}, {kDev, g.data(2), 2048}, {kHost, g.data(3), 7},
                   {kHost, g.data(4), 2048}},
                  g.data(5), &down) == 2, "slots 0-1 and 3-4");
        CHECK(down == 1, "slot 2");
    }
    {  // device-only
        BatchLedger lg;
        size_t down = 0;
        CHECK(run("device only", lg, {{kDev, 48, 2048}, {kDev, 48 + 2096, 2048}, {kDev, 48 + 2 * 2096, 1}}, 3 * 2096,
                  &down) == 0, "no upload");
        CHECK(down == 1 && lg.any_device() && !lg.any_host(), "one copy back");
    }
    {  // a slot cleared for the next batch: the same offsets again, the other way round, nothing left over
        BatchLedger lg;
        run("before reuse", lg, {{kHost, 48, 700}, {kDev, 748, 1348}, {kDev, 48 + 2096, 512}}, 2 * 2096);
        lg.clear();
        CHECK(!lg.any_device() && !lg.any_host(), "cleared");
        size_t down = 0;
        CHECK(run("after reuse", lg, {{kDev, 48, 700}, {kHost, 748, 1348}, {kHost, 48 + 2096, 512}}, 2 * 2096, &down) == 1,
              "one host run after the reuse");
        CHECK(down == 1, "one device run after the reuse");
        lg.clear();
        CHECK(run("host only after reuse", lg, {{kHost, 48, 10}}, 2 * 2096, &down) == 1 && down == 0, "host only");
    }
    {  // out of order and overlapping input (not what the stream does): still sorted, merged, in bounds
        BatchLedger lg;
        run("unordered", lg, {{kHost, 500, 100}, {kHost, 100, 50}, {kHost, 120, 100}, {kDev, 300, 10}, {kDev, 250, 20}},
            1000);
    }
}

// batches as the stream fills them: slot after slot, each packet's data region from its start, every piece
// host or device at random; `flavour` 0 host-only, 1 device-only, 2 mixed
void check_batches(size_t slots, int flavour, int rounds) {
    const Geom g{48, 48 + 2048};
    BatchLedger lg;  // one ledger through every round, cleared like a batch that went to the sink
    for (int round = 0; round < rounds; ++round) {
        std::vector<Op> ops;
        const size_t used = 1 + rnd() % slots;
        for (size_t s = 0; s < (round == 0 ? slots : used); ++s) {
            const uint64_t fill = rnd() % 8 == 0 ? rnd() % 2049 : 2048;  // some packets short (flush), some empty (last)
            for (uint64_t at = 0; at < fill;) {
                const uint64_t n = 1 + rnd() % (rnd() % 4 == 0 ? 2048 : 300);
                const uint64_t len = n < fill - at ? n : fill - at;
                const uint8_t kind = flavour == 0 ? kHost : flavour == 1 ? kDev : (rnd() & 1 ? kHost : kDev);
                ops.push_back(Op{kind, g.data(s) + at, len});
                at += len;
            }
        }
        char name[64];
        std::snprintf(name, sizeof name, "batch of %zu, flavour %d, round %d", slots, flavour, round);
        run(name, lg, ops, g.data(slots));
        lg.clear();
    }
}

}  // namespace

int main() {
    check_small();
    for (int flavour = 0; flavour < 3; ++flavour) {
        check_batches(1, flavour, 20);
        check_batches(3, flavour, 50);
        check_batches(64, flavour, 20);
        check_batches(1024, flavour, 3);
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("write ledger ok\n");
    return 0;
}
