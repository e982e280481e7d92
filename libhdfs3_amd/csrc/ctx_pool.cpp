// The process-wide pool of contexts (ctx.h: ctx_acquire / ctx_release) and its pinned-memory budget
// (HDFS3_POOL_PINNED_MAX; hdfs3_crc_pool_stats_get, hdfs3_crc_pool_trim).
#include "hdfs3_crc.h"

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "ctx.h"

namespace hdfs3crc {
namespace {
std::mutex g_ctx_pool_mu;
std::vector<hdfs3_crc_ctx *> g_ctx_pool;
constexpr size_t kCtxPoolMax = 32;
constexpr size_t kDeepCtxMax = 8;      // pooled contexts allowed to keep a read-ahead ring's worth
// 1 GiB: the rings of a read-ahead stream up to depth 3 (whole 128 MiB blocks) plus the usual
// shallow contexts; with 512 MiB, depth 2 / 3 read 9.1-10.7 / 5.1-7.0 GiB/s against 13.2-13.9 /
// 11.1-14.1 (every open re-pinned rings the pool had shed; profiles/r03/reentry/r3e2e_caps_*)
constexpr uint64_t kPoolPinnedDefault = uint64_t(1) << 30;

// HDFS3_POOL_PINNED_MAX: bytes, or with a K/M/G suffix
uint64_t pool_pinned_cap() {
    static const uint64_t cap = [] {
        const char *e = std::getenv("HDFS3_POOL_PINNED_MAX");
        if (!e || !*e) return kPoolPinnedDefault;
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        const int shift = *end == 'K' || *end == 'k' ? 10 : *end == 'M' || *end == 'm' ? 20
                          : *end == 'G' || *end == 'g' ? 30 : 0;
        // a whole number with at most one K/M/G suffix; anything else ("1.5G", "64MiB", "-1")
        // is not silently read as a prefix of itself: the default stays and a warning says so
        const char *rest = end + (shift ? 1 : 0);
        if (end == e || *e == '-' || *rest != '\0' || (shift && v > (~0ull >> shift))) {
            std::fprintf(stderr, "libhdfs3_crc: HDFS3_POOL_PINNED_MAX=\"%s\" is not a byte count "
                                 "(digits with an optional K/M/G suffix); using the default %llu bytes\n",
                         e, (unsigned long long)kPoolPinnedDefault);
            return kPoolPinnedDefault;
        }
        return uint64_t(v) << shift;
    }();
    return cap;
}

struct Footprint {
    uint64_t pinned = 0, device = 0;
};

// what a ctx holds beyond its tables: pinned host and device bytes of its staging slots, cached
// arenas (with their piece scratch), descriptor stagings, word and piece scratch and result word
Footprint footprint(hdfs3_crc_ctx *ctx) {
    Footprint f;
    auto add = [&f](const auto &owner) {
        f.pinned += owner.pinned_bytes();
        f.device += owner.device_bytes();
    };
    for (const Slot &s : ctx->slot) add(s);
    {
        std::lock_guard<std::mutex> lk(ctx->arena_mu);
        for (const PacketArena &a : ctx->arena_cache) add(a);
    }
    for (const auto &st : ctx->seg_ring) add(st);
    f.pinned += ctx->result.bytes();
    f.device += ctx->words.cap + ctx->pieces.cap[0] + ctx->pieces.cap[1] + ctx->result.bytes();
    f.device += ctx->compose.words_cap + ctx->compose.partials_cap;
    f.device += table_image_bytes();
    return f;
}

// give back what a pooled ctx can rebuild on demand: cached arenas beyond `keep`, then the
// staging slots of the host API
void shed(hdfs3_crc_ctx *ctx, size_t keep_arenas, bool slots) {
    DeviceGuard g(ctx->device);
    {
        std::lock_guard<std::mutex> alk(ctx->arena_mu);
        while (ctx->arena_cache.size() > keep_arenas) {
            ctx->arena_cache.back().release();
            ctx->arena_cache.pop_back();
        }
    }
    if (!slots) return;
    for (Slot &s : ctx->slot) s.release();
}
}  // namespace

uint64_t pool_pinned_cap_bytes() { return pool_pinned_cap(); }

std::mutex &pool_admission_mu() {
    static std::mutex mu;
    return mu;
}

void ctx_footprint(hdfs3_crc_ctx *ctx, uint64_t *pinned, uint64_t *device) {
    const Footprint f = footprint(ctx);
    if (pinned) *pinned = f.pinned;
    if (device) *device = f.device;
}

uint64_t ctx_pool_pinned_bytes() {
    std::lock_guard<std::mutex> lk(g_ctx_pool_mu);
    uint64_t n = 0;
    for (hdfs3_crc_ctx *c : g_ctx_pool) n += footprint(c).pinned;
    return n;
}

int ctx_acquire(int device, hdfs3_crc_ctx **out, bool deep) {
    if (!out) return fail(-EINVAL, "null out");
    {
        std::lock_guard<std::mutex> lk(g_ctx_pool_mu);
        // deep: the pooled ctx with the most cached arenas (a read-ahead reader's ring);
        // otherwise the one with the fewest, which keeps the deep ones for read-ahead
        long best = -1;
        for (size_t i = 0; i < g_ctx_pool.size(); ++i) {
            if (g_ctx_pool[i]->device != device) continue;
            if (best < 0 || (deep ? g_ctx_pool[i]->arena_cache.size() > g_ctx_pool[size_t(best)]->arena_cache.size()
                                  : g_ctx_pool[i]->arena_cache.size() < g_ctx_pool[size_t(best)]->arena_cache.size()))
                best = long(i);
        }
        if (best >= 0) {
            hdfs3_crc_ctx *ctx = g_ctx_pool[size_t(best)];
            g_ctx_pool.erase(g_ctx_pool.begin() + best);
            ctx->stream = ctx->own_stream;
            select_checksum_type(ctx, HDFS3_CHECKSUM_TYPE_CRC32C);
            *out = ctx;
            return 0;
        }
    }
    return hdfs3_crc_ctx_create(device, out);
}

void ctx_release(hdfs3_crc_ctx *ctx) {
    if (!ctx) return;
    bool ok;
    {
        DeviceGuard g(ctx->device);
        ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    for (Slot &s : ctx->slot) s.pending_out = nullptr;
    if (ok) {
        // one admission at a time across both pools (pool_admission_mu): the short-circuit readers'
        // pool counts against the same cap, and its bytes cannot grow while this decision is made
        std::lock_guard<std::mutex> adm(pool_admission_mu());
        const uint64_t local = local_pool_stats().pinned;
        std::lock_guard<std::mutex> lk(g_ctx_pool_mu);
        if (g_ctx_pool.size() < kCtxPoolMax) {
            // a read-ahead reader's deep ring leaves up to a block's worth of pinned arenas in
            // its ctx (block_reader.cpp); at most kDeepCtxMax pooled contexts keep that much,
            // the others go back to the usual few arenas
            size_t deep = 0;
            for (hdfs3_crc_ctx *c : g_ctx_pool) deep += c->arena_cache.size() > kArenaCacheKeep;
            if (deep >= kDeepCtxMax && ctx->arena_cache.size() > kArenaCacheKeep) shed(ctx, kArenaCacheKeep, false);
            // and the pool as a whole retains at most pool_pinned_cap() pinned bytes. The ctx released
            // last is the one most likely to be taken again soon (a read-ahead stream releases the
            // ring of the block it finished and at once acquires a deep ctx for the next block ahead),
            // so the pooled contexts give back their arenas first, least recently released first
            // (the pool's front); then this ctx sheds arenas and staging, and is destroyed if it still
            // does not fit. Shedding this ctx first made every read-ahead block re-pin its ring once
            // older pooled rings filled the cap: 1 GiB with read-ahead 2 / 7 at 6.6 / 2.3 GiB/s
            // against 11.8 / 10.6 uncapped (profiles/r03/reentry/r3e2eab_*).
            const uint64_t cap = pool_pinned_cap() > local ? pool_pinned_cap() - local : 0;
            const uint64_t mine = footprint(ctx).pinned;
            uint64_t others = 0;
            for (hdfs3_crc_ctx *c : g_ctx_pool) others += footprint(c).pinned;
            for (const bool slots : {false, true})  // their arenas first, then their staging slots
                for (size_t i = 0; i < g_ctx_pool.size() && others + mine > cap; ++i) {
                    const uint64_t before = footprint(g_ctx_pool[i]).pinned;
                    shed(g_ctx_pool[i], 0, slots);
                    others -= before - footprint(g_ctx_pool[i]).pinned;
                }
            if (others + footprint(ctx).pinned > cap) shed(ctx, 0, false);
            if (others + footprint(ctx).pinned > cap) shed(ctx, 0, true);
            if (others + footprint(ctx).pinned <= cap) {
                g_ctx_pool.push_back(ctx);
                return;
            }
        }
    }
    hdfs3_crc_ctx_destroy(ctx);
}

}  // namespace hdfs3crc

using hdfs3crc::fail;

extern "C" {

int hdfs3_crc_ctx_acquire(int device, hdfs3_crc_ctx **out) { return hdfs3crc::ctx_acquire(device, out); }
void hdfs3_crc_ctx_release(hdfs3_crc_ctx *ctx) { hdfs3crc::ctx_release(ctx); }

int hdfs3_crc_pool_stats_get(hdfs3_crc_pool_stats *out) {
    if (!out) return fail(-EINVAL, "null out");
    hdfs3_crc_pool_stats st{};
    // The short-circuit readers' pooled contexts and windows are part of the same budget. The two pools
    // are read one after the other: without the admission lock an entry taken out of the first and a ctx
    // admitted into the second in between were both counted, a sum above the cap that never existed. With
    // it only removals can fall between the two reads, so the sum is at most what was retained.
    std::lock_guard<std::mutex> adm(hdfs3crc::pool_admission_mu());
    const hdfs3crc::LocalPoolStats lp = hdfs3crc::local_pool_stats();
    std::lock_guard<std::mutex> lk(hdfs3crc::g_ctx_pool_mu);
    for (hdfs3_crc_ctx *c : hdfs3crc::g_ctx_pool) {
        const hdfs3crc::Footprint f = hdfs3crc::footprint(c);
        st.pinned_bytes += f.pinned;
        st.device_bytes += f.device;
    }
    st.pinned_bytes += lp.pinned;
    st.device_bytes += lp.device;
    st.pooled_contexts = hdfs3crc::g_ctx_pool.size() + lp.entries;
    st.pinned_cap_bytes = hdfs3crc::pool_pinned_cap();
    *out = st;
    return 0;
}

int hdfs3_crc_pool_trim(void) {
    const int local = hdfs3crc::local_pool_trim();
    std::vector<hdfs3_crc_ctx *> idle;
    {
        std::lock_guard<std::mutex> lk(hdfs3crc::g_ctx_pool_mu);
        idle.swap(hdfs3crc::g_ctx_pool);
    }
    for (hdfs3_crc_ctx *c : idle) hdfs3_crc_ctx_destroy(c);
    return int(idle.size()) + local;
}

}  // extern "C"
