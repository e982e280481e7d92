// Internal: the hdfs3_crc_ctx definition and what its owners share. ctx.cpp: the error slot, the table
// images, a ctx's life cycle and settings; ctx_pool.cpp: the process-wide pool and its pinned budget;
// hdfs3_crc.cpp: the C entry points that launch; client/: the readers and streams. Not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "crc32c_kernels.h"

namespace hdfs3crc {

// Sets the thread-local message returned by hdfs3_crc_last_error(); returns `code`.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// The ABI layer's mapping of a HIP error (ctx.cpp, hdfs3_crc.cpp, the lab hooks): -ENOMEM,
// -EINVAL, -ENODEV or -EIO, the message "<what>: <HIP's text>". The readers and streams of client/ keep
// mappings of their own.
int hip_fail(hipError_t e, const char *what);
#define HIP_TRY(expr)                                               \
    do {                                                            \
        hipError_t e_ = (expr);                                     \
        if (e_ != hipSuccess) return hdfs3crc::hip_fail(e_, #expr); \
    } while (0)

// Makes `dev` the calling thread's current device for the guard's lifetime (hipMalloc,
// hipHostMalloc and event creation act on the current device).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// Staging segment of the host-buffer API: 16 MiB of payload per H2D transfer.
constexpr size_t kSegmentBytes = 16u << 20;

// Cached arenas any pooled ctx keeps for its next reader (ctx_release, the block reader's close), and
// what an input stream's read-ahead budget leaves for such contexts
constexpr size_t kArenaCacheKeep = 6;

// A pinned host buffer and its device mirror, owned together. `cap` (bytes of each) is set only once
// both exist: after a failed grow whatever was allocated is freed by the next grow or release.
// The owner picks the host flags (numa.h pinned_host_flags() or hipHostMallocDefault).
template <class T = uint8_t>
struct Mirror {
    T *h = nullptr, *d = nullptr;
    size_t cap = 0;

    hipError_t grow(size_t bytes, unsigned host_flags) {
        if (bytes <= cap) return hipSuccess;
        release();
        if (hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&h), bytes, host_flags); e != hipSuccess) return e;
        if (hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), bytes); e != hipSuccess) return e;
        cap = bytes;
        return hipSuccess;
    }
    void release() {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        h = d = nullptr;
        cap = 0;
    }
    size_t bytes() const { return cap; }
};

struct Slot {
    Mirror<> data, crc;
    hipEvent_t done = nullptr;
    // compute: CRC bytes waiting in crc.h to be copied out once `done` fires
    uint8_t *pending_out = nullptr;
    size_t pending_bytes = 0;

    void release() {  // the buffers only: the event stays for the slot's next use
        data.release();
        crc.release();
    }
    uint64_t pinned_bytes() const { return data.bytes() + crc.bytes(); }
    uint64_t device_bytes() const { return pinned_bytes(); }
};

// One packet batch's buffers for the block reader: pinned wire arena + its HBM mirror,
// packet descriptors, the verify result word and the completion event. Cached in the ctx
// so the block readers an input stream opens one after another reuse them.
struct PacketArena {
    Mirror<> buf;
    Mirror<DevSegment> desc;         // descriptor staging
    Mirror<unsigned long long> res;  // the verify result word
    hipEvent_t done = nullptr;
    // 4096-byte piece CRCs of a batch at bpc = R x 4096 (launch_chunks' pieces + combine): the
    // batch's own, so two readers verifying on one ctx (a stream's sequential reader and a pread's)
    // never share it (round 5; the ctx's scratch is for the calls of the ctx's own thread)
    PieceScratch pieces;

    void release() {
        pieces.release();
        buf.release();
        desc.release();
        res.release();
        if (done) (void)hipEventDestroy(done);
        *this = PacketArena();
    }
    uint64_t pinned_bytes() const { return buf.bytes() + desc.bytes() + res.bytes(); }
    // the arena's own piece scratch (bpc = R x 4096 batches) stays allocated while it is cached
    uint64_t device_bytes() const { return pinned_bytes() + pieces.cap[0] + pieces.cap[1]; }
};

}  // namespace hdfs3crc

struct hdfs3_crc_ctx;
namespace hdfs3crc {
// Process-wide pool of contexts for the client drop-ins (input/output streams, block and
// local readers). libhdfs3 opens a stream per file and a reader per block; creating a ctx
// (stream, table uploads, device query) and its pinned arenas costs milliseconds, more than
// reading a small file. A released ctx keeps its arena cache and goes back to the pool.
// acquire: a pooled ctx of `device` (stream reset to its own, type CRC32C) or a new one.
// deep = true: prefer the pooled ctx holding the most cached arenas (block read-ahead rings).
int ctx_acquire(int device, hdfs3_crc_ctx **out, bool deep = false);
// release: synchronizes the ctx's stream; pooled when that succeeds and the pool has room.
void ctx_release(hdfs3_crc_ctx *ctx);
// the pinned bytes the pool may retain (HDFS3_POOL_PINNED_MAX, default 1 GiB)
uint64_t pool_pinned_cap_bytes();
// pinned / device bytes a ctx holds beyond its tables (staging, cached arenas), and the pinned
// bytes the ctx pool retains now
void ctx_footprint(hdfs3_crc_ctx *ctx, uint64_t *pinned, uint64_t *device);
uint64_t ctx_pool_pinned_bytes();
// Serialises every ADMISSION into either pool (ctx_release, the local readers' give_back): the only
// operations that add retained pinned bytes. Each admission reads the other pool's bytes and decides
// under this lock, so two releases at once cannot both fit the same headroom. Taking a
// ctx or an entry out of a pool, shedding and trimming only lower the total and do not take it.
// Order: this lock first, then a pool's own mutex (never the reverse).
std::mutex &pool_admission_mu();
// The short-circuit readers' own pool (local_reader.cpp: a ctx and its windows per entry) counts
// against the same cap: its retained bytes, pooled entries, and a trim that frees them all
struct LocalPoolStats {
    uint64_t pinned = 0, device = 0, entries = 0;
};
LocalPoolStats local_pool_stats();
int local_pool_trim();
}  // namespace hdfs3crc

struct hdfs3_crc_ctx {
    int device = 0;
    int grid_cap = 256;            // one 1024-thread workgroup per CU (128 KiB LDS image)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    uint32_t *d_tables = nullptr;  // active 4 x 256 slice-table image (checksum_type)
    uint32_t *d_fold = nullptr;    // active lane-fold GF(2) matrices (crc32c_tables.h)
    // per polynomial: [0] CRC32C (CHECKSUM_CRC32C = 2), [1] CRC-32/zlib (CHECKSUM_CRC32 = 1)
    uint32_t *d_tables_by[2] = {nullptr, nullptr};
    uint32_t *d_fold_by[2] = {nullptr, nullptr};
    int checksum_type = 2;
    uint32_t poly = 0x82F63B78u;        // reflected polynomial of checksum_type
    hdfs3crc::Mirror<unsigned long long> result;  // the blocking calls' verdict word
    // blocks API: a ring of descriptor stagings, each reusable once its event fired
    struct SegStage {
        hdfs3crc::Mirror<hdfs3crc::DevSegment> seg;
        hipEvent_t done = nullptr;
        bool armed = false;  // done recorded after a copy out of seg.h that may still be pending
        hipEvent_t copied = nullptr;  // the descriptors' copy on desc_stream (DescCopy)
        uint64_t pinned_bytes() const { return seg.bytes(); }
        uint64_t device_bytes() const { return seg.bytes(); }
    } seg_ring[4];
    // long descriptor lists copy on this stream, beside the previous launch (DescCopy; created on first use)
    hipStream_t desc_stream = nullptr;
    unsigned seg_next = 0;
    hdfs3crc::WordScratch words;  // dense CRC words of compute over in-packet word regions
    hdfs3crc::PieceScratch pieces;  // 4096-byte piece CRCs of chunks above 4 KiB (launch_chunks)
    hdfs3crc::ComposeScratch compose;  // the composite calls' chunk words and partials (crc32c_compose.hip)
    hdfs3crc::Slot slot[2];
    std::atomic<uint64_t> launches{0};
    std::mutex arena_mu;                          // guards arena_cache
    std::vector<hdfs3crc::PacketArena> arena_cache;
};

namespace hdfs3crc {
// Makes `type` (HDFS3_CHECKSUM_TYPE_CRC32C or _CRC32, checked by the caller) the ctx's polynomial: its
// table and fold images and `poly`
void select_checksum_type(hdfs3_crc_ctx *ctx, int type);
// device bytes of a ctx's table and fold images, both polynomials
uint64_t table_image_bytes();
// true when p is device memory of the ctx's device. Anything else (a host pointer is the caller's mistake,
// not a fault of the GPU) clears HIP's sticky error and gives false; the caller words its own error.
bool is_device_memory_of(hdfs3_crc_ctx *ctx, const void *p);
// A ctx's launch environment. own_pieces: a batch arena's piece scratch (block reader, output stream), whose
// launches may come from another thread and so leave the ctx's own word and piece scratch alone
inline LaunchEnv launch_env(hdfs3_crc_ctx *ctx, PieceScratch *own_pieces = nullptr) {
    return LaunchEnv{ctx->d_tables, ctx->d_fold, ctx->grid_cap, ctx->stream, own_pieces ? nullptr : &ctx->words,
                     own_pieces ? own_pieces : &ctx->pieces, nullptr};
}
// hdfs3_gather_dev_async without its argument checks: every range checked first (-EINVAL before any launch),
// then one gather launch per kGatherMaxRanges planned ranges on the ctx stream. Touches the ctx's stream and
// launch counter only, so the block reader's caller thread may run it beside the receiver's launches (the
// calling thread's current device is the ctx's). *launched (if given) is raised by the launches made.
int gather_dev(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const void *d_src, size_t src_len, const CopyRange *r,
               size_t n, unsigned *launched = nullptr);
// hdfs3_gather_sources_dev_async without its null checks: gather_dev with a source address per range (r[i].src_off;
// launch_plan.h: gather_sources_first_bad), the same checks first, the same launches, stream and counter.
int gather_sources_dev(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const CopyRange *r, size_t n,
                       unsigned *launched = nullptr);
// hdfs3_deliver_verified_dev_async without its null checks of ctx and buffers: the guard and every range checked
// first (-EINVAL before any launch), then gather_dev's launches as guarded deliveries, each reading the same
// guard words and writing the same chain word; with nothing to copy one launch still passes the gate on.
// Like gather_dev it touches the ctx's stream and launch counter only.
int deliver_dev(hdfs3_crc_ctx *ctx, void *d_dst, size_t dst_len, const void *d_src, size_t src_len, const CopyRange *r,
                size_t n, const DeliverGuard &guard, unsigned *launched = nullptr);
}  // namespace hdfs3crc

