// hdfs3_local_reader: LocalBlockReader (src/client/LocalBlockReader.cpp) — the short-
// circuit read of a block file and its .meta file — with readAndVerify's per-chunk CPU
// loop (:138-163) replaced by GPU verification of large windows.
//
// .meta layout (:40-43, :64-121): BE16 version (1) | u8 checksum type | BE32 bytesPerChecksum
// | one BE32 CRC per chunk. Local semantics check every chunk, the short tail included.
//
// Pipeline: a loader thread preads a window (window_buffers x buffer_size bytes of block
// data, chunk aligned) and its CRC words into a pinned arena, then queues H2D + verify
// (check_short_tail=1) + result D2H + event on the ctx stream; the caller's read() waits
// for a window's event and copies verified bytes out, while the loader fills the next.
// Delivery granularity on a mismatch is the reference's: readAndVerify verifies one
// buffer_size buffer before any of it is returned, so bytes of the buffer holding the
// first bad chunk — and everything after — are withheld and -EIO is returned.
// read_dev() delivers into device memory instead: the window's device copy goes to the caller's
// buffer in a guarded delivery (crc32c_gather.hip) that reads the window's result word on the
// device, so the caller enqueues it without waiting for the verify (see read_dev_verified).
//
// Geometry. Every size and offset here comes from local_layout.h (host arithmetic, checked on the CPU by
// tests/test_local_layout.py): the buffer, the first byte, the windows, their chunks and .meta words, where a
// corrupt block's good bytes end (good_end) and the span of a window a read takes. This file holds the files,
// the mapping, the pool and the threads. The three reads (read, read_dev_plain, read_dev_verified) take their
// next window through next_ready() and end through finish().
//
// Staging. Verification on: a window is pread into its pinned arena by the loader and the
// helper threads together (a single pread thread was the single-stream limit), DMA'd, and
// copied out. Verification off: the block file is mmap'd (MappedFileWrapper, MappedFileWrapper.cpp:
// 58-70, is the reference's own mmap reader) and read() copies straight out of the page cache,
// one copy per byte. HDFS3_LOCAL_MMAP=1 also maps verified reads: each window's page-cache pages
// are registered with HIP (pinned in place) and DMA'd directly, then copied out of the mapping;
// registration pins at ~23 GiB/s and serialises across threads in the runtime, so it is an
// opt-in (docs/DESIGN_HISTORY.md §5.1). HDFS3_LOCAL_MMAP=0 disables mapping altogether. Any mmap or
// registration failure falls back to the pread path for that window or reader.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <climits>
#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../copy_pool.h"
#include "../ctx.h"
#include "../numa.h"
#include "hdfs3_client.h"
#include "hdfs3_crc.h"
#include "local_layout.h"
#include "local_reader.h"
#include "wire.h"

using namespace hdfs3crc;

namespace {

constexpr int kSlots = 3;

// Window events: HDFS3_LOCAL_BLOCKING_SYNC=1 makes the consumer sleep in hipEventSynchronize
// (hipEventBlockingSync) instead of spinning, leaving the cores to the copies when many readers
// run at once (round 4 measurement knob; the default keeps the spin)
unsigned window_event_flags() {
    static const unsigned f = [] {
        const char *e = getenv("HDFS3_LOCAL_BLOCKING_SYNC");
        return unsigned(hipEventDisableTiming) | (e && e[0] == '1' ? unsigned(hipEventBlockingSync) : 0u);
    }();
    return f;
}

int hip_err(hipError_t e, const char *what) {
    return fail(e == hipErrorOutOfMemory ? -ENOMEM : -EIO, "%s: %s", what, hipGetErrorString(e));
}

#define HIP_OK(expr)                                      \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return hip_err(e_, #expr);  \
    } while (0)

// read_dev's own words, made on a reader's first device read and pooled with the rest: the two gate words
// of the delivery chain (device), the pinned word the last one is read back into, and the event behind it
struct DeviceWords {
    uint64_t *d_gate = nullptr;
    unsigned long long *h_gate = nullptr;
    hipEvent_t done = nullptr;

    void release() {
        if (d_gate) (void)hipFree(d_gate);
        if (h_gate) (void)hipHostFree(h_gate);
        if (done) (void)hipEventDestroy(done);
        *this = DeviceWords();
    }
};

// Reader resources — a ctx (stream, table images) and kSlots pinned + device windows —
// are pooled per process. The reference opens one LocalBlockReader per block
// (InputStreamImpl::setupBlockReader), and creating a ctx and pinning the windows costs
// more than reading a 128 MiB block from the page cache (docs/DESIGN_HISTORY.md §5.1).
struct LocalResources {
    hdfs3_crc_ctx *ctx = nullptr;
    PacketArena a[kSlots];
    DeviceWords dev;
};
std::mutex g_pool_mu;
std::vector<LocalResources> g_pool;
constexpr size_t kPoolMax = 16;

bool take_pooled(int device, size_t cap, LocalResources *out) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); ++i) {
        if (g_pool[i].ctx->device == device && g_pool[i].a[0].buf.cap >= cap) {
            *out = g_pool[i];
            g_pool.erase(g_pool.begin() + long(i));
            return true;
        }
    }
    return false;
}

// Drops an entry's windows and words. Its ctx is released into the ctx pool, or destroyed outright: an entry
// dropped to keep the pinned cap, or by a trim, must not move the bytes just refused into the other pool.
void drop_resources(LocalResources &r, bool destroy_ctx) {
    for (PacketArena &a : r.a) a.release();
    r.dev.release();
    if (destroy_ctx) hdfs3_crc_ctx_destroy(r.ctx);
    else ctx_release(r.ctx);
    r.ctx = nullptr;
}

// pinned / device bytes of a pooled entry: its windows and what its ctx holds
LocalPoolStats entry_bytes(const LocalResources &r) {
    LocalPoolStats st;
    ctx_footprint(r.ctx, &st.pinned, &st.device);
    for (const PacketArena &a : r.a) {
        st.pinned += a.pinned_bytes();
        st.device += a.device_bytes();
    }
    if (r.dev.d_gate) st.device += 2 * sizeof(uint64_t);
    if (r.dev.h_gate) st.pinned += sizeof(unsigned long long);
    st.entries = 1;
    return st;
}

// Pooled unless that would take the retained pinned bytes of both pools past the cap
// (HDFS3_POOL_PINNED_MAX): the oldest pooled entries are evicted first, then this one is not
// admitted. The decision is made under pool_admission_mu (ctx.h), so a ctx_release or another
// give_back on another thread cannot admit bytes into the same headroom meanwhile.
void give_back(LocalResources r) {
    std::vector<LocalResources> evict;
    bool keep = false;
    {
        std::lock_guard<std::mutex> adm(pool_admission_mu());
        const uint64_t cap = pool_pinned_cap_bytes(), ctxs = ctx_pool_pinned_bytes(), mine = entry_bytes(r).pinned;
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (g_pool.size() < kPoolMax) {
            uint64_t local = 0;
            for (const LocalResources &e : g_pool) local += entry_bytes(e).pinned;
            while (!g_pool.empty() && ctxs + local + mine > cap) {
                local -= entry_bytes(g_pool.front()).pinned;
                evict.push_back(g_pool.front());
                g_pool.erase(g_pool.begin());
            }
            if (ctxs + local + mine <= cap) {
                g_pool.push_back(r);
                keep = true;
            }
        }
    }
    for (LocalResources &e : evict) drop_resources(e, /*destroy_ctx=*/true);
    // not admitted: the windows go, and the ctx takes its own admission into the ctx pool
    // (ctx_release takes pool_admission_mu itself, so this runs after the scope above)
    if (!keep) drop_resources(r, /*destroy_ctx=*/false);
}

// Copies out of a verified window (one thread ~11 GiB/s) and the window preads (one thread
// ~9-12 GiB/s) are this reader's single-stream limits: both go through the process-wide
// CopyPool (copy_pool.h).

struct Window {
    PacketArena a;            // h/d: [data (cap_data)][crc words]
    LocalWindow g;            // its bytes of the block, its chunks and their .meta words
    int64_t bad_chunk = -1;   // first mismatching chunk (block-relative), after wait
    bool verified = false;
    const uint8_t *src = nullptr;  // where read() copies from: a.buf.h, or the mapping
    void *reg = nullptr;           // mapped mode: the window's registered page range
};

constexpr int64_t kPage = 4096;

}  // namespace

namespace hdfs3crc {
LocalPoolStats local_pool_stats() {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    LocalPoolStats st;
    for (const LocalResources &e : g_pool) {
        const LocalPoolStats b = entry_bytes(e);
        st.pinned += b.pinned;
        st.device += b.device;
        st.entries += 1;
    }
    return st;
}

int local_pool_trim() {
    std::vector<LocalResources> idle;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        idle.swap(g_pool);
    }
    // destroyed outright, not released: a trim leaves no context behind in either pool
    for (LocalResources &e : idle) drop_resources(e, /*destroy_ctx=*/true);
    return int(idle.size());
}
}  // namespace hdfs3crc

struct hdfs3_local_reader {
    int data_fd = -1, meta_fd = -1;
    hdfs3_crc_ctx *ctx = nullptr;
    bool verify = true;
    int checksum_type = 2;
    uint32_t flags = 0;                      // hdfs3_local_opts.flags
    uint32_t chunk_size = 0;
    LocalLayout lay;                         // buffer, first byte, end, windows (local_layout.h)
    int64_t cursor = 0;                      // next byte handed to the caller

    std::mutex mu;
    std::condition_variable cv;
    Window slot[kSlots];
    std::deque<int> ready, free_slots;
    bool load_done = false, stop = false;
    int load_error = 0;
    std::string load_msg;
    std::thread loader;
    int error = 0;
    std::string error_msg;
    // the failure is the replica's (its files or their contents); every other failure is this host's
    // (local_reader_host_fault). Set by the loader before it publishes load_error, by the caller otherwise.
    std::atomic<bool> replica_fault{false};
    std::atomic<uint64_t> batches{0};
    // mapped mode
    uint8_t *map = nullptr;
    size_t map_len = 0;                      // length rounded up to a page
    bool map_verified = false;               // HDFS3_LOCAL_MMAP=1: verified windows DMA'd from the mapping
    std::atomic<uint64_t> mapped_windows{0};
    // read_dev
    DeviceWords dev;
    bool gate_zeroed = false;                // this reader's chain starts from two zero words
    int gate_cur = 0;                        // the gate word the last delivery of the chain wrote
    std::atomic<uint64_t> dev_launches{0}, dev_bytes{0};

    int sticky(int code, const std::string &msg) {
        error = code;
        error_msg = msg;
        return fail(code, "%s", msg.c_str());
    }

    // LocalBlockReader ctor (:46-130): meta header, engine selection, buffer size
    int open_meta(bool want_verify) {
        uint8_t h[kLocalMetaHeader];
        if (int rc = pread_fully(meta_fd, h, sizeof(h), 0)) return sticky(rc, "LocalBlockReader: cannot read the meta header");
        const int version = (h[0] << 8) | h[1];
        if (version != 1)
            return sticky(-EIO, "LocalBlockReader get an unmatched block, expected block version 1, real version is " +
                                    std::to_string(version));
        checksum_type = h[2];
        verify = want_verify;
        switch (checksum_type) {
        case wire::kChecksumNull: verify = false; break;
        case wire::kChecksumCrc32c:
        case wire::kChecksumCrc32:
            // Both types select the CRC32C engine (:85-98), as in the reference: a block
            // whose meta declares CHECKSUM_CRC32 is verified with CRC32C and so fails with
            // ChecksumException there and here. HDFS3_LOCAL_CRC32_AS_ZLIB opts into the
            // polynomial the meta declares instead (see engine_type()).
            chunk_size = (uint32_t(h[3]) << 24) | (uint32_t(h[4]) << 16) | (uint32_t(h[5]) << 8) | h[6];
            break;
        default:
            return sticky(-EIO, "LocalBlockReader cannot recognize checksum type: " + std::to_string(checksum_type));
        }
        // LocalBlockReader.cpp:100-115 reads bytesPerChecksum as a signed int and rejects only
        // chunkSize <= 0; a chunk above 1 GiB then fails the local buffer bound at open
        if (verify && (chunk_size == 0 || chunk_size > uint32_t(INT32_MAX)))
            return sticky(-EIO, "LocalBlockReader get an invalid checksum parameter, bytes per check: " +
                                    std::to_string(chunk_size));
        return 0;
    }

    // the polynomial the GPU checks this block with
    int engine_type() const {
        return checksum_type == wire::kChecksumCrc32 && (flags & HDFS3_LOCAL_CRC32_AS_ZLIB) ? HDFS3_CHECKSUM_TYPE_CRC32
                                                                                          : HDFS3_CHECKSUM_TYPE_CRC32C;
    }

    // ---- loader thread ------------------------------------------------------------------
    int load(Window &w, int64_t start) {
        w.g = lay.window_at(start);
        const uint32_t len = w.g.len;
        const size_t cap_data = lay.cap_data;
        w.bad_chunk = -1;
        w.verified = false;
        w.src = w.a.buf.h;
        w.reg = nullptr;
        const uint8_t *h2d_src = w.a.buf.h;
        if (map && !verify) {
            w.src = map + start;  // no staging at all: read() copies from the page cache
        } else if (map && map_verified && start % kPage == 0) {
            // pin the window's page-cache pages in place; the DMA reads them directly
            const size_t reg_len = size_t(std::min<int64_t>((start + len + kPage - 1) / kPage * kPage,
                                                            int64_t(map_len)) - start);
            if (hipHostRegister(map + start, reg_len, hipHostRegisterReadOnly) == hipSuccess) {
                w.reg = map + start;
                w.src = h2d_src = map + start;
                mapped_windows.fetch_add(1, std::memory_order_relaxed);
            } else {
                (void)hipGetLastError();  // pread path for this window
            }
        }
        if (w.src == w.a.buf.h) {
            if (int rc = CopyPool::get().pread(data_fd, w.a.buf.h, len, start)) {
                load_msg = "LocalBlockReader: failed to read the block file";
                replica_fault = true;
                return rc;
            }
        }
        batches.fetch_add(1, std::memory_order_relaxed);
        if (!verify) {
            w.verified = true;
            return 0;
        }
        if (int rc = pread_fully(meta_fd, w.a.buf.h + cap_data, w.g.meta_bytes, w.g.meta_off)) {
            load_msg = "LocalBlockReader: failed to read the meta file";
            replica_fault = true;
            return rc;
        }
        HIP_OK(hipMemcpyAsync(w.a.buf.d, h2d_src, len, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(hipMemcpyAsync(w.a.buf.d + cap_data, w.a.buf.h + cap_data, w.g.meta_bytes, hipMemcpyHostToDevice,
                              ctx->stream));
        HIP_OK(hipMemsetAsync(w.a.res.d, 0, sizeof(unsigned long long), ctx->stream));
        if (int rc = hdfs3_crc32c_verify_dev_async(ctx, w.a.buf.d, len, chunk_size, w.a.buf.d + cap_data,
                                                   /*check_short_tail=*/1, reinterpret_cast<uint64_t *>(w.a.res.d))) {
            load_msg = hdfs3_crc_last_error();
            return rc;
        }
        HIP_OK(hipMemcpyAsync(w.a.res.h, w.a.res.d, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipEventRecord(w.a.done, ctx->stream));
        return 0;
    }

    void run_loader() {
        (void)hipSetDevice(ctx->device);
        bind_thread_to_device(ctx->device);  // preads land next to the GPU (numa.h)
        int64_t next = lay.first;
        while (next < lay.length) {
            int s;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !free_slots.empty(); });
                if (stop) return;
                s = free_slots.front();
                free_slots.pop_front();
            }
            const int rc = load(slot[s], next);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (rc) {
                    load_error = rc;
                    if (load_msg.empty()) load_msg = hdfs3_crc_last_error();
                    free_slots.push_back(s);
                } else {
                    ready.push_back(s);
                }
                if (rc || slot[s].g.end() >= lay.length) load_done = true;
            }
            cv.notify_all();
            if (rc) return;
            next = slot[s].g.end();
        }
        std::lock_guard<std::mutex> lk(mu);
        load_done = true;
        cv.notify_all();
    }

    void release_pages(Window &w) {
        if (w.reg) {
            (void)hipHostUnregister(w.reg);
            w.reg = nullptr;
        }
    }

    // ---- caller side ----------------------------------------------------------------------
    int wait(Window &w) {
        if (w.verified) return 0;
        HIP_OK(hipEventSynchronize(w.a.done));
        const unsigned long long r = *w.a.res.h;
        if (r) w.bad_chunk = int64_t(w.g.chunk0) + hdfs3_crc_decode_result(r);
        w.verified = true;
        return 0;
    }

    // The loader's failure as a read met it, captured under mu
    struct LoadError {
        int code = 0;
        std::string msg;
    };

    // The slot `depth` windows into `ready`; at depth 0 waits until there is one or the loader is done. -1 when
    // there is none: then, at depth 0, *le holds the loader's error, if it had one.
    int next_ready(size_t depth, LoadError *le) {
        std::unique_lock<std::mutex> lk(mu);
        if (depth == 0) cv.wait(lk, [&] { return !ready.empty() || load_done; });
        if (ready.size() > depth) return ready[depth];
        if (depth == 0) *le = LoadError{load_error, load_msg};
        return -1;
    }

    int front_slot() {  // -1: `ready` is empty
        std::lock_guard<std::mutex> lk(mu);
        return ready.empty() ? -1 : ready.front();
    }

    // The front window was read to its end (its DMA completed: its `done` event has passed)
    void give_slot_back(Window &w, int s) {
        release_pages(w);
        {
            std::lock_guard<std::mutex> lk(mu);
            ready.pop_front();
            free_slots.push_back(s);
        }
        cv.notify_all();
    }

    // How every read ends, `total` bytes delivered and the cursor behind them. A bad chunk whose good bytes
    // (up to `end`) are all delivered: sticky -EIO, the bytes now and the error next time. Else a loader's error:
    // now if nothing was delivered, sticky for the next call if something was.
    int32_t finish(int32_t total, int64_t bad_chunk, int64_t end, const LoadError &le) {
        if (bad_chunk >= 0 && cursor >= end) {
            replica_fault = true;
            sticky(-EIO, "ChecksumException: LocalBlockReader checksum not match for block (chunk " +
                             std::to_string(bad_chunk) + ")");
            return total ? total : error;
        }
        if (le.code && !total) return sticky(le.code, le.msg);
        if (le.code) {
            error = le.code;
            error_msg = le.msg;
        }
        return total;
    }

    int32_t read(uint8_t *out, int32_t len) {
        if (error) return fail(error, "%s", error_msg.c_str());
        if (!out || len <= 0) return fail(-EINVAL, "invalid read buffer");
        int32_t total = 0;
        int64_t bad_chunk = -1, end = INT64_MAX;  // the front window's first bad chunk and its good end, once known
        LoadError le;
        while (total < len && cursor < lay.length) {
            const int s = next_ready(0, &le);
            if (s < 0) break;
            Window &w = slot[s];
            if (int rc = wait(w)) return total ? total : sticky(rc, hdfs3_crc_last_error());
            if (w.bad_chunk >= 0) {
                bad_chunk = w.bad_chunk;
                end = lay.good_end(bad_chunk);
            }
            const LocalSpan sp = LocalLayout::span(w.g, cursor, len - total, end);
            if (sp.n > 0) {
                CopyPool::get().copy(out + total, w.src + (sp.begin - w.g.start), size_t(sp.n));
                total += int32_t(sp.n);
                cursor = sp.begin + sp.n;
            }
            if (bad_chunk >= 0 && cursor >= end) break;
            if (cursor >= w.g.end()) give_slot_back(w, s);
        }
        return finish(total, bad_chunk, end, le);
    }

    // ---- read() into device memory ----------------------------------------------------------
    // Verification on: a window's bytes are already in HBM (load() uploaded them for the verify), so they go
    // from w.a.buf.d to d_out in one guarded delivery per window (deliver_dev: the kernel reads the window's result
    // word itself and copies only what it allows). The caller's thread does not wait for a window's result
    // before it enqueues: it waits for a window's `done` event only when it has nothing left to enqueue, to
    // give the slot back (the loader's next pread overwrites the PINNED window, which no stream orders against
    // the upload; the DEVICE copy needs no wait, the next upload into it is behind the delivery in the stream).
    // The deliveries of one call form a chain over the reader's two gate words, so after a bad window nothing
    // more is written, and the last gate word, read back once at the end, tells where the delivered bytes end.
    int ensure_device_words() {
        if (!dev.done) HIP_OK(hipEventCreateWithFlags(&dev.done, window_event_flags()));
        if (!verify) return 0;
        if (!dev.d_gate) HIP_OK(hipMalloc(reinterpret_cast<void **>(&dev.d_gate), 2 * sizeof(uint64_t)));
        if (!dev.h_gate)
            HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&dev.h_gate), sizeof(unsigned long long), pinned_host_flags()));
        if (!gate_zeroed) {
            HIP_OK(hipMemsetAsync(dev.d_gate, 0, 2 * sizeof(uint64_t), ctx->stream));
            gate_zeroed = true;
            gate_cur = 0;
        }
        return 0;
    }

    // an event behind everything this thread enqueued, waited for (not a drain: the loader may have queued
    // the next window's upload and verify behind it)
    int wait_enqueued() {
        HIP_OK(hipEventRecord(dev.done, ctx->stream));
        HIP_OK(hipEventSynchronize(dev.done));
        return 0;
    }

    int32_t read_dev(uint8_t *d_out, int32_t len) {
        if (error) return fail(error, "%s", error_msg.c_str());
        if (!d_out || len <= 0) return fail(-EINVAL, "invalid read buffer");
        DeviceGuard guard(ctx->device);
        if (!is_device_memory_of(ctx, d_out))
            return fail(-EINVAL, "read_dev: the buffer is not device memory of device %d", ctx->device);
        if (cursor >= lay.length) return 0;
        if (int rc = ensure_device_words()) return sticky(rc, std::string(hdfs3_crc_last_error()));
        return verify ? read_dev_verified(d_out, len) : read_dev_plain(d_out, len);
    }

    // verify off or CHECKSUM_NULL: nothing was uploaded, so the window's bytes go from w.src (the pinned window
    // or the mapping) to d_out with a runtime copy, waited for before the slot goes back. No kernel runs.
    int32_t read_dev_plain(uint8_t *d_out, int32_t len) {
        int32_t total = 0;
        LoadError le;
        while (total < len && cursor < lay.length) {
            const int s = next_ready(0, &le);
            if (s < 0) break;
            Window &w = slot[s];
            const LocalSpan sp = LocalLayout::span(w.g, cursor, len - total);
            if (sp.n > 0) {
                const hipError_t e = hipMemcpyAsync(d_out + total, w.src + (sp.begin - w.g.start), size_t(sp.n),
                                                    hipMemcpyHostToDevice, ctx->stream);
                int rc = e == hipSuccess ? 0 : hip_err(e, "hipMemcpyAsync");
                if (!rc) rc = wait_enqueued();
                if (rc) return sticky(rc, std::string(hdfs3_crc_last_error()));  // nothing is known to be in place
                total += int32_t(sp.n);
                cursor = sp.begin + sp.n;
                dev_bytes.fetch_add(uint64_t(sp.n), std::memory_order_relaxed);
            }
            if (cursor >= w.g.end()) give_slot_back(w, s);
        }
        return finish(total, -1, INT64_MAX, le);
    }

    int32_t read_dev_verified(uint8_t *d_out, int32_t len) {
        const int64_t from = cursor;
        int64_t pos = cursor;       // the enqueue cursor: deliveries for [from, pos) are in the stream
        size_t held = 0;            // windows at the front of `ready` wholly enqueued, slots not yet given back
        bool enqueued = false, chained = false, halt = false;
        int64_t bad_chunk = -1;     // the first bad chunk (block-relative), once a bad window is known,
        int64_t end = INT64_MAX;    // and where the deliverable bytes end before it
        LoadError le;
        // the front window was wholly enqueued: wait for its result; a good one's slot goes back to the loader
        auto settle_front = [&]() -> int {
            const int s = front_slot();
            Window &w = slot[s];
            if (int rc = wait(w)) return rc;
            if (w.bad_chunk >= 0) {
                halt = true;  // the deliveries behind it write nothing (the gate); nothing more is enqueued
                return 0;
            }
            give_slot_back(w, s);
            --held;
            return 0;
        };
        while (!halt && pos - from < len && pos < lay.length) {
            const int s = next_ready(held, &le);
            if (s < 0) {
                if (held == 0) break;  // the loader finished, or failed
                // nothing left to enqueue: only now wait for the oldest window's event, for its slot
                if (int rc = settle_front()) return sticky(rc, std::string(hdfs3_crc_last_error()));
                continue;
            }
            Window &w = slot[s];
            // a window an earlier call found bad stays at the front for the reader's life: the host knows where
            // its good bytes end, and the delivery needs no gate (the chain's own stays closed)
            const bool known_bad = w.verified && w.bad_chunk >= 0;
            if (known_bad) {
                bad_chunk = w.bad_chunk;
                end = lay.good_end(bad_chunk);
                halt = true;
            }
            const LocalSpan sp = LocalLayout::span(w.g, pos, len - (pos - from), end);
            if (sp.n > 0) {
                const CopyRange rg{uint64_t(sp.begin - w.g.start), uint64_t(sp.begin - from), uint64_t(sp.n)};
                const DeliverGuard g{reinterpret_cast<const uint64_t *>(w.a.res.d),
                                     known_bad ? nullptr : dev.d_gate + gate_cur,
                                     known_bad ? nullptr : dev.d_gate + (gate_cur ^ 1),
                                     0,
                                     w.g.chunk0,
                                     uint64_t(lay.buffer_size),
                                     chunk_size};
                unsigned launched = 0;
                const int rc = deliver_dev(ctx, d_out, size_t(len), w.a.buf.d, w.g.len, &rg, 1, g, &launched);
                dev_launches.fetch_add(launched, std::memory_order_relaxed);
                if (rc) return sticky(rc, std::string(hdfs3_crc_last_error()));  // nothing is known to be in place
                enqueued = true;
                if (!known_bad) {
                    gate_cur ^= 1;
                    chained = true;
                }
                pos = sp.begin + sp.n;
            }
            if (halt || pos < w.g.end()) break;  // a window consumed in part stays at the front
            ++held;
        }
        // the returned bytes are in place when the call returns: the chain's last gate word comes back behind
        // the last delivery, and says whether, and at which chunk, the chain stopped
        if (enqueued) {
            int rc = 0;
            if (chained) {
                const hipError_t e = hipMemcpyAsync(dev.h_gate, dev.d_gate + gate_cur, sizeof(unsigned long long),
                                                    hipMemcpyDeviceToHost, ctx->stream);
                if (e != hipSuccess) rc = hip_err(e, "hipMemcpyAsync");
            }
            if (!rc) rc = wait_enqueued();
            if (rc) return sticky(rc, std::string(hdfs3_crc_last_error()));
            if (chained && *dev.h_gate) {
                bad_chunk = hdfs3_crc_decode_result(*dev.h_gate);
                end = lay.good_end(bad_chunk);
            }
        }
        const int64_t reached = std::min(pos, std::max(end, from));
        const int32_t total = int32_t(reached - from);
        cursor = reached;
        dev_bytes.fetch_add(uint64_t(total), std::memory_order_relaxed);
        // every window a delivery was enqueued from has passed its event by now: the good ones this call
        // consumed go back, a bad one stays (and everything behind it)
        for (int s; (s = front_slot()) >= 0;) {
            Window &w = slot[s];
            if (w.g.start >= pos) break;  // not touched
            if (int rc = wait(w)) return sticky(rc, std::string(hdfs3_crc_last_error()));
            if (w.bad_chunk >= 0 || cursor < w.g.end()) break;
            give_slot_back(w, s);
        }
        return finish(total, bad_chunk, end, le);
    }

    int64_t available() {
        std::lock_guard<std::mutex> lk(mu);
        int64_t a = 0;
        for (int s : ready)
            if (slot[s].verified && slot[s].bad_chunk < 0)
                a += LocalLayout::available_in(slot[s].g, cursor);
        return a;
    }

    ~hdfs3_local_reader() {
        if (loader.joinable()) {
            {
                std::lock_guard<std::mutex> lk(mu);
                stop = true;
            }
            cv.notify_all();
            loader.join();
        }
        if (ctx) {
            LocalResources res;
            res.ctx = ctx;
            for (int i = 0; i < kSlots; ++i) res.a[i] = slot[i].a;
            res.dev = dev;
            // a ctx whose stream completes cleanly goes back to the pool for the next reader
            const bool clean = hipStreamSynchronize(ctx->stream) == hipSuccess;
            for (Window &w : slot) release_pages(w);  // no DMA is in flight any more
            if (clean && res.a[kSlots - 1].done)
                give_back(res);
            else
                drop_resources(res, /*destroy_ctx=*/false);
        }
        if (map) munmap(map, map_len);
        if (data_fd >= 0) ::close(data_fd);
        if (meta_fd >= 0) ::close(meta_fd);
    }
};

namespace hdfs3crc {

bool local_reader_host_fault(const hdfs3_local_reader *r) { return r && r->error && !r->replica_fault.load(); }

int local_opts_check(const hdfs3_local_opts *opts) {
    if (opts && (opts->flags & ~HDFS3_LOCAL_CRC32_AS_ZLIB)) return fail(-EINVAL, "unknown local reader flags");
    if (opts && opts->buffer_size > kLocalMaxBuffer) return fail(-EINVAL, "LocalBlockReader: local buffer above 1 GiB");
    return 0;
}

// kSlots windows of `bytes` each: pinned and device arena, result words, event. false: one allocation failed
// (the reader's destructor frees what was made).
static bool alloc_windows(Window (&slot)[kSlots], size_t bytes) {
    for (Window &w : slot) {
        PacketArena &a = w.a;
        if (a.buf.grow(bytes, pinned_host_flags()) != hipSuccess ||
            a.res.grow(sizeof(unsigned long long), pinned_host_flags()) != hipSuccess ||
            hipEventCreateWithFlags(&a.done, window_event_flags()) != hipSuccess)
            return false;
    }
    return true;
}

int open_local_reader(const char *data_path, const char *meta_path, int64_t num_bytes, int64_t offset,
                      const hdfs3_local_opts *opts, LocalOpenExtra *extra, hdfs3_local_reader **out) {
    if (!out || !data_path || !meta_path || offset < 0) return fail(-EINVAL, "invalid argument");
    const bool replica = extra && extra->replica;
    *out = nullptr;
    hdfs3_local_reader *r = new (std::nothrow) hdfs3_local_reader();
    if (!r) return fail(-ENOMEM, "reader allocation");
    auto bail = [&](int rc) {
        delete r;
        return rc;
    };
    std::string why;
    auto refused = [&](int rc) { return bail(fail(rc, "%s", why.c_str())); };
    const int device = opts ? opts->device : 0;
    if (opts) r->flags = opts->flags;
    if (opts && (opts->flags & ~HDFS3_LOCAL_CRC32_AS_ZLIB)) return bail(fail(-EINVAL, "unknown local reader flags"));
    r->data_fd = ::open(data_path, O_RDONLY | O_CLOEXEC);
    if (r->data_fd < 0) return bail(fail(-errno, "LocalBlockReader: cannot open block file %s", data_path));
    r->meta_fd = ::open(meta_path, O_RDONLY | O_CLOEXEC);
    if (r->meta_fd < 0) return bail(fail(-errno, "LocalBlockReader: cannot open meta file %s", meta_path));
    struct stat st;
    if (fstat(r->data_fd, &st) != 0) return bail(fail(-errno, "fstat failed"));
    const int64_t block_len = num_bytes > 0 ? num_bytes : int64_t(st.st_size);
    const bool short_file = block_len > int64_t(st.st_size);
    if (short_file && !replica) return bail(fail(-EIO, "block file shorter than the block length"));
    if (int rc = LocalLayout::check_offset(offset, block_len, &why)) return refused(rc);
    if (short_file && offset > int64_t(st.st_size)) return bail(fail(-EIO, "LocalBlockReader: offset beyond the block file"));
    if (int rc = r->open_meta(opts ? opts->verify != 0 : true)) return bail(rc);
    if (int rc = LocalLayout::make(offset, block_len, r->chunk_size, opts ? opts->buffer_size : 0,
                                   opts ? opts->window_buffers : 0, r->verify, extra ? extra->range_end : 0, &r->lay, &why))
        return refused(rc);
    const LocalLayout &lay = r->lay;
    r->cursor = offset;
    // mapped mode: verification off always (copies straight from the page cache); verified
    // reads only with HDFS3_LOCAL_MMAP=1, and only when every window starts on a page (first
    // and the window size page multiples), so windows register disjoint page ranges
    const char *mm = getenv("HDFS3_LOCAL_MMAP");
    r->map_verified = mm && mm[0] == '1' && r->verify && lay.first % kPage == 0 && lay.window % kPage == 0;
    // (a block file shorter than the block is never mapped: the pages past its end would fault, the pread fails)
    if (lay.length > 0 && !short_file && !(mm && mm[0] == '0') && (!r->verify || r->map_verified)) {
        r->map_len = size_t((lay.length + kPage - 1) / kPage * kPage);
        void *m = mmap(nullptr, r->map_len, PROT_READ, MAP_SHARED, r->data_fd, 0);
        if (m != MAP_FAILED) {
            r->map = static_cast<uint8_t *>(m);
            (void)madvise(m, r->map_len, MADV_SEQUENTIAL);
        } else {
            r->map_len = 0;
        }
    }
    // the files are in order: whatever fails from here on is this host's
    if (extra) extra->host_fault = true;
    // the windows live on `device`, whatever the calling thread's current device is
    DeviceGuard guard(device);
    LocalResources pooled;
    if (take_pooled(device, lay.arena_bytes(), &pooled)) {
        r->ctx = pooled.ctx;
        for (int i = 0; i < kSlots; ++i) r->slot[i].a = pooled.a[i];
        r->dev = pooled.dev;
    } else {
        if (int rc = ctx_acquire(device, &r->ctx)) return bail(rc);
        // the windows are pinned from a thread bound to the GPU's NUMA node (numa.h), so the
        // block file's pages are read into memory next to the GPU that DMAs them
        bool ok = true;
        if (!numa_binding_enabled()) {
            ok = alloc_windows(r->slot, lay.arena_bytes());  // binding off (the default): the caller's thread, under the guard
        } else {
            try {
                std::thread([&] {
                    (void)hipSetDevice(device);
                    bind_thread_to_device(device);
                    ok = alloc_windows(r->slot, lay.arena_bytes());
                }).join();
            } catch (const std::system_error &) {
                ok = false;  // no thread: never let the exception cross the extern "C" entry point
            }
        }
        if (!ok) return bail(fail(-ENOMEM, "LocalBlockReader: window allocation failed"));
    }
    if (int rc = hdfs3_crc_ctx_set_checksum_type(r->ctx, r->engine_type())) return bail(rc);
    for (int i = 0; i < kSlots; ++i) r->free_slots.push_back(i);
    if (lay.first < lay.length) {
        r->loader = std::thread([r] { r->run_loader(); });
    } else {
        r->load_done = true;
    }
    if (extra) extra->host_fault = false;
    *out = r;
    return 0;
}

}  // namespace hdfs3crc

extern "C" {

int hdfs3_local_reader_open(const char *data_path, const char *meta_path, int64_t num_bytes, int64_t offset,
                            const hdfs3_local_opts *opts, hdfs3_local_reader **out) {
    return open_local_reader(data_path, meta_path, num_bytes, offset, opts, nullptr, out);
}

int32_t hdfs3_local_reader_read(hdfs3_local_reader *r, void *buf, int32_t len) {
    if (!r) return fail(-EINVAL, "null reader");
    return r->read(static_cast<uint8_t *>(buf), len);
}

int32_t hdfs3_local_reader_read_dev(hdfs3_local_reader *r, void *d_buf, int32_t len) {
    if (!r) return fail(-EINVAL, "null reader");
    return r->read_dev(static_cast<uint8_t *>(d_buf), len);
}

int hdfs3_local_reader_device_stats(hdfs3_local_reader *r, uint64_t *deliver_launches, uint64_t *bytes_delivered) {
    if (!r) return fail(-EINVAL, "null reader");
    if (deliver_launches) *deliver_launches = r->dev_launches.load();
    if (bytes_delivered) *bytes_delivered = r->dev_bytes.load();
    return 0;
}

int64_t hdfs3_local_reader_available(hdfs3_local_reader *r) { return r ? r->available() : 0; }

int hdfs3_local_reader_stats(hdfs3_local_reader *r, uint32_t *bpc, int *checksum_type, uint64_t *gpu_batches) {
    if (!r) return fail(-EINVAL, "null reader");
    if (bpc) *bpc = r->chunk_size;
    if (checksum_type) *checksum_type = r->checksum_type;
    if (gpu_batches) *gpu_batches = r->batches.load();
    return 0;
}

uint64_t hdfs3_local_reader_mapped_windows(hdfs3_local_reader *r) { return r ? r->mapped_windows.load() : 0; }

int hdfs3_local_reader_close(hdfs3_local_reader *r) {
    delete r;
    return 0;
}

}  // extern "C"
