// CPU check of the short-circuit reader's geometry (libhdfs3_amd/csrc/client/local_layout.h), built with
// -fsanitize=address,undefined by tests/test_local_layout.py. Includes that header alone: no GPU runtime,
// no block file, no loader thread. The expected figures come from the reader's rules, walked byte by byte
// or chunk by chunk here, not from the header's own formulas.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "client/local_layout.h"

using namespace hdfs3crc;

static int failures = 0;

#define EXPECT(cond, ...)                                          \
    do {                                                           \
        if (!(cond) && ++failures <= 20) {                         \
            std::printf("line %d: %s: ", __LINE__, #cond);         \
            std::printf(__VA_ARGS__);                              \
            std::printf("\n");                                     \
        }                                                          \
    } while (0)

using ll = long long;
static const int64_t kMiB = 1 << 20, kGiB = 1 << 30;

static LocalLayout made(int64_t offset, int64_t len, uint32_t chunk, int32_t buf, int wbuf, bool verify = true,
                        int64_t range_end = 0) {
    LocalLayout l;
    std::string why;
    const int rc = LocalLayout::make(offset, len, chunk, buf, wbuf, verify, range_end, &l, &why);
    EXPECT(rc == 0, "offset %lld len %lld chunk %u buf %d: %d %s", (ll)offset, (ll)len, chunk, buf, rc, why.c_str());
    return l;
}

static std::vector<LocalWindow> windows_of(const LocalLayout &l) {
    std::vector<LocalWindow> ws;
    for (int64_t at = l.first; at < l.length; at += ws.back().len) ws.push_back(l.window_at(at));
    return ws;
}

// The withholding rule against the model, the host's count against the kernel's, and the tiling, over small
// blocks: chunk sizes 1, 3, 512, 513, 4096; buffers of 1 to 3 chunks (asked for whole and one byte short,
// which rounds up to the same); 1 and 2 buffers per window; a block of three windows and a chunk and a half
static void small_blocks() {
    for (uint32_t chunk : {1u, 3u, 512u, 513u, 4096u})
        for (int bufchunks = 1; bufchunks <= 3; ++bufchunks)
            for (int wbuf = 1; wbuf <= 2; ++wbuf)
                for (int shy = 0; shy <= (chunk > 1 ? 1 : 0); ++shy) {
                    const int64_t buf = int64_t(bufchunks) * chunk, window = wbuf * buf;
                    const int64_t len = 3 * window + chunk + (chunk + 1) / 2;  // the last chunk is short (chunk > 1)
                    const int64_t last_chunk = (len - 1) / chunk;
                    for (int64_t offset : {int64_t(0), int64_t(1), int64_t(chunk) - 1, int64_t(chunk), len - 1}) {
                        const LocalLayout l = made(offset, len, chunk, int32_t(buf - shy), wbuf);
                        const int64_t first = offset / chunk * chunk;
                        EXPECT(l.buffer_size == buf && l.first == first && l.length == len && l.window == window,
                               "chunk %u buf %lld offset %lld: %d %lld %lld %u", chunk, (ll)buf, (ll)offset, l.buffer_size,
                               (ll)l.first, (ll)l.length, l.window);
                        // byte b is deliverable iff its buffer, counted from first, lies before the buffer of the
                        // bad chunk's first byte
                        for (int64_t bad = first / chunk; bad <= last_chunk; ++bad) {
                            const int64_t end = l.good_end(bad), bad_buffer = (bad * chunk - first) / buf;
                            for (int64_t b = first; b < len; ++b)
                                if ((b < end) != ((b - first) / buf < bad_buffer)) {
                                    EXPECT(false, "chunk %u buf %lld offset %lld bad %lld: byte %lld, good_end %lld", chunk,
                                           (ll)buf, (ll)offset, (ll)bad, (ll)b, (ll)end);
                                    break;
                                }
                        }
                        // the windows tile [first, len); chunks and .meta words as a walk of the block's chunks gives
                        const std::vector<LocalWindow> ws = windows_of(l);
                        int64_t at = first, c = first / chunk;
                        for (const LocalWindow &w : ws) {
                            int64_t starts = 0;  // chunks that begin inside the window
                            while (c + starts <= last_chunk && (c + starts) * chunk < w.end()) ++starts;
                            EXPECT(w.start == at && w.len > 0 && (w.len == window || w.end() == len), "window at %lld + %u",
                                   (ll)w.start, w.len);
                            EXPECT((w.start - first) % window == 0 && (w.start - first) % buf == 0 && w.start % chunk == 0,
                                   "window at %lld is not on a window, buffer and chunk boundary", (ll)w.start);
                            EXPECT(int64_t(w.chunk0) == c && int64_t(w.chunks) == starts, "window at %lld: chunks %llu + %llu",
                                   (ll)w.start, (unsigned long long)w.chunk0, (unsigned long long)w.chunks);
                            EXPECT(w.meta_off == 7 + 4 * c && int64_t(w.meta_bytes) == 4 * starts && w.meta_bytes <= l.crc_bytes,
                                   "window at %lld: meta %lld + %zu", (ll)w.start, (ll)w.meta_off, w.meta_bytes);
                            EXPECT(w.len <= l.cap_data && l.cap_data + w.meta_bytes <= l.arena_bytes(), "arena");
                            // the kernel counts granules from the window's first byte, the host buffers from `first`
                            for (int64_t bad = c; bad < c + starts; ++bad) {
                                const uint64_t lim = deliver_limit(~uint64_t(bad - c), 0, 0, uint64_t(buf), chunk);
                                const int64_t dev = w.start + int64_t(std::min<uint64_t>(lim, w.len));
                                const int64_t host = std::min(std::max(l.good_end(bad), w.start), w.end());
                                EXPECT(dev == host && w.start + int64_t(lim) == l.good_end(bad),
                                       "chunk %u buf %lld offset %lld window %lld bad %lld: device %lld host %lld", chunk,
                                       (ll)buf, (ll)offset, (ll)w.start, (ll)bad, (ll)dev, (ll)host);
                            }
                            at = w.end();
                            c += starts;
                        }
                        EXPECT(at == len && c == last_chunk + 1 && ws.size() == size_t((len - first + window - 1) / window),
                               "tiling ends at %lld, chunk %lld, %zu windows", (ll)at, (ll)c, ws.size());
                        if (chunk > 1) EXPECT(ws.back().end() % chunk != 0, "the last window ends in the block's short chunk");
                    }
                }
}

static void refused(int64_t offset, int64_t len, uint32_t chunk, int32_t buf, bool verify, const char *text) {
    LocalLayout l;
    std::string why;
    const int rc = LocalLayout::make(offset, len, chunk, buf, 4, verify, 0, &l, &why);
    EXPECT(rc == -EINVAL && why == text, "rc %d, '%s', want '%s'", rc, why.c_str(), text);
}

static void edges() {
    // a buffer that is no chunk multiple rounds up
    EXPECT(made(0, 10 * kMiB, 513, 1 << 20, 1).buffer_size == 2045 * 513, "1 MiB at chunk 513");
    EXPECT(made(0, 10 * kMiB, 517, 1 << 20, 1).buffer_size == 2029 * 517, "1 MiB at chunk 517");
    for (uint32_t chunk : {513u, 517u}) {
        const LocalLayout l = made(chunk + 1, 10 * kMiB, chunk, 1 << 20, 0);
        EXPECT(l.buffer_size % chunk == 0 && l.buffer_size >= kMiB && l.buffer_size - chunk < kMiB, "%d", l.buffer_size);
        EXPECT(l.first == chunk && l.window == 4u * l.buffer_size, "default of 4 buffers per window: %u", l.window);
        EXPECT(l.cap_data % 256 == 0 && l.cap_data >= l.window && l.cap_data < l.window + 256, "cap_data %zu", l.cap_data);
        EXPECT(l.crc_bytes == 4 * size_t(4 * (l.buffer_size / chunk)), "crc_bytes %zu", l.crc_bytes);
    }
    EXPECT(made(0, kMiB, 512, 0, 0).buffer_size == kMiB && made(0, kMiB, 512, -3, -1).window == 4 * kMiB, "defaults");
    // the 1 GiB bound, before and after rounding
    EXPECT(made(0, 4 * kGiB, 512, int32_t(kGiB), 4).buffer_size == kGiB, "1 GiB is accepted");
    EXPECT(made(0, 4 * kGiB, 512, int32_t(kGiB - 511), 4).buffer_size == kGiB, "rounds to 1 GiB: accepted");
    refused(0, 4 * kGiB, 513, int32_t(kGiB - 1), true,
            "LocalBlockReader: local buffer of 1073741832 bytes (chunk-rounded) exceeds 1073741824");
    refused(0, 4 * kGiB, 512, int32_t(kGiB + 1), true,
            "LocalBlockReader: local buffer of 1073742336 bytes (chunk-rounded) exceeds 1073741824");
    refused(0, 4 * kGiB, uint32_t(INT32_MAX), 1 << 20, true,  // the largest chunk a .meta header may declare
            "LocalBlockReader: local buffer of 2147483647 bytes (chunk-rounded) exceeds 1073741824");
    EXPECT(made(0, 4 * kGiB, 512, int32_t(kGiB), 4, false).buffer_size == kGiB, "verify off, 1 GiB");
    refused(0, 4 * kGiB, 512, int32_t(kGiB + 1), false, "LocalBlockReader: local buffer above 1 GiB");
    refused(101, 100, 512, 0, true, "offset beyond the block");
    refused(101, 100, 0, 0, false, "offset beyond the block");
    std::string why;
    EXPECT(LocalLayout::check_offset(100, 100, &why) == 0 && LocalLayout::check_offset(101, 100, &why) == -EINVAL &&
               why == "offset beyond the block", "check_offset: %s", why.c_str());
    // a window is whole buffers, at most 1 GiB, at least one buffer
    EXPECT(made(0, 4 * kGiB, 512, 1 << 20, 2048).window == kGiB, "1024 buffers of 1 MiB");
    EXPECT(made(0, 4 * kGiB, 512, 384 << 20, 4).window == 768u * kMiB, "2 buffers of 384 MiB");
    EXPECT(made(0, 4 * kGiB, 512, (512 << 20) + 512, 4).window == 512u * kMiB + 512, "one buffer above half a GiB");
    EXPECT(made(0, 4 * kGiB, 512, int32_t(kGiB), 4).window == kGiB, "one buffer of 1 GiB");
    // offset == length: nothing to read, unless the block ends in a short chunk that holds the offset's predecessors
    EXPECT(windows_of(made(4096, 4096, 512, 1024, 2)).empty(), "offset == length, whole chunks");
    EXPECT(windows_of(made(4100, 4100, 512, 1024, 2, false)).empty(), "offset == length, verify off");
    const std::vector<LocalWindow> tail = windows_of(made(4100, 4100, 512, 1024, 2));
    EXPECT(tail.size() == 1 && tail[0].start == 4096 && tail[0].len == 4 && tail[0].chunk0 == 8 && tail[0].chunks == 1,
           "offset == length inside the tail chunk: that chunk is still read and verified");
    EXPECT(windows_of(made(0, 0, 512, 1024, 2)).empty(), "an empty block");
    // verify off: no rounding, no alignment, no words (a CHECKSUM_NULL .meta has no chunk size at all)
    for (uint32_t chunk : {0u, 512u}) {
        const LocalLayout l = made(777, 100000, chunk, 1000, 3, false);
        EXPECT(l.first == 777 && l.buffer_size == 1000 && l.window == 3000 && l.crc_bytes == 0 && l.cap_data == 3072, "off");
        const std::vector<LocalWindow> ws = windows_of(l);
        EXPECT(ws.size() == 34 && ws[0].start == 777 && ws[0].chunks == 0 && ws[0].meta_bytes == 0 && ws[33].end() == 100000 &&
                   ws[33].len == 100000 - 777 - 33 * 3000, "verify off: %zu windows", ws.size());
    }
    // the range end goes through local_read_limit, counted from the chunk-aligned first byte
    EXPECT(made(513, 300001, 512, 64 << 10, 2, true, 523).length == 512 + (64 << 10), "a short range");
    EXPECT(made(513, 300001, 512, 64 << 10, 2, true, 513 + (64 << 10)).length == 512 + 2 * (64 << 10), "two buffers");
    EXPECT(made(513, 300001, 512, 64 << 10, 2, true, 0).length == 300001, "no range end");
    for (int64_t end : {-1, 1, 600, 70000, 299999, 300001, 400000}) {
        const LocalLayout l = made(600, 300001, 100, 1000, 2, true, end), off = made(600, 300001, 100, 999, 2, false, end);
        EXPECT(l.length == local_read_limit(600, end, 1000, 300001), "range end %lld: %lld", (ll)end, (ll)l.length);
        EXPECT(off.length == local_read_limit(600, end, 999, 300001), "range end %lld, verify off", (ll)end);
        const std::vector<LocalWindow> ws = windows_of(l);
        EXPECT(!ws.empty() && ws.back().end() == l.length, "the windows end at the limit");
    }
}

static void spans() {
    LocalWindow w;
    w.start = 100, w.len = 50;
    auto is = [&](int64_t cursor, int64_t want, int64_t limit, int64_t begin, int64_t n) {
        const LocalSpan s = LocalLayout::span(w, cursor, want, limit);
        EXPECT(s.begin == begin && s.n == n, "cursor %lld want %lld limit %lld: %lld + %lld", (ll)cursor, (ll)want, (ll)limit,
               (ll)s.begin, (ll)s.n);
    };
    is(90, 10, INT64_MAX, 100, 10);    // a cursor before the window starts at the window
    is(90, 1000, INT64_MAX, 100, 50);
    is(100, 1, INT64_MAX, 100, 1);
    is(120, 1, INT64_MAX, 120, 1);     // inside: a want of 1 byte, and one beyond the window
    is(120, 1000, INT64_MAX, 120, 30);
    is(149, 1000, INT64_MAX, 149, 1);
    is(150, 1000, INT64_MAX, 150, 0);  // at the end
    is(160, 1000, INT64_MAX, 160, 0);
    is(120, 1000, 130, 120, 10);       // an end limit inside, at and beyond the window's end
    is(120, 5, 130, 120, 5);
    is(120, 1000, 150, 120, 30);
    is(120, 1000, 200, 120, 30);
    is(120, 1000, 120, 120, 0);        // an end limit at and before the cursor: nothing, never negative
    is(120, 1000, 110, 120, 0);
    is(120, 1000, 0, 120, 0);
    is(90, 1000, 95, 100, 0);
    is(120, 0, INT64_MAX, 120, 0);
    EXPECT(LocalLayout::span(w, 120, 1000).n == 30, "no limit given");
    EXPECT(LocalLayout::available_in(w, 90) == 50 && LocalLayout::available_in(w, 100) == 50 &&
               LocalLayout::available_in(w, 120) == 30 && LocalLayout::available_in(w, 150) == 0, "available");
}

int main() {
    small_blocks();
    edges();
    spans();
    if (failures) return 1;
    std::printf("local layout ok\n");
    return 0;
}
