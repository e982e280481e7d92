// The short-circuit reader's geometry: the chunk-rounded local buffer, the first byte read, where the loader
// stops, the GPU windows and their chunks and .meta words, where the good bytes of a corrupt block end, and
// the span of a window a read may take. Plain host arithmetic: no GPU runtime, no files, no threads
// (tests/native/local_layout_check.cpp includes this header alone).
//
// THE INVARIANT. window % buffer_size == 0, and when verifying first % chunk_size == 0 and buffer_size %
// chunk_size == 0. Windows are laid from `first`, so every window's first byte is first + k * window: a
// chunk boundary and a buffer boundary. That is why the host, which counts buffers from `first` (good_end),
// and the guarded delivery kernel, which counts granules of buffer_size from the window's first byte
// (launch_plan.h: deliver_limit), name the same byte as the end of a corrupt block's good bytes.
#pragma once

#include <algorithm>
#include <cassert>
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>

#include "../launch_plan.h"
#include "local_range.h"

namespace hdfs3crc {

constexpr int kLocalMetaHeader = 7;                  // HEADER_SIZE: version 2 + type 1 + bpc 4
constexpr int32_t kLocalDefaultBuffer = 1 << 20;     // input.localread.default.buffersize
constexpr int kLocalDefaultWindowBuffers = 4;        // 4 MiB windows: first delivery sooner (docs/DESIGN_HISTORY.md §5.1)
constexpr int32_t kLocalMaxBuffer = 1 << 30;         // largest local buffer / window

// One GPU window: block bytes [start, start + len), and when verifying its chunks (block-relative) and
// where their words lie in the .meta file
struct LocalWindow {
    int64_t start = 0;
    uint32_t len = 0;
    uint64_t chunk0 = 0, chunks = 0;
    int64_t meta_off = 0;
    size_t meta_bytes = 0;
    int64_t end() const { return start + len; }
};

struct LocalSpan {
    int64_t begin, n;  // n >= 0
};

struct LocalLayout {
    bool verify = true;
    uint32_t chunk_size = 0;
    int32_t buffer_size = kLocalDefaultBuffer;  // localBufferSize (chunk-rounded when verifying)
    int64_t first = 0;                          // first byte the loader reads (chunk aligned when verifying)
    int64_t length = 0;                         // where the loader stops: the block's end, or the range's limit
    uint32_t window = 0;                        // bytes per GPU window (whole buffers)
    size_t cap_data = 0, crc_bytes = 0;         // an arena is [data (cap_data)][crc words]
    size_t arena_bytes() const { return cap_data + crc_bytes; }

    static int refuse(std::string *why, std::string text) {
        *why = std::move(text);
        return -EINVAL;
    }
    // The first refusal of an open, made before the .meta header is read (make() repeats it)
    static int check_offset(int64_t offset, int64_t block_len, std::string *why) {
        return offset > block_len ? refuse(why, "offset beyond the block") : 0;
    }

    // The geometry of a reader opened at `offset` of a block of block_len bytes (0 <= offset). buffer_size
    // and window_buffers <= 0 take the defaults; range_end as local_read_limit takes it. 0, or the refusal's
    // code with its text in *why.
    static int make(int64_t offset, int64_t block_len, uint32_t chunk_size, int32_t buffer_size, int window_buffers,
                    bool verify, int64_t range_end, LocalLayout *out, std::string *why) {
        if (int rc = check_offset(offset, block_len, why)) return rc;
        LocalLayout l;
        l.verify = verify;
        l.chunk_size = chunk_size;
        if (buffer_size > 0) l.buffer_size = buffer_size;
        if (verify) {  // chunk-rounded local buffer (:112-116); reads start on a chunk (skip, :232-263)
            const int64_t rounded = (int64_t(l.buffer_size) + chunk_size - 1) / chunk_size * chunk_size;
            if (rounded > kLocalMaxBuffer)
                return refuse(why, "LocalBlockReader: local buffer of " + std::to_string(rounded) +
                                       " bytes (chunk-rounded) exceeds " + std::to_string(kLocalMaxBuffer));
            l.buffer_size = int32_t(rounded);
            l.first = offset / chunk_size * chunk_size;
        } else {
            if (l.buffer_size > kLocalMaxBuffer) return refuse(why, "LocalBlockReader: local buffer above 1 GiB");
            l.first = offset;
        }
        // a range read ends with the buffer that holds the range's last byte: from here on that is the block's end
        l.length = local_read_limit(l.first, range_end, l.buffer_size, block_len);
        // whole buffers per window, at least one (the buffer itself is at most 1 GiB)
        const int wbuf = window_buffers > 0 ? window_buffers : kLocalDefaultWindowBuffers;
        l.window = uint32_t(std::max<int64_t>(1, std::min<int64_t>(wbuf, kLocalMaxBuffer / l.buffer_size)) * l.buffer_size);
        l.cap_data = (size_t(l.window) + 255) & ~size_t(255);
        l.crc_bytes = verify ? 4 * ((size_t(l.window) + chunk_size - 1) / chunk_size) : 0;
        assert(l.window % uint32_t(l.buffer_size) == 0);
        assert(!verify || (l.first % chunk_size == 0 && uint32_t(l.buffer_size) % chunk_size == 0));
        *out = l;
        return 0;
    }

    // The window that starts at `start` = first + k * window < length
    LocalWindow window_at(int64_t start) const {
        LocalWindow w;
        w.start = start;
        w.len = uint32_t(std::min<int64_t>(window, length - start));
        if (!verify) return w;
        w.chunk0 = uint64_t(start) / chunk_size;
        w.chunks = (uint64_t(w.len) + chunk_size - 1) / chunk_size;
        w.meta_off = kLocalMetaHeader + 4 * int64_t(w.chunk0);
        w.meta_bytes = size_t(4 * w.chunks);
        return w;
    }

    // THE WITHHOLDING RULE (readAndVerify verifies one buffer_size buffer before any of it is returned):
    // the good bytes of a block whose first bad chunk is bad_chunk end where the buffer, counted from `first`,
    // that holds the chunk's first byte begins
    int64_t good_end(int64_t bad_chunk) const {
        const int64_t bad_off = bad_chunk * int64_t(chunk_size);
        return first + (bad_off - first) / buffer_size * int64_t(buffer_size);
    }

    // What a read at `cursor` that still wants `want` bytes may take of w, below `limit` (a good_end). The
    // cursor never lies before the front window: windows tile the block from first <= offset.
    static LocalSpan span(const LocalWindow &w, int64_t cursor, int64_t want, int64_t limit = INT64_MAX) {
        const int64_t begin = std::max(cursor, w.start);
        return LocalSpan{begin, std::max<int64_t>(0, std::min(std::min(w.end(), limit) - begin, want))};
    }

    // bytes of a verified, good window at or behind the cursor: what available() sums
    static int64_t available_in(const LocalWindow &w, int64_t cursor) { return w.end() - std::max(cursor, w.start); }
};

}  // namespace hdfs3crc
