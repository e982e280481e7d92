// Where the loader of a short-circuit RANGE read stops (the input stream's pread over a local replica).
// Plain arithmetic, no GPU runtime: tests/native/local_range_check.cpp includes this header alone.
//
// The reference's LocalBlockReader takes no range end (LocalBlockReader.cpp:201-206): it verifies whole
// localBufferSize refills, counted from the chunk-aligned first byte it read, so a pread of a few bytes
// checks the whole buffer that holds them and nothing after it. The same rule here: the loader stops at
// the end of the buffer_size buffer that holds the range's last byte, clipped to the block.
#pragma once

#include <algorithm>
#include <cstdint>

namespace hdfs3crc {

// first: the first byte the loader reads (chunk aligned when verifying); range_end: one past the range's
// last byte, block-relative (<= 0: no range end, the block's); buffer_size > 0. Returns the block offset
// the loader stops at, in [min(first, block_len), block_len].
inline int64_t local_read_limit(int64_t first, int64_t range_end, int64_t buffer_size, int64_t block_len) {
    if (block_len <= 0) return 0;
    if (first >= block_len) return block_len;
    if (range_end <= 0 || range_end >= block_len || buffer_size <= 0 || first < 0) return block_len;
    const int64_t last = std::max(range_end - 1, first);  // an empty range still names the buffer it starts in
    const int64_t buffers = (last - first) / buffer_size + 1;
    if (buffers > (block_len - first) / buffer_size) return block_len;  // also keeps the product in range
    return first + buffers * buffer_size;
}

}  // namespace hdfs3crc
