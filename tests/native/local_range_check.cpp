// CPU check of csrc/client/local_range.h (where the loader of a short-circuit range read stops), built with
// -fsanitize=address,undefined by tests/test_local_range.py. Includes that header alone.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "client/local_range.h"

using hdfs3crc::local_read_limit;

static int failures = 0;

#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                               \
        }                                                             \
    } while (0)

// the definition, buffer by buffer: the end of the first buffer (counted from `first`) that holds last byte
static int64_t slow(int64_t first, int64_t range_end, int64_t buf, int64_t len) {
    if (first >= len) return len;
    if (range_end <= 0 || range_end >= len) return len;
    int64_t end = first;
    do {
        end += buf;
    } while (end < range_end && end < len);
    return end < len ? end : len;
}

int main() {
    const int64_t K = 64 << 10;
    // the shapes of tests/test_input_stream_local.py: 64 KiB buffers, chunk 512
    EXPECT(local_read_limit(0, 1, K, 300001) == K);
    EXPECT(local_read_limit(0, K, K, 300001) == K);
    EXPECT(local_read_limit(0, K + 1, K, 300001) == 2 * K);
    EXPECT(local_read_limit(512, K, K, 300001) == 512 + K);        // buffers are counted from the first byte read
    EXPECT(local_read_limit(512, 513 + K, K, 300001) == 512 + 2 * K);
    EXPECT(local_read_limit(4 * K, 4 * K + 10, K, 300001) == 300001);  // the block's short last buffer
    EXPECT(local_read_limit(0, 300001, K, 300001) == 300001);
    EXPECT(local_read_limit(0, 0, K, 300001) == 300001);            // no range end
    EXPECT(local_read_limit(0, -5, K, 300001) == 300001);
    EXPECT(local_read_limit(0, 400000, K, 300001) == 300001);
    EXPECT(local_read_limit(300001, 300001, K, 300001) == 300001);  // nothing to read
    EXPECT(local_read_limit(1024, 1024, K, 300001) == 1024 + K);    // an empty range names its first buffer
    EXPECT(local_read_limit(0, 10, K, 0) == 0);
    // no overflow at the largest sizes the reader takes
    const int64_t G = int64_t(1) << 30, big = INT64_MAX - 7;
    EXPECT(local_read_limit(0, big - 1, G, big) == big);
    EXPECT(local_read_limit(big - G - 3, big - 2, G, big) == big);
    EXPECT(local_read_limit(0, 5, G, big) == G);
    // against the definition
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t m) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return int64_t(x % m);
    };
    for (int i = 0; i < 200000; ++i) {
        const int64_t chunk = int64_t(1) << rnd(13), buf = chunk * (1 + rnd(40)), len = 1 + rnd(3000000);
        const int64_t first = rnd(uint64_t(len + 1)) / chunk * chunk;
        const int64_t range_end = first + rnd(uint64_t(len - first + 2));
        const int64_t got = local_read_limit(first, range_end, buf, len), want = slow(first, range_end, buf, len);
        if (got != want) {
            std::printf("first %lld end %lld buf %lld len %lld: %lld, want %lld\n", (long long)first, (long long)range_end,
                        (long long)buf, (long long)len, (long long)got, (long long)want);
            if (++failures > 10) break;
        }
        // the limit covers the range and is a whole number of buffers from `first`, or the block's end
        if (range_end > first) EXPECT(got >= (range_end < len ? range_end : len));
        EXPECT(got == len || (got - first) % buf == 0);
    }
    if (failures) return 1;
    std::printf("local range ok\n");
    return 0;
}
