// Composite CRC arithmetic (crc_compose.h).
#include "crc_compose.h"

namespace hdfs3crc {

uint32_t mulmod(uint32_t a, uint32_t b, uint32_t poly) {
    // a's terms from x^0 (bit 31) upwards, b multiplied by x at every step
    uint32_t p = 0;
    for (uint32_t m = kXpow0; m && a; m >>= 1) {
        if (a & m) {
            p ^= b;
            a &= ~m;
        }
        b = (b >> 1) ^ ((b & 1u) ? poly : 0u);
    }
    return p;
}

uint32_t xpow_bytes(uint64_t n, uint32_t poly) {
    uint32_t r = kXpow0, sq = kXpow8;  // sq = (x^8)^(2^k)
    for (; n; n >>= 1) {
        if (n & 1u) r = mulmod(r, sq, poly);
        sq = mulmod(sq, sq, poly);
    }
    return r;
}

uint32_t compose(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t poly) {
    return mulmod(crc_a, xpow_bytes(len_b, poly), poly) ^ crc_b;
}

uint32_t composite_of_words(const void *crc_be, uint64_t n, uint32_t bpc, uint32_t last_len, uint32_t poly) {
    const uint8_t *w = static_cast<const uint8_t *>(crc_be);
    const uint32_t full = xpow_bytes(bpc, poly);
    uint32_t r = 0;
    for (uint64_t i = 0; i < n; ++i, w += 4) {
        const uint32_t v = uint32_t(w[0]) << 24 | uint32_t(w[1]) << 16 | uint32_t(w[2]) << 8 | uint32_t(w[3]);
        r = mulmod(r, i + 1 == n && last_len != bpc ? xpow_bytes(last_len, poly) : full, poly) ^ v;
    }
    return r;
}

uint32_t composite_of_blocks(const uint32_t *block_crcs, const uint64_t *block_lens, size_t n_blocks, uint32_t poly) {
    uint32_t r = 0;
    for (size_t i = 0; i < n_blocks; ++i) r = compose(r, block_crcs[i], block_lens[i], poly);
    return r;
}

}  // namespace hdfs3crc
