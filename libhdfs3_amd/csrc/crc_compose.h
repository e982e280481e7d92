// Composite CRC arithmetic: CRCs of adjacent byte ranges combined without their data. Plain host
// arithmetic, no GPU runtime (tests/native/crc_compose_check.cpp); crc32c_compose.hip runs the same
// reduction on the device with multipliers computed here.
//
// A CRC value is a polynomial over GF(2) modulo P in the reflected representation of the stored
// words: bit 31 is x^0, bit 0 is x^31 (x^0 = 0x80000000, x^8 = 0x00800000); `poly` is P in that
// form without its x^32 term (kPolyReflected, kPolyCrc32). For finished CRCs (init ~0, final xor ~0)
//   crc(A || B) = crc(A) * x^(8 |B|) ^ crc(B)   (mod P),
// since the init and final xor terms of the two sides cancel: no un-finalising, and the empty range
// has CRC 0, the neutral element of the composition.
#pragma once

#include <cstddef>
#include <cstdint>

#include "crc32c_tables.h"

namespace hdfs3crc {

constexpr uint32_t kXpow0 = 0x80000000u;  // x^0
constexpr uint32_t kXpow8 = 0x00800000u;  // x^8: one zero byte

// a * b in GF(2)[x] / P
uint32_t mulmod(uint32_t a, uint32_t b, uint32_t poly);
// x^(8n) mod P for any n: square-and-multiply on (x^8)^n, so 8n is never formed
uint32_t xpow_bytes(uint64_t n, uint32_t poly);
// CRC of A || B from crc_a = crc(A), crc_b = crc(B) and len_b = |B|
uint32_t compose(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t poly);

// The composite of n stored big-endian words (4 bytes each at crc_be, any alignment): every word covers
// bpc bytes but the last, which covers last_len (1..bpc). n == 0: 0.
uint32_t composite_of_words(const void *crc_be, uint64_t n, uint32_t bpc, uint32_t last_len, uint32_t poly);
// The composite of a file from its blocks' CRCs (host order) and byte lengths, in block order
uint32_t composite_of_blocks(const uint32_t *block_crcs, const uint64_t *block_lens, size_t n_blocks, uint32_t poly);

}  // namespace hdfs3crc
