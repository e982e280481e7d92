// CPU check of the composite CRC arithmetic (libhdfs3_amd/csrc/crc_compose.cpp), built with the host
// compiler under ASan + UBSan by tests/test_crc_compose.py. The references here share no code with it:
// a product in the unreflected representation (carry-less multiply to 64 bits, then a bitwise
// reduction), the one-zero-byte advance of the bitwise CRC register, and a bitwise CRC over buffers.
#include <cstdio>
#include <vector>

#include "crc_compose.h"

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

const uint32_t kPolys[2] = {kPolyReflected, kPolyCrc32};

uint64_t g_rng = 0x243F6A8885A308D3ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

uint32_t bitrev(uint32_t v) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}

// the product a second way: bit i = x^i, 64-bit carry-less product, reduced by x^32 + P from the top
uint32_t ref_mul(uint32_t a, uint32_t b, uint32_t poly) {
    const uint64_t full = (uint64_t(1) << 32) | bitrev(poly);
    const uint64_t ua = bitrev(a), ub = bitrev(b);
    uint64_t p = 0;
    for (int i = 0; i < 32; ++i)
        if ((ua >> i) & 1u) p ^= ub << i;
    for (int i = 63; i >= 32; --i)
        if ((p >> i) & 1u) p ^= full << (i - 32);
    return bitrev(uint32_t(p));
}

// one zero byte through the bitwise CRC register: times x^8
uint32_t advance_byte(uint32_t s, uint32_t poly) {
    for (int k = 0; k < 8; ++k) s = (s >> 1) ^ ((s & 1u) ? poly : 0u);
    return s;
}

uint32_t crc_bytewise(const uint8_t *p, size_t n, uint32_t poly) {
    uint32_t s = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        s ^= p[i];
        for (int k = 0; k < 8; ++k) s = (s >> 1) ^ ((s & 1u) ? poly : 0u);
    }
    return ~s;
}

// x^(8 * 2^k) by k squarings of x^8 with the reference product
uint32_t ref_xpow_pow2(int k, uint32_t poly) {
    uint32_t v = kXpow8;
    for (int i = 0; i < k; ++i) v = ref_mul(v, v, poly);
    return v;
}

void check_mulmod() {
    for (uint32_t poly : kPolys) {
        for (int i = 0; i < 20000; ++i) {
            const uint32_t a = uint32_t(rnd()), b = uint32_t(rnd());
            CHECK(mulmod(a, b, poly) == mulmod(b, a, poly), "a %08x b %08x", a, b);
            CHECK(mulmod(a, b, poly) == ref_mul(a, b, poly), "a %08x b %08x", a, b);
            CHECK(mulmod(a, kXpow0, poly) == a && mulmod(kXpow0, a, poly) == a, "a %08x", a);
            CHECK(mulmod(a, 0, poly) == 0 && mulmod(0, a, poly) == 0, "a %08x", a);
        }
        // (x^a)(x^b) = x^(a+b), exponents in bytes up to 2^40
        for (int i = 0; i < 4000; ++i) {
            const uint64_t a = rnd() >> (24 + rnd() % 40), b = rnd() >> (24 + rnd() % 40);
            CHECK(mulmod(xpow_bytes(a, poly), xpow_bytes(b, poly), poly) == xpow_bytes(a + b, poly), "a %llu b %llu",
                  (unsigned long long)a, (unsigned long long)b);
        }
        const uint64_t top = uint64_t(1) << 40;
        CHECK(mulmod(xpow_bytes(top, poly), xpow_bytes(top, poly), poly) == xpow_bytes(2 * top, poly), "2^40");
        CHECK(mulmod(xpow_bytes(top, poly), xpow_bytes(top - 1, poly), poly) == xpow_bytes(2 * top - 1, poly), "2^40 - 1");
    }
}

void check_xpow() {
    for (uint32_t poly : kPolys) {
        uint32_t s = kXpow0;
        for (uint64_t n = 0; n <= 70000; ++n) {
            CHECK(xpow_bytes(n, poly) == s, "n %llu", (unsigned long long)n);
            s = advance_byte(s, poly);
        }
        CHECK(xpow_bytes(1, poly) == kXpow8, "x^8");
        // 2^32 - 1, 2^32, 2^32 + 1 and 2^63 from the squarings done with the reference product
        const uint32_t p32 = ref_xpow_pow2(32, poly);
        CHECK(xpow_bytes(uint64_t(1) << 32, poly) == p32, "2^32");
        CHECK(xpow_bytes((uint64_t(1) << 32) + 1, poly) == advance_byte(p32, poly), "2^32 + 1");
        CHECK(advance_byte(xpow_bytes((uint64_t(1) << 32) - 1, poly), poly) == p32, "2^32 - 1");
        uint32_t below = kXpow0;  // x^(8 (2^32 - 1)) = the product of x^(8 2^k), k < 32
        for (int k = 0; k < 32; ++k) below = ref_mul(below, ref_xpow_pow2(k, poly), poly);
        CHECK(xpow_bytes((uint64_t(1) << 32) - 1, poly) == below, "2^32 - 1");
        CHECK(xpow_bytes(uint64_t(1) << 63, poly) == ref_xpow_pow2(63, poly), "2^63");
        CHECK(xpow_bytes(~uint64_t(0), poly) != 0, "2^64 - 1");  // x is a unit: no power is 0
    }
}

void check_compose() {
    std::vector<uint8_t> buf(5000);
    for (auto &b : buf) b = uint8_t(rnd());
    for (uint32_t poly : kPolys) {
        CHECK(crc_bytewise(buf.data(), 0, poly) == 0, "empty");
        CHECK(crc_bytewise(reinterpret_cast<const uint8_t *>("123456789"), 9, poly) ==
                  (poly == kPolyReflected ? 0xE3069283u : 0xCBF43926u),
              "check value");
        for (size_t total : {size_t(0), size_t(1), size_t(2), size_t(63), size_t(512), size_t(513), size_t(5000)}) {
            const uint32_t whole = crc_bytewise(buf.data(), total, poly);
            for (size_t cut : {size_t(0), size_t(1), total / 2, total ? total - 1 : 0, total}) {
                if (cut > total) continue;
                const uint32_t a = crc_bytewise(buf.data(), cut, poly);
                const uint32_t b = crc_bytewise(buf.data() + cut, total - cut, poly);
                CHECK(compose(a, b, total - cut, poly) == whole, "total %zu cut %zu", total, cut);
            }
        }
        // Horner over chunk CRCs, as stored big-endian words, and over blocks
        const size_t cases[][2] = {{0, 512}, {1, 512}, {511, 512}, {512, 512}, {513, 512}, {5000, 512}, {1000, 7},
                                   {4097, 4096}};
        for (const auto &c : cases) {
            const size_t total = c[0], bpc = c[1], n = (total + bpc - 1) / bpc;
            std::vector<uint8_t> words(4 * n + 1);
            std::vector<uint32_t> crcs(n);
            std::vector<uint64_t> lens(n);
            for (size_t i = 0; i < n; ++i) {
                lens[i] = total - i * bpc < bpc ? total - i * bpc : bpc;
                crcs[i] = crc_bytewise(buf.data() + i * bpc, lens[i], poly);
                for (int k = 0; k < 4; ++k) words[1 + 4 * i + k] = uint8_t(crcs[i] >> (24 - 8 * k));  // unaligned
            }
            const uint32_t whole = crc_bytewise(buf.data(), total, poly);
            const uint32_t last = n ? uint32_t(lens[n - 1]) : 0;
            CHECK(composite_of_words(words.data() + 1, n, uint32_t(bpc), last, poly) == whole, "total %zu bpc %zu",
                  total, bpc);
            CHECK(composite_of_blocks(crcs.data(), lens.data(), n, poly) == whole, "total %zu bpc %zu", total, bpc);
        }
    }
}

}  // namespace

int main() {
    check_mulmod();
    check_xpow();
    check_compose();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("crc compose ok\n");
    return 0;
}
