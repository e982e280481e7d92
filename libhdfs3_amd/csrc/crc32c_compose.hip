// gfx950 (CDNA4) composite CRC: the CRC of a whole block from its stored chunk words, without the data.
//
// With X = x^(8 unit) in GF(2)[x] / P (crc_compose.h), the composite of n words w_0 .. w_{n-1}, all of
// `unit` bytes but the last of `tail` bytes, is
//   C = (sum_{i < n-1} w_i X^(n-2-i)) x^(8 tail) ^ w_{n-1}.
// The sum over the m = n - 1 whole chunks is a tree reduction whose multipliers depend only on a
// node's span, never on the lane: they are computed on the host and travel in the kernel arguments
// (scalar registers), and a product with one of them is 32 select-and-xor steps on the lane's value
// while the scalar unit multiplies the multiplier by x. The words are taken right-aligned: the grid
// covers G * kComposeSpan >= m virtual words whose first G * kComposeSpan - m are zero, the neutral
// element, so every span of the tree is full and the last word's multiplier is x^0 at every level.
//
//   lane       Horner over kComposeLaneWords consecutive words with X
//   wave       6 butterfly steps (__shfl_xor): the earlier half of a pair times X^(K 2^s), xor the later
//   workgroup  the 4 wave values through LDS, 2 more steps on the first wave -> one partial
//   grid       one big-endian partial per workgroup; the same kernel over the partials with
//              X' = X^kComposeSpan until one workgroup is left, which applies the tail step
//
// 128 MiB at bpc 512 is 2^18 words = 1 MiB: 256 workgroups, then 1. Latency-bound by its two launches.
#include "crc32c_kernels.h"
#include "crc_compose.h"

namespace hdfs3crc {

namespace {

constexpr int kComposeSteps = 8;  // 64 lanes x 4 waves
static_assert(kComposeThreads == 256 && (1 << kComposeSteps) == kComposeThreads, "6 wave steps + 2 LDS steps");

// one level's multipliers (kernel arguments)
struct ComposeMul {
    uint32_t unit;                 // X: the lane's Horner step
    uint32_t step[kComposeSteps];  // X^(kComposeLaneWords 2^s): a pair of nodes of 2^s lanes each
    uint32_t tail;                 // x^(8 tail): the last level's final step
};

// a * b mod P, b the same in every lane: its multiples by x stay in scalar registers
__device__ __forceinline__ uint32_t mulmod_uniform(uint32_t a, uint32_t b, uint32_t poly) {
    uint32_t p = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        p ^= uint32_t(-int32_t((a >> (31 - k)) & 1u)) & b;
        b = (b >> 1) ^ ((b & 1u) ? poly : 0u);
    }
    return p;
}

// Workgroup g reduces virtual words [g * kComposeSpan, (g + 1) * kComposeSpan); virtual word v is
// w_be[v - pad], zero below pad (gridDim.x * kComposeSpan = m + pad). last_be == null: the partial goes
// big-endian to out[g]. last_be != null (one workgroup): out[0] = partial * mul.tail ^ *last_be, host order.
__global__ __launch_bounds__(kComposeThreads) void crc_compose_kernel(const uint32_t *__restrict__ w_be, uint64_t m,
                                                                       uint64_t pad, ComposeMul mul, uint32_t poly,
                                                                       const uint32_t *__restrict__ last_be,
                                                                       uint32_t *__restrict__ out) {
    __shared__ uint32_t wave_value[kComposeThreads / 64];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t v0 = uint64_t(blockIdx.x) * kComposeSpan + uint64_t(threadIdx.x) * kComposeLaneWords;
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < kComposeLaneWords; ++j) {
        const uint64_t v = v0 + j;
        const uint32_t w = v >= pad && v - pad < m ? __builtin_bswap32(w_be[v - pad]) : 0u;
        acc = (j ? mulmod_uniform(acc, mul.unit, poly) : 0u) ^ w;
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const uint32_t t = (lane >> s) & 1u ? acc : mulmod_uniform(acc, mul.step[s], poly);
        acc = t ^ __shfl_xor(t, 1 << s);
    }
    if (lane == 0) wave_value[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    acc = wave_value[lane & 3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint32_t t = (lane >> s) & 1u ? acc : mulmod_uniform(acc, mul.step[6 + s], poly);
        acc = t ^ __shfl_xor(t, 1 << s);
    }
    if (threadIdx.x != 0) return;
    if (last_be) out[0] = mulmod_uniform(acc, mul.tail, poly) ^ __builtin_bswap32(*last_be);
    else out[blockIdx.x] = __builtin_bswap32(acc);
}

}  // namespace

void ComposeScratch::release() {
    if (words) (void)hipFree(words);
    if (partials) (void)hipFree(partials);
    *this = ComposeScratch();
}

hipError_t grow_compose_buffer(uint8_t **d, uint64_t *cap, uint64_t need, hipStream_t stream) {
    if (need <= *cap) return hipSuccess;
    if (*d) {
        if (hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return e;
        (void)hipFree(*d);
    }
    *d = nullptr;
    *cap = 0;
    if (hipError_t e = hipMalloc(reinterpret_cast<void **>(d), need); e != hipSuccess) return e;
    *cap = need;
    return hipSuccess;
}

hipError_t launch_compose_words(const LaunchEnv &env, ComposeScratch *scratch, const uint8_t *d_crc_be, uint64_t n,
                                uint32_t unit, uint32_t tail, uint32_t poly, uint32_t *d_out, unsigned *launched) {
    if (launched) *launched = 0;
    if (!scratch || !d_crc_be || !d_out || n == 0 || n > kComposeMaxWords || unit == 0 || tail == 0 || tail > unit ||
        (reinterpret_cast<uintptr_t>(d_crc_be) & 3u) != 0)
        return hipErrorInvalidValue;
    const uint32_t *last = reinterpret_cast<const uint32_t *>(d_crc_be) + (n - 1);
    uint64_t m = n - 1;  // the whole chunks
    uint64_t grid = m ? (m + kComposeSpan - 1) / kComposeSpan : 1;
    if (grid > 1) {
        // every level's partials, one after the other: grid + grid / kComposeSpan + ... + a word per level
        const uint64_t need = (grid + grid / (kComposeSpan - 1) + 8) * 4;
        if (hipError_t e = grow_compose_buffer(&scratch->partials, &scratch->partials_cap, need, env.stream);
            e != hipSuccess)
            return e;
    }
    ComposeMul mul{};
    mul.unit = xpow_bytes(unit, poly);
    mul.tail = xpow_bytes(tail, poly);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(d_crc_be);
    uint32_t *partials = reinterpret_cast<uint32_t *>(scratch->partials);
    for (;;) {
        uint32_t sq = mul.unit;  // X^(K 2^s) by squaring (K = 4): no exponent is formed, so none overflows
        for (int k = 1; k < kComposeLaneWords; k <<= 1) sq = mulmod(sq, sq, poly);
        for (int s = 0; s < kComposeSteps; ++s, sq = mulmod(sq, sq, poly)) mul.step[s] = sq;
        const bool final_level = grid == 1;
        hipLaunchKernelGGL(crc_compose_kernel, dim3(uint32_t(grid)), dim3(kComposeThreads), 0, env.stream, src, m,
                           grid * kComposeSpan - m, mul, poly, final_level ? last : nullptr,
                           final_level ? d_out : partials);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (launched) ++*launched;
        if (final_level) return hipSuccess;
        // the next level: this one's partials, each covering kComposeSpan of its units
        src = partials;
        partials += grid;
        m = grid;
        grid = (m + kComposeSpan - 1) / kComposeSpan;
        mul.unit = sq;  // X^kComposeSpan
    }
}

}  // namespace hdfs3crc
