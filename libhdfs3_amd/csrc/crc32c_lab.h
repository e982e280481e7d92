// Lab-only device code of the round kernel's clock stamps: LabClock and the device symbols it writes
// through. Included by crc32c_wave.h in HDFS3_LAB builds only; the product library never sees it. Internal.
#pragma once

#include "crc32c_kernels.h"

namespace hdfs3crc {
namespace {

// Lab-only clock stamps (hdfs3x_clock_stamps, tools/clock_ramp.py): thread 0 of workgroup 0 of every
// launch of a stamping kernel records {s_memtime, s_memrealtime} at its start and end into the next
// slot of g_lab_clk (4 words per launch). s_memtime counts the shader clock and s_memrealtime a fixed
// 100 MHz, so the ratio of their deltas is the shader clock over that workgroup's lifetime. Vector
// stores and a vector atomic only; nothing when no buffer is set.
// With a wave buffer installed (hdfs3x_wave_stamps, tools/wave_spread.py) lane 0 of EVERY wave also
// records {realtime start, realtime end, shader clocks elapsed, HW_ID | XCC_ID << 32 | wave << 36 |
// launch << 52}:
// where each launch's time goes between its first wave's start and its last wave's end.
__device__ unsigned long long *g_lab_clk = nullptr;
__device__ unsigned int g_lab_clk_cap = 0;
__device__ unsigned int g_lab_clk_n = 0;
__device__ unsigned long long *g_lab_wave = nullptr;
__device__ unsigned int g_lab_wave_cap = 0;
struct LabClock {
    unsigned long long t0 = 0, r0 = 0;
    __device__ __forceinline__ void start() {
        if ((threadIdx.x & 63) == 0) {
            t0 = __builtin_amdgcn_s_memtime();
            r0 = __builtin_amdgcn_s_memrealtime();
        }
    }
    // seq: the launch's number (host counter g_lab_seq): wave w of launch seq owns slot
    // (seq * waves + w) % cap, so no two waves meet on an atomic (a shared counter serialised
    // 4,096 waves per launch and stretched a 128 MiB launch 8x)
    // word2: what word 2 of the wave's stamp holds (default: the shader clocks of its life)
    __device__ __forceinline__ void end(uint32_t seq = 0, unsigned long long word2 = ~0ull) {
        if ((threadIdx.x & 63) != 0) return;
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (blockIdx.x == 0 && threadIdx.x == 0 && g_lab_clk) {
            const unsigned int i = atomicAdd(&g_lab_clk_n, 1u);
            if (i < g_lab_clk_cap) {
                g_lab_clk[4 * i] = t0;
                g_lab_clk[4 * i + 1] = r0;
                g_lab_clk[4 * i + 2] = t1;
                g_lab_clk[4 * i + 3] = r1;
            }
        }
        if (g_lab_wave) {
            // HW_ID (hwreg 4, 32 bits: wave/simd/cu/sh/se) and XCC_ID (hwreg 20, low 4 bits)
            const unsigned long long hw = uint32_t(__builtin_amdgcn_s_getreg((31 << 11) | 4));
            const unsigned long long xcc = uint32_t(__builtin_amdgcn_s_getreg((3 << 11) | 20));
            const uint64_t wpl = uint64_t(gridDim.x) * (blockDim.x / 64);
            const uint64_t wv = uint64_t(blockIdx.x) * (blockDim.x / 64) + threadIdx.x / 64;
            const uint64_t i = (uint64_t(seq) * wpl + wv) % g_lab_wave_cap;
            g_lab_wave[4 * i] = r0;
            g_lab_wave[4 * i + 1] = r1;
            g_lab_wave[4 * i + 2] = word2 == ~0ull ? t1 - t0 : word2;
            g_lab_wave[4 * i + 3] = hw | (xcc & 15) << 32 | (wv & 0xFFFF) << 36 | uint64_t(seq & 0xFFF) << 52;
        }
    }
};

}  // namespace
}  // namespace hdfs3crc
