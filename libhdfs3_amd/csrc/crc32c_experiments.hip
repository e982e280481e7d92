// Kernel variants kept for in-process A/B and diagnostics (hdfs3x_set_variant, tools/ab.py;
// docs/DESIGN_HISTORY.md §5.0), the read-ceiling and access-pattern kernels of the bench
// (stream_read_kernel, lane_read_kernel), the clock stamps' host side (crc32c_lab.h). Linked into the measurement
// library libhdfs3_crc_lab.so only (HDFS3_LAB=1); the product libhdfs3_crc.so never sees it.
// Bit-exact variants are parity-tested (tests/test_gpu_parity.py); the diagnostic one gives
// wrong results on purpose. The designs that lost their A/B were removed in round 3; their
// numbers stay in docs/DESIGN_HISTORY.md §5 and profiles/.
#include <cerrno>

#include "crc32c_wave.h"
#include "ctx.h"
#include "hdfs3_crc.h"

namespace hdfs3crc {
namespace {

// ---- measurement-only kernels ------------------------------------------------

// Coalesced streaming read (1 KiB per wave-instruction): the achievable HBM read
// ceiling the CRC kernel is compared with.
template <bool NT>
__global__ __launch_bounds__(256) void stream_read_kernel(const uint8_t *__restrict__ d,
                                                          uint64_t n16, uint32_t *sink, uint32_t seq) {
    auto ld = [](const uint8_t *p) -> u32x4 {
        if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
        return ld16(p);
    };
    LabClock clk;
    clk.start();
    uint32_t acc = 0;
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const u32x4 a = ld(d + 16 * i), b = ld(d + 16 * (i + stride));
        const u32x4 c = ld(d + 16 * (i + 2 * stride)), e = ld(d + 16 * (i + 3 * stride));
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ e.x ^ e.y ^
               e.z ^ e.w;
    }
    for (; i < n16; i += stride) {
        const u32x4 a = ld(d + 16 * i);
        acc ^= a.x ^ a.y ^ a.z ^ a.w;
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;  // keep the loads live
    clk.end(seq);
}

// Access-pattern probes (xor instead of table arithmetic), selected by `variant`:
//  0: chunk per lane, 8 x 16 B per 128 B line, nt loads   (the v1 CRC kernel's pattern)
//  1: same, default cache policy
//  2: G=8 lanes per chunk, one full 128 B line per chunk per instruction (coalesced)
//  3: G=4 lanes per chunk, 64 B per chunk per instruction
//  4: chunk per lane, 2 x 16 B (32 B) per lane per instruction pair, lines split over 4 lanes
template <int BPC, int VARIANT>
__global__ __launch_bounds__(kBlockThreads) void lane_read_kernel(const uint8_t *__restrict__ d,
                                                                  uint64_t nchunks, uint32_t *sink) {
    uint32_t acc = 0;
    const uint64_t tid = uint64_t(blockIdx.x) * kBlockThreads + threadIdx.x;
    const uint64_t nthreads = uint64_t(gridDim.x) * kBlockThreads;
    if constexpr (VARIANT <= 1) {
        for (uint64_t chunk = tid; chunk < nchunks; chunk += nthreads) {
            const uint8_t *p = d + chunk * BPC;
#pragma unroll
            for (int l = 0; l < BPC / 128; ++l) {
                u32x4 v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const u32x4 *q = reinterpret_cast<const u32x4 *>(p + 128 * l + 16 * i);
                    v[i] = VARIANT == 0 ? __builtin_nontemporal_load(q) : *q;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) acc = (acc ^ v[i].x ^ v[i].y ^ v[i].z ^ v[i].w) * 3u;
            }
        }
    } else if constexpr (VARIANT == 2 || VARIANT == 3) {
        constexpr int G = VARIANT == 2 ? 8 : 4;
        const uint64_t groups = nthreads / G;
        for (uint64_t chunk = tid / G; chunk < nchunks; chunk += groups) {
            const uint8_t *p = d + chunk * BPC + 16 * (tid % G);
            constexpr int N = BPC / (16 * G), U = N < 8 ? N : 8;
#pragma unroll
            for (int t0 = 0; t0 < N; t0 += U) {
                u32x4 v[U];
#pragma unroll
                for (int i = 0; i < U; ++i) v[i] = *reinterpret_cast<const u32x4 *>(p + 16 * G * (t0 + i));
#pragma unroll
                for (int i = 0; i < U; ++i) acc = (acc ^ v[i].x ^ v[i].y ^ v[i].z ^ v[i].w) * 3u;
            }
        }
    } else {
        for (uint64_t chunk = tid; chunk < nchunks; chunk += nthreads) {
            const uint8_t *p = d + chunk * BPC;
#pragma unroll
            for (int l = 0; l < BPC / 128; ++l) {
                u32x4 v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const u32x4 *>(p + 128 * l + 16 * ((i * 2) % 8 + (i / 4)));
#pragma unroll
                for (int i = 0; i < 8; ++i) acc = (acc ^ v[i].x ^ v[i].y ^ v[i].z ^ v[i].w) * 3u;
            }
        }
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;
}

template <int BPC, bool V>
hipError_t launch_exp(const LaunchEnv &env, int variant, const ChunkLaunch &a) {
    const auto [tab, fold, grid_cap, s] = std::tie(env.tables, env.fold, env.grid_cap, env.stream);
    if constexpr (BPC > kRoundBytes) {
        if (variant == 115) return launch_r3<BPC, V, true>(a, tab, fold, grid_cap, s);  // s_setprio
        if (variant == 123) return launch_r3<BPC, V>(a, tab, fold, grid_cap, s);  // multi-round kernel
    }
    if constexpr (BPC <= kRoundBytes) {
        switch (variant) {
        case 92:  // production with the prefetch issued at the start of each step (early)
            return launch_wave3<BPC, V, false, true, kLabEarly>(a, tab, fold, grid_cap, s);
        case 93:  // production without the solo last step (overlapped verifies end interleaved)
            return launch_wave3<BPC, V, false, false>(a, tab, fold, grid_cap, s);
        case 94:  // the solo last step for overlapped verifies only (round-3 production before r3i)
            return launch_wave3<BPC, V, false, V>(a, tab, fold, grid_cap, s);
        case 95:  // compute: each round's words stored at once everywhere (Words::kPerRound)
            return launch_wave3<BPC, V, false, true, kLabNoHold>(a, tab, fold, grid_cap, s);
        case 77:  // diagnostic: production with the table lookups replaced by an XOR (wrong results)
            return launch_wave3<BPC, V, false, true, kLabNoMath>(a, tab, fold, grid_cap, s);
        case 99:    // the pitch walk over this contiguous block as ONE packet (power-of-two rounds only)
        case 100: {  // the pitch walk over it as 8 equal packets (blocks of one 2-D tensor)
            const uint64_t units = a.len / kRoundBytes;
            const uint64_t npk = variant == 99 ? 1 : 8;
            const uint64_t upp = units / npk;
            if (a.len % kRoundBytes || units % npk || (upp & (upp - 1)) || a.chunk_base) return hipErrorInvalidValue;
            ChunkLaunch p = a;
            p.npk = npk;
            p.pitch = upp * kRoundBytes;
            p.crc_pitch = upp * (kRoundBytes / BPC) * 4;
            p.last_len = uint32_t(upp * kRoundBytes);
            if (!packet_geom(p.pitch, p.last_len, npk, BPC, &p.geom)) return hipErrorInvalidValue;
            return launch_wave3<BPC, V, true, false>(p, tab, fold, grid_cap, s);
        }
        case 115:  // s_setprio by rounds left at every launch size (production: waves of >= 16 rounds)
            return launch_wave3<BPC, V, false, true, kLabPrio>(a, tab, fold, grid_cap, s);
        case 117:  // no s_setprio at any size (production before r3y)
            return launch_wave3<BPC, V, false, true, kLabNoPrio>(a, tab, fold, grid_cap, s);
        case 118:  // diagnostic, compute: held words not stored (wrong results)
            return launch_wave3<BPC, V, false, true, kLabNoStore>(a, tab, fold, grid_cap, s);
        case 119:  // diagnostic, compute: held words stored over the wave's first round's words (wrong results)
            return launch_wave3<BPC, V, false, true, kLabNearStore>(a, tab, fold, grid_cap, s);
        case 123:  // (chunks above 4 KiB take the multi-round kernel; this size is production)
            return launch_wave3<BPC, V, false, true>(a, tab, fold, grid_cap, s);
        case 122:  // compute: held stores where production stages the words in LDS (before r3zb)
            return launch_wave3<BPC, V, false, true, kLabNoStage>(a, tab, fold, grid_cap, s);
        case 130:  // compute: staged words at every size, written out window by window (kLabStageWin)
            return launch_wave3<BPC, V, false, true, kLabStageWin>(a, tab, fold, grid_cap, s);
        case 128:  // compute: staged words through plain global stores (production before round 4)
            return launch_wave3<BPC, V, false, true, kLabStorePlain>(a, tab, fold, grid_cap, s);
        case 146:  // production with every wave's fill-done and first-data times (wave_spread.py --variant 146 --mid)
            return launch_wave3<BPC, V, false, true, kLabClock | kLabMid>(a, tab, fold, grid_cap, s);
        case 147:  // diagnostic: no table loads (wrong results), with fill-done / first-data stamps
            return launch_wave3<BPC, V, false, true, kLabNoTabLoad | kLabClock | kLabMid>(a, tab, fold, grid_cap, s);
        case 148:  // diagnostic: no table loads (wrong results)
            return launch_wave3<BPC, V, false, true, kLabNoTabLoad>(a, tab, fold, grid_cap, s);
        case 137:  // verify: 1024-thread workgroups at every launch size (production before round 4)
            return launch_wave3<BPC, V, false, true, kLabWg1024>(a, tab, fold, grid_cap, s);
        case 162:  // launches of <= 4096 units (16 MiB): one round per wave, twice the workgroups (round 6)
            return launch_wave3<BPC, V, false, true, kLabOneRound>(a, tab, fold, grid_cap, s);
        case 132:  // 256-thread workgroups (4 waves each): small launches spread over 4x the CUs
            return launch_wave3<BPC, V, false, true, 0, 256>(a, tab, fold, grid_cap, s);
        case 134:  // 512-thread workgroups (8 waves each)
            return launch_wave3<BPC, V, false, true, 0, 512>(a, tab, fold, grid_cap, s);
        case 125:  // production with clock stamps of workgroup 0 (kLabClock; tools/clock_ramp.py)
            return launch_wave3<BPC, V, false, true, kLabClock>(a, tab, fold, grid_cap, s);
        case 78:  // diagnostic: 77 without the slice-table LDS fill
            return launch_wave3<BPC, V, false, true, kLabNoMath | kLabNoFill>(a, tab, fold, grid_cap, s);
        default: return hipErrorInvalidValue;
        }
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_experiment(const LaunchEnv &env, int variant, const ChunkLaunch &a, bool verify) {
    return dispatch_bpc<true>(a.bpc, [&](auto bpc) {
        return verify ? launch_exp<bpc(), true>(env, variant, a) : launch_exp<bpc(), false>(env, variant, a);
    });
}

void set_variant(int v) { g_variant = v; }

hipError_t lab_clock_buffer(unsigned long long *d, unsigned int cap, unsigned int *n_out) {
    // read the count of the previous buffer first, then install the new one with a zero count
    unsigned int n = 0;
    hipError_t e = hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_lab_clk_n), sizeof n);
    if (e != hipSuccess) return e;
    if (n_out) *n_out = n;
    const unsigned int zero = 0;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(g_lab_clk), &d, sizeof d)) != hipSuccess) return e;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(g_lab_clk_cap), &cap, sizeof cap)) != hipSuccess) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_lab_clk_n), &zero, sizeof zero);
}

hipError_t lab_wave_buffer(unsigned long long *d, unsigned int cap, unsigned int *n_out) {
    // *n_out = launches stamped since the previous install; the launch counter restarts at 0
    if (n_out) *n_out = g_lab_seq.exchange(0);
    hipError_t e;
    const unsigned long long *none = nullptr;  // no stamps while the pair changes
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(g_lab_wave), &none, sizeof none)) != hipSuccess) return e;
    if (!d || !cap) return hipSuccess;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(g_lab_wave_cap), &cap, sizeof cap)) != hipSuccess) return e;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_lab_wave), &d, sizeof d);
}

hipError_t launch_stream_read(const uint8_t *d, uint64_t len, uint32_t *sink, int grid,
                              hipStream_t stream, bool overlap_previous) {
    // grid < 0: non-temporal loads over |grid| workgroups (the production kernels' policy);
    // overlap_previous: AQL packet without the barrier bit, as the overlapped verify launches
    const bool nt = grid < 0;
    const dim3 g(nt ? -grid : grid), b(256);
    auto k = nt ? stream_read_kernel<true> : stream_read_kernel<false>;
    if (overlap_previous)
        hipExtLaunchKernelGGL(k, g, b, 0, stream, nullptr, nullptr, hipExtAnyOrderLaunch, d, len / 16, sink,
                              g_lab_seq++);
    else
        hipLaunchKernelGGL(k, g, b, 0, stream, d, len / 16, sink, g_lab_seq++);
    return hipGetLastError();
}

hipError_t launch_lane_read(const uint8_t *d, uint64_t len, uint32_t bpc, uint32_t *sink,
                            int grid_cap, hipStream_t stream) {
    const int variant = int(bpc >> 16);  // probe selector rides in the high bits of bpc
    bpc &= 0xFFFFu;
    const uint64_t chunks = len / bpc;
    const uint64_t lanes = variant == 2 ? chunks * 8 : variant == 3 ? chunks * 4 : chunks;
    const uint64_t need = (lanes + kBlockThreads - 1) / kBlockThreads;
    const int grid = int(need < uint64_t(grid_cap) ? need : uint64_t(grid_cap));
#define LR(B, V) hipLaunchKernelGGL((lane_read_kernel<B, V>), dim3(grid), dim3(kBlockThreads), 0, stream, d, chunks, sink)
#define LRV(B)                          \
    switch (variant) {                  \
    case 0: LR(B, 0); break;            \
    case 1: LR(B, 1); break;            \
    case 2: LR(B, 2); break;            \
    case 3: LR(B, 3); break;            \
    default: LR(B, 4); break;           \
    }
    switch (bpc) {
    case 512: LRV(512); break;
    case 2048: LRV(2048); break;
    case 4096: LRV(4096); break;
    default: return hipErrorInvalidValue;
    }
#undef LRV
#undef LR
    return hipGetLastError();
}

}  // namespace hdfs3crc

// ---- measurement hooks (bench.py's read ceiling, tools/, the A/B tests). Not part of hdfs3_crc.h;
// like the rest of this file they exist in libhdfs3_crc_lab.so only. ----
using namespace hdfs3crc;

extern "C" {

// Coalesced read-only stream over [d, d+len): the achievable HBM read ceiling.
int hdfs3x_stream_read_ex(hdfs3_crc_ctx *ctx, const void *d, size_t len, int grid, void *d_sink, uint32_t flags);
int hdfs3x_stream_read(hdfs3_crc_ctx *ctx, const void *d, size_t len, int grid, void *d_sink) {
    return hdfs3x_stream_read_ex(ctx, d, len, grid, d_sink, 0);
}

// flags: HDFS3_LAUNCH_OVERLAP_PREVIOUS, for the same-shape ceiling of overlapped verifies
int hdfs3x_stream_read_ex(hdfs3_crc_ctx *ctx, const void *d, size_t len, int grid, void *d_sink, uint32_t flags) {
    if (!ctx) return fail(-EINVAL, "null ctx");
    DeviceGuard g(ctx->device);
    HIP_TRY(launch_stream_read(static_cast<const uint8_t *>(d), len, static_cast<uint32_t *>(d_sink),
                               grid != 0 ? grid : ctx->grid_cap * 8, ctx->stream,
                               (flags & HDFS3_LAUNCH_OVERLAP_PREVIOUS) != 0));
    return 0;
}

// The CRC kernel's chunk-per-lane access pattern without the table arithmetic.
int hdfs3x_lane_read(hdfs3_crc_ctx *ctx, const void *d, size_t len, uint32_t bpc, void *d_sink) {
    if (!ctx) return fail(-EINVAL, "null ctx");
    DeviceGuard g(ctx->device);
    HIP_TRY(launch_lane_read(static_cast<const uint8_t *>(d), len, bpc, static_cast<uint32_t *>(d_sink),
                             ctx->grid_cap, ctx->stream));
    return 0;
}

int hdfs3x_grid_cap(hdfs3_crc_ctx *ctx) { return ctx ? ctx->grid_cap : 0; }

// Process-wide kernel-variant knob for in-process A/B measurements (tools/ab.py).
void hdfs3x_set_variant(int v) { set_variant(v); }

// Clock stamps of variant 125 and the stream-read kernel (tools/clock_ramp.py): installs a device
// buffer of cap x 4 u64 ({s_memtime, s_memrealtime} at workgroup 0's start and end, one slot per
// launch); returns the number of stamps written into the previous buffer, or a negative errno.
int hdfs3x_clock_stamps(void *d_buf, unsigned int cap) {
    unsigned int n = 0;
    HIP_TRY(lab_clock_buffer(static_cast<unsigned long long *>(d_buf), cap, &n));
    return int(n);
}

int hdfs3x_wave_stamps(void *d_buf, unsigned int cap) {
    unsigned int n = 0;
    HIP_TRY(lab_wave_buffer(static_cast<unsigned long long *>(d_buf), cap, &n));
    return int(n);
}

}  // extern "C"
