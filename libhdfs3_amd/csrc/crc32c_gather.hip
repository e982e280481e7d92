// Byte-exact range gather: one launch copies up to kGatherMaxRanges ranges {src_off, dst_off, len} from
// one device buffer to another (launch_plan.h: GatherLaunch, planned by plan_gather_launch). The block
// reader's device delivery: a verified batch's packets go from the arena's device copy to the caller's
// device buffer in one launch instead of one runtime copy per packet.
//
// Work is split by destination bytes: a range is cut into tiles of kGatherTileBytes of the aligned
// 16-byte destination lines it touches, and workgroup w finds its range from the tile prefix sums in the
// kernel arguments (everything about the range is then wave-uniform, held in scalar registers). A lane
// owns whole destination lines:
//   - a line that lies inside the range is one aligned 16-byte store, fed by the one or two aligned
//     16-byte source quads that hold its bytes, shifted by k = (source - destination) mod 16, the same
//     for every line of the range;
//   - a range's first and last line may be partial: only the range's own bytes are written, byte by
//     byte, never the line read back and merged, so two ranges that abut inside one line (copied by
//     different workgroups) cannot disturb each other.
// No load touches memory outside [src, src + src_len) and no store memory outside [dst, dst + dst_len):
// a quad's load is an aligned 16-byte one only when the whole quad lies inside the source buffer, else
// (the first and last quad of a buffer whose ends are not 16-byte aligned) the line's bytes are loaded
// one by one, each tested against the buffer. A buffer resource's range check cannot serve here: it
// drops a 16-byte load whole when its last byte is out of range, and the bytes before it are needed.
//
// The gather with a source per range (the kernel's third instantiation; the output stream's vectored write
// from device memory) is the same copy with each range's src_off an ADDRESS and the range its own source
// buffer: the bound above then holds per range, so nothing next to a caller's tensor is ever read, at the
// price of at most two byte-loaded lines per range.
//
// The guarded delivery (the kernel's second instantiation) is the same copy behind a verify's result
// word: it reads that word and a chain word on the device, clips every range to the limit they give
// (launch_plan.h: deliver_limit) and leaves the chain word for the next delivery, so verify -> copy ->
// verify -> copy can sit on one stream with no host read in between and the destination still never
// holds an unverified byte.
#include <hip/hip_runtime.h>

#include "crc32c_kernels.h"

namespace hdfs3crc {

namespace {

typedef uint32_t u32x4g __attribute__((ext_vector_type(4)));
// a source address out of the kernel arguments read as a global one (a pointer made from an integer is flat)
#define HDFS3_GLOBAL __attribute__((address_space(1)))

// bytes k .. k+15 of the 32 bytes {lo, hi}, k = 4 j + b
__device__ __forceinline__ u32x4g shift_quads(const u32x4g lo, const u32x4g hi, uint32_t j, uint32_t b) {
    uint32_t w[5];
    switch (j) {  // wave-uniform
    case 0: w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w, w[4] = hi.x; break;
    case 1: w[0] = lo.y, w[1] = lo.z, w[2] = lo.w, w[3] = hi.x, w[4] = hi.y; break;
    case 2: w[0] = lo.z, w[1] = lo.w, w[2] = hi.x, w[3] = hi.y, w[4] = hi.z; break;
    default: w[0] = lo.w, w[1] = hi.x, w[2] = hi.y, w[3] = hi.z, w[4] = hi.w; break;
    }
    u32x4g o;
    // v_alignbyte_b32: ({w[i+1], w[i]} >> 8 b), low 32 bits
    o.x = __builtin_amdgcn_alignbyte(w[1], w[0], b);
    o.y = __builtin_amdgcn_alignbyte(w[2], w[1], b);
    o.z = __builtin_amdgcn_alignbyte(w[3], w[2], b);
    o.w = __builtin_amdgcn_alignbyte(w[4], w[3], b);
    return o;
}

// One kernel, three instantiations. Without a guard argument (launch_gather) it is the plain gather. With one
// (launch_deliver: Guard = DeliverGuard) it is the guarded delivery, the same copy behind a verify's result
// word: every workgroup reads the two guard words itself (uniform loads, once) and derives the limit, a source
// offset at which every range ends, so the copy is ordered behind the verify on the device and the host never
// reads the result in between. One lane of the launch leaves the chain word for the next delivery; gate_out
// aliases neither word read here (checked by the host), since other workgroups of the launch may still be
// reading them. A delivery with g.n == 0 only passes the gate on.
// kOwnSource (launch_gather_sources): src and src_len are unused, a range's src_off is its source address
// and [src_off, src_off + len) the only bytes its workgroups may load.
template <bool kOwnSource, typename... Guard>
__global__ __launch_bounds__(kGatherThreads) void gather_ranges_kernel(uint8_t *dst, uint64_t dst_len, const uint8_t *src,
                                                                       uint64_t src_len, const GatherLaunch g,
                                                                       const Guard... guard) {
    constexpr bool kGuarded = sizeof...(Guard) != 0;
    uint64_t limit = kDeliverNoLimit;
    if constexpr (kGuarded) {
        const DeliverGuard &gd = (guard, ...);
        const uint64_t result = *gd.result;
        const uint64_t gate_in = gd.gate_in ? *gd.gate_in : 0;
        if (blockIdx.x == 0 && threadIdx.x == 0 && gd.gate_out) *gd.gate_out = deliver_gate(result, gate_in, gd.chunk_base);
        if (g.n == 0) return;
        limit = deliver_limit(result, gate_in, gd.data_off, gd.granule, gd.bpc);
        if (limit == 0) return;
    }
    // the workgroup's range: the first whose tile_end is above this tile
    const uint32_t tile = blockIdx.x;
    uint32_t lo_r = 0, hi_r = g.n - 1;
    while (lo_r < hi_r) {
        const uint32_t mid = (lo_r + hi_r) >> 1;
        if (g.tile_end[mid] > tile) hi_r = mid;
        else lo_r = mid + 1;
    }
    const uint32_t r = lo_r;
    if (tile >= g.tile_end[r]) return;  // a grid larger than the plan
    const uint32_t ltile = tile - (r ? g.tile_end[r - 1] : 0);
    CopyRange c = g.r[r];
    if constexpr (kGuarded) {
        // a range the limit cuts ends exactly there: its last line becomes a partial one
        c.len = deliver_clip(limit, c.src_off, c.len);
        if (c.len == 0) return;
    }

    uint64_t src_b = reinterpret_cast<uint64_t>(src);
    if constexpr (kOwnSource) {
        src_b = c.src_off;
        src_len = c.len;
        c.src_off = 0;
    }
    const uint64_t src_e = src_b + src_len;  // every load below is tested against [src_b, src_e)
    auto load_quad = [&](uint64_t a) -> u32x4g {
        if constexpr (kOwnSource) return *reinterpret_cast<const HDFS3_GLOBAL u32x4g *>(a);
        // addressed through the kernel's pointer arguments, so the accesses are global, not flat
        else return *reinterpret_cast<const u32x4g *>(src + (a - src_b));
    };
    auto load_byte = [&](uint64_t a) -> uint8_t {
        if constexpr (kOwnSource) return *reinterpret_cast<const HDFS3_GLOBAL uint8_t *>(a);
        else return src[a - src_b];
    };
    const uint64_t dst_b = reinterpret_cast<uint64_t>(dst), dst_e = dst_b + dst_len;
    const uint64_t D = dst_b + c.dst_off, S = src_b + c.src_off;  // the range's first bytes
    // the range's bytes, clipped once more to the destination buffer (the planner checked them already)
    const uint64_t d_lo = D < dst_b ? dst_b : D;
    const uint64_t d_hi = D + c.len > dst_e ? dst_e : D + c.len;
    const uint64_t line0 = D & ~uint64_t(15);
    const uint64_t delta = S - D;  // source address of destination address a: a + delta
    const uint32_t k = uint32_t(delta) & 15, kj = k >> 2, kb = k & 3;

    uint64_t line[kGatherLinesPerLane];
    bool fast[kGatherLinesPerLane];
    u32x4g qlo[kGatherLinesPerLane], qhi[kGatherLinesPerLane];
#pragma unroll
    for (uint32_t i = 0; i < kGatherLinesPerLane; ++i) {
        const uint64_t idx = uint64_t(ltile) * (kGatherThreads * kGatherLinesPerLane) + i * kGatherThreads + threadIdx.x;
        line[i] = line0 + idx * 16;
        const uint64_t q = line[i] + delta - k;  // the aligned quad holding the line's first source byte
        fast[i] = line[i] >= d_lo && line[i] + 16 <= d_hi && q >= src_b && q + (k ? 32 : 16) <= src_e;
        qlo[i] = qhi[i] = u32x4g{0, 0, 0, 0};
        if (fast[i]) {
            qlo[i] = load_quad(q);
            if (k) qhi[i] = load_quad(q + 16);
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kGatherLinesPerLane; ++i) {
        if (fast[i]) {
            *reinterpret_cast<u32x4g *>(dst + (line[i] - dst_b)) = k ? shift_quads(qlo[i], qhi[i], kj, kb) : qlo[i];
            continue;
        }
        // a partial line, or a line whose quads leave the source buffer: its bytes inside the range
        const uint64_t a0 = line[i] > d_lo ? line[i] : d_lo;
        const uint64_t a1 = line[i] + 16 < d_hi ? line[i] + 16 : d_hi;
        for (uint64_t a = a0; a < a1; ++a) {
            const uint64_t s = a + delta;
            if (s >= src_b && s < src_e) dst[a - dst_b] = load_byte(s);
        }
    }
}

}  // namespace

hipError_t launch_deliver(hipStream_t stream, void *d_dst, uint64_t dst_len, const void *d_src, uint64_t src_len,
                          const GatherLaunch &g, const DeliverGuard &guard) {
    if (g.n > kGatherMaxRanges) return hipErrorInvalidValue;
    hipLaunchKernelGGL((gather_ranges_kernel<false, DeliverGuard>), dim3(g.n ? g.tile_end[g.n - 1] : 1), dim3(kGatherThreads), 0, stream,
                       static_cast<uint8_t *>(d_dst), dst_len, static_cast<const uint8_t *>(d_src), src_len, g, guard);
    return hipGetLastError();
}

hipError_t launch_gather(hipStream_t stream, void *d_dst, uint64_t dst_len, const void *d_src, uint64_t src_len,
                         const GatherLaunch &g) {
    if (g.n == 0) return hipSuccess;
    if (g.n > kGatherMaxRanges) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_ranges_kernel<false>, dim3(g.tile_end[g.n - 1]), dim3(kGatherThreads), 0, stream,
                       static_cast<uint8_t *>(d_dst), dst_len, static_cast<const uint8_t *>(d_src), src_len, g);
    return hipGetLastError();
}

hipError_t launch_gather_sources(hipStream_t stream, void *d_dst, uint64_t dst_len, const GatherLaunch &g) {
    if (g.n == 0) return hipSuccess;
    if (g.n > kGatherMaxRanges) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_ranges_kernel<true>, dim3(g.tile_end[g.n - 1]), dim3(kGatherThreads), 0, stream,
                       static_cast<uint8_t *>(d_dst), dst_len, static_cast<const uint8_t *>(nullptr), uint64_t(0), g);
    return hipGetLastError();
}

}  // namespace hdfs3crc
