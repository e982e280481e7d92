// Launch planning (launch_plan.h): host arithmetic only.
#include "launch_plan.h"

namespace hdfs3crc {

static uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }
// what the wave kernels' loads need: 16-byte aligned data, 4-byte aligned words
static bool wave_aligned(uintptr_t data, uintptr_t crc) { return ((data & 15u) | (crc & 3u)) == 0; }

bool packet_geom(uint64_t data_len, uint64_t last_len, uint64_t npk, uint32_t unit_bpc, PacketGeom *g) {
    if (npk == 0 || unit_bpc == 0 || unit_bpc > uint32_t(kRoundBytes) || last_len > data_len) return false;
    if (npk > 1 && (data_len == 0 || data_len % unit_bpc)) return false;  // only the last packet ends short
    PacketGeom r;
    const uint64_t lw = last_len / unit_bpc * unit_bpc;
    r.lunits = uint32_t((lw + kRoundBytes - 1) / kRoundBytes);
    r.ltail = r.lunits ? uint32_t(lw - uint64_t(r.lunits - 1) * kRoundBytes) : 0;
    if (npk > 1) {
        r.pk_len = data_len;
        r.upp = uint32_t((data_len + kRoundBytes - 1) / kRoundBytes);
        r.ptail = uint32_t(data_len - uint64_t(r.upp - 1) * kRoundBytes);
    } else {
        // one packet is its own last packet: with upp = lunits every unit u < lunits is round u of
        // packet 0 (u / upp = 0), whatever data_len and the pitch are
        r.pk_len = 0;
        r.upp = r.lunits;
        r.ptail = r.ltail;
    }
    const uint64_t units = (npk - 1) * uint64_t(r.upp) + r.lunits;
    if (units == 0 || units >= (uint64_t(1) << 31)) return false;
    // q = (u * magic) >> shift = u / upp for every u < 2^31: magic = ceil(2^(31 + l) / upp), l =
    // ceil(log2 upp), so magic < 2^32 and u * magic < 2^63
    uint32_t l = 0;
    while ((uint64_t(1) << l) < r.upp) ++l;
    r.shift = 31 + l;
    r.magic = uint32_t(((uint64_t(1) << r.shift) + r.upp - 1) / r.upp);
    *g = r;
    return true;
}

bool packet_stream_ok(uint64_t data_len, uint64_t last_len, uint64_t npk, uint32_t bpc, const void *data,
                      const void *crc, uint64_t pitch, PacketGeom *geom) {
    // bpc 512..4096: the round kernel's pitch walk, a packet's last round partial when its chunks
    // end inside one (round 6); R * 4096 (R >= 2): the walk's 4096-byte piece CRCs + the combine
    // (launch_stream_pieces, round 4), every packet but the last whole chunks
    const bool pieces = pieces_bpc(bpc);
    if (!round_bpc(bpc) && !pieces) return false;
    if (npk == 0 || data_len == 0 || last_len > data_len) return false;
    if (npk > 1 && pitch == 0) return false;
    if (npk >= (uint64_t(1) << 31)) return false;  // keys are (packet << 32) | chunk
    if (!wave_aligned(addr(data), addr(crc)) || (pitch & 15u)) return false;
    if (pieces && npk > 1 && data_len % bpc) return false;
    return packet_geom(data_len, last_len, npk, pieces ? uint32_t(kRoundBytes) : bpc, geom);
}

bool plan_packet_stream(uint64_t data_len, uint64_t last_len, uint64_t npk, uint32_t bpc, const void *data,
                        const void *crc, uint64_t pitch, bool have_pieces, int variant, PitchStream *s) {
    if (variant == 52 || variant == 53 || (pieces_bpc(bpc) && !have_pieces)) return false;
    if (!packet_stream_ok(data_len, last_len, npk, bpc, data, crc, pitch, &s->geom)) return false;
    s->pitch = pitch;
    s->crc_pitch = 0;
    s->npk = npk;
    s->last_len = uint32_t(last_len);
    return true;
}

bool plan_strided_blocks(const DevSegment *h_seg, size_t n, uint32_t bpc, int variant, PitchStream *s) {
    if (variant == 54 || n < 2) return false;
    const int64_t dp = int64_t(addr(h_seg[1].data) - addr(h_seg[0].data));
    const int64_t cp = int64_t(addr(h_seg[1].crc) - addr(h_seg[0].crc));
    if (dp <= 0 || cp <= 0 || (cp & 3)) return false;
    for (size_t i = 0; i < n; ++i)
        if (addr(h_seg[i].data) != addr(h_seg[0].data) + i * uint64_t(dp) ||
            addr(h_seg[i].crc) != addr(h_seg[0].crc) + i * uint64_t(cp) ||
            (i + 1 < n && h_seg[i].len != h_seg[0].len) || h_seg[i].len > h_seg[0].len)
            return false;
    // no piece scratch: blocks at bpc = R x 4096 stay with the segmented path's per-block launches
    if (!plan_packet_stream(h_seg[0].len, h_seg[n - 1].len, n, bpc, h_seg[0].data, h_seg[0].crc, uint64_t(dp), false,
                            variant, s))
        return false;
    s->crc_pitch = uint64_t(cp);
    return true;
}

uint64_t plan_segments(DevSegment *h_seg, size_t n, uint32_t bpc, uint64_t *uniform) {
    uint64_t units = 0, u0 = n ? seg_units(h_seg[0].len, bpc) : 0;
    bool same = true;
    for (size_t i = 0; i < n; ++i) {
        h_seg[i].unit_begin = units;
        const uint64_t u = seg_units(h_seg[i].len, bpc);
        if (i + 1 < n && u != u0) same = false;
        units += u;
    }
    *uniform = same && u0 > 0 ? u0 : 0;
    return units;
}

bool segments_fast(const DevSegment *h_seg, size_t n, uint32_t bpc) {
    if (!round_bpc(bpc)) return false;
    for (size_t i = 0; i < n; ++i)
        if (!wave_aligned(addr(h_seg[i].data), addr(h_seg[i].crc))) return false;
    return true;
}

BatchPlan plan_packet_batch(uint64_t arena, const DevPacket *h_pk, size_t n, uint32_t bpc, const uint64_t *arena_len,
                            bool have_pieces, int variant, DevSegment *h_stage) {
    BatchPlan p;
    // one pass: bounds, the alignment test of segments_fast, the unit plan of plan_segments and the
    // two constant-pitch detectors
    bool fast = variant != 17 && round_bpc(bpc);
    // bpc = R * 4096: the pitch walk's pieces + combine when the batch is a constant-pitch stream
    const bool pieces = variant != 17 && have_pieces && pieces_bpc(bpc);
    bool aligned = fast || pieces;
    const uint32_t ubpc = bpc <= uint32_t(kRoundBytes) ? bpc : uint32_t(kRoundBytes);
    uint64_t units = 0, u0 = seg_units(h_pk[0].data_len, ubpc);
    bool same = true;
    // constant pitch: packet i at data_off[0] + i*S, crc_off[0] + i*S, one data length
    // (the last may be shorter) -> the kernel derives every descriptor (SegLaunch::stride)
    const uint64_t pitch = n > 1 ? h_pk[1].data_off - h_pk[0].data_off : 0;
    bool strided = n > 1 && variant != 52 && pitch > 0 && pitch == h_pk[1].crc_off - h_pk[0].crc_off;
    // the same with the words at a pitch of their own (round 5: the output stream's batches, whose
    // words are dense at 4 x chunks per packet while the data sits in packet slots): the pitch walk
    // with ChunkLaunch::crc_pitch, so writer packets of whole rounds (bpc 1024 ... 65536: 64 KiB of
    // data) take the round kernel, and at bpc = R x 4096 its pieces + combine, instead of the
    // descriptor-array segmented kernel or (above 4 KiB) the chunk-per-lane packet kernel
    const uint64_t cpitch = n > 1 ? h_pk[1].crc_off - h_pk[0].crc_off : 0;
    bool dstrided = n > 1 && variant != 52 && pitch > 0 && h_pk[1].crc_off > h_pk[0].crc_off && (cpitch & 3) == 0;
    for (size_t i = 0; i < n; ++i) {
        const DevPacket &d = h_pk[i];
        if (arena_len) {  // bounds, fused into this pass (the API's only pass over pk[])
            const uint64_t chunks = (uint64_t(d.data_len) + bpc - 1) / bpc;
            if (d.data_off > *arena_len || d.data_len > *arena_len - d.data_off || d.crc_off > *arena_len ||
                4 * chunks > *arena_len - d.crc_off) {
                p.route = Route::kOutOfBounds;
                p.bad_index = i;
                return p;
            }
        }
        const uint64_t u = seg_units(d.data_len, ubpc);
        const bool al = wave_aligned(uintptr_t(arena + d.data_off), uintptr_t(arena + d.crc_off));
        fast = fast && al;
        aligned = aligned && al;
        if (i + 1 < n && u != u0) same = false;
        const bool row = d.data_off == h_pk[0].data_off + i * pitch && (i + 1 == n || d.data_len == h_pk[0].data_len);
        strided = strided && row && d.crc_off == h_pk[0].crc_off + i * pitch;
        dstrided = dstrided && row && d.crc_off == h_pk[0].crc_off + i * cpitch;
        units += u;
    }
    const auto at = [&](uint64_t off) { return reinterpret_cast<uint8_t *>(uintptr_t(arena + off)); };
    if (aligned && (strided || dstrided) &&
        plan_packet_stream(h_pk[0].data_len, h_pk[n - 1].data_len, n, bpc, at(h_pk[0].data_off), at(h_pk[0].crc_off),
                           pitch, have_pieces, variant, &p.stream)) {
        p.stream.crc_pitch = strided ? 0 : cpitch;
        p.route = Route::kPitchStream;
        return p;
    }
    p.units = units;
    p.uniform = same && u0 > 0 ? u0 : 0;
    if (fast && strided && p.uniform && n > kInlineSegments) {
        p.stream.pitch = pitch;
        p.route = Route::kStridedSegments;
        return p;
    }
    if (!fast && !(aligned && n < (size_t(1) << 31))) {
        // variant 17 (A/B) or unaligned / other chunk sizes: one wave per packet
        DevPacket *hp = reinterpret_cast<DevPacket *>(h_stage);
        for (size_t i = 0; i < n; ++i) hp[i] = h_pk[i];
        p.route = Route::kPackets;
        return p;
    }
    units = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t len = h_pk[i].data_len;
        h_stage[i] = DevSegment{at(h_pk[i].data_off), at(h_pk[i].crc_off), len, units, uint64_t(i) << 32};
        units += seg_units(len, ubpc);
        if (!fast) {
            const uint64_t nf = len / bpc;
            p.max_chunks = nf > p.max_chunks ? nf : p.max_chunks;
            p.any_tail = p.any_tail || (len % bpc) != 0;
        }
    }
    if (!fast) {
        // bpc = R x 4096, aligned, not one constant-pitch stream: piece CRCs over the segment list + the
        // combine (round 6; the chunk-per-lane packet kernel before, ~1 TiB/s); a unit is a piece here
        p.pieces_total = units;
        p.route = Route::kSegmentPieces;
    } else if (n <= kInlineSegments) {
        p.route = Route::kInlineSegments;  // no descriptor copy in front of the kernel
    } else if (!p.uniform && n > kUnitMapMinSegments && have_pieces && units) {
        // a long ragged list: the unit -> segment map in the piece scratch (4 B per 4 KiB unit)
        // instead of a binary search per round; 1 GiB of 32-64 KiB packets at bpc 512: 313.6 ->
        // 219.7 us verify (profiles/r06/r6za_partial_rate.jsonl, r6zb_partial_rate.jsonl)
        p.route = Route::kMappedSegments;
    } else {
        p.route = Route::kStagedSegments;
    }
    return p;
}

size_t gather_first_bad(const CopyRange *in, size_t n, uint64_t src_len, uint64_t dst_len) {
    for (size_t i = 0; i < n; ++i) {
        const CopyRange &c = in[i];
        if (c.src_off > src_len || c.len > src_len - c.src_off) return i;
        if (c.dst_off > dst_len || c.len > dst_len - c.dst_off) return i;
        if (c.len > (kGatherMaxTiles - 1) * kGatherTileBytes) return i;  // whatever the destination's alignment
    }
    return n;
}

size_t gather_sources_first_bad(const CopyRange *in, size_t n, uint64_t dst_len) {
    // the address space as the one source buffer: a range inside it does not wrap
    return gather_first_bad(in, n, ~uint64_t(0), dst_len);
}

size_t plan_gather_launch(uint64_t dst_addr, const CopyRange *in, size_t n, size_t pos, GatherLaunch *g) {
    g->n = 0;
    uint64_t tiles = 0;  // of the ranges before the last one
    for (; pos < n; ++pos) {
        const CopyRange &c = in[pos];
        if (c.len == 0) continue;
        if (g->n) {
            CopyRange &p = g->r[g->n - 1];
            const uint64_t merged = gather_tiles(dst_addr + p.dst_off, p.len + c.len);
            if (p.src_off + p.len == c.src_off && p.dst_off + p.len == c.dst_off && tiles + merged <= kGatherMaxTiles) {
                p.len += c.len;
                g->tile_end[g->n - 1] = uint32_t(tiles + merged);
                continue;
            }
            tiles = g->tile_end[g->n - 1];
        }
        const uint64_t t = gather_tiles(dst_addr + c.dst_off, c.len);
        if (g->n == kGatherMaxRanges || tiles + t > kGatherMaxTiles) break;
        g->r[g->n] = c;
        g->tile_end[g->n] = uint32_t(tiles + t);
        ++g->n;
    }
    return pos;
}

}  // namespace hdfs3crc
