// The block reader's batch geometry: where each packet of a batch lands in its arena, when a batch
// closes, how a verify result maps back to a packet, how delivery walks the packets, how large an arena
// is. Plain host arithmetic: no GPU runtime, no arena allocation (tests/native/reader_layout_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../launch_plan.h"

namespace hdfs3crc {

// A batch arena's room per packet: the datanode's default 64 KiB packet, its 128 words at bpc 512 and
// the 16-byte alignment of its data (larger packets close a batch early; one that does not fit an
// empty arena grows it). Round 4: 80 KiB before, so a 64-packet arena pinned 5 MiB for 4.03 MiB of
// packets and a read-ahead stream's rings overran the pool's pinned cap by a ring (config 5)
constexpr size_t kPacketGuess = 64 * 1024 + 512 + 16;
// bytes of a ring arena, payload of a batch of 64 KiB datanode packets, and what one batch pins: the
// arena, its descriptor staging and the result word
constexpr size_t ring_arena_bytes(int batch_packets) { return size_t(batch_packets) * kPacketGuess; }
constexpr int64_t batch_payload_bytes(int batch_packets) { return int64_t(batch_packets) * 64 * 1024; }
constexpr int64_t arena_pinned_bytes(int batch_packets) {
    return int64_t(batch_packets) * int64_t(kPacketGuess + sizeof(DevSegment)) + int64_t(sizeof(unsigned long long));
}

// Chunk sizes the contiguous kernels take (launch_chunks); others keep the wire layout
constexpr bool dense_bpc(uint32_t bpc) { return round_bpc(bpc) || pieces_bpc(bpc); }

struct PacketRef {
    uint64_t data_off, crc_off;  // inside the arena
    uint32_t data_len;
    uint32_t skip;               // pendingAhead (RemoteBlockReader.cpp:264-266)
    uint32_t deliver;            // bytes of this packet inside [start, end)
};

// place()'s answer: close the batch (the packet's header opens the next), or the arena offsets of the
// packet's words and data and the capacity they need (above the arena's only for a batch's first packet)
struct Placement { bool close; uint64_t crc_off, data_off, crc_len, need; };

// Wire layout: [words][data] of each packet as on the socket, the data 16-byte aligned.
// Dense layout (round 5): the socket's [words][data] of each packet land in two places, the words
// after the batch's earlier words from offset 0, the data after its earlier data from d0. While every
// packet but the last holds whole chunks, the batch is then ONE contiguous block with its own
// .meta-style word array, and the GPU verifies it with the contiguous round kernel: no packet pitch,
// no 4 KiB rounds straddling packets. Same bytes on the wire, same delivery (PacketRef), same
// ChecksumException semantics.
struct BatchLayout {
    bool dense = false, sealed = false;
    uint32_t chunk_size = 0;
    uint64_t d0 = 0, words_used = 0, data_used = 0, used = 0;
    std::vector<PacketRef> pk;
    std::vector<uint64_t> chunk0;  // dense: packet i's first chunk in the batch

    void reset() {
        dense = sealed = false;
        d0 = words_used = data_used = used = 0;
        pk.clear();
        chunk0.clear();
    }

    // Before an empty batch's first packet (of data_len bytes). Dense: room for batch_packets packets'
    // words, sized for the largest packet expected (a datanode's 64 KiB, or this one if larger): a short
    // first packet must not shrink the word region and close the batch after a few packets
    void open(uint32_t data_len, uint32_t bpc, uint32_t checksum_size, int batch_packets, bool dense_layout) {
        dense = dense_layout;
        chunk_size = bpc;
        if (!dense) return;
        const uint64_t exp_data = std::max<uint64_t>(data_len, uint64_t(64) << 10);
        const uint64_t max_crc = (exp_data + bpc - 1) / bpc * checksum_size;
        d0 = (uint64_t(batch_packets) * max_crc + 4095) & ~uint64_t(4095);
    }

    // The arena as acquired holds a dense batch (64 KiB packets: 32 KiB of words + 4 MiB of data in the
    // 64 x 66,064 B the ring is sized for); larger packets close the batch early, as in the wire
    // layout, and only a single packet that does not fit an empty batch grows the arena
    Placement place(uint32_t data_len, uint64_t crc_len, uint64_t cap) const {
        if (dense) {
            const uint64_t need = d0 + data_used + data_len;
            const bool close = !pk.empty() && (sealed || words_used + crc_len > d0 || need > cap);
            return Placement{close, words_used, d0 + data_used, crc_len, need};
        }
        const uint64_t off = ((used + crc_len + 15) & ~uint64_t(15)) - crc_len, size = crc_len + data_len;
        const bool fits = off + size <= cap;
        return Placement{!fits && !pk.empty(), off, off + crc_len, crc_len, fits ? off + size : size + 64};
    }

    // The packet was received where place() said
    void commit(const Placement &p, uint32_t data_len, uint32_t ahead, uint32_t useful) {
        pk.push_back(PacketRef{p.data_off, p.crc_off, data_len, ahead, useful});
        used = p.data_off + data_len;
        if (!dense) return;
        chunk0.push_back(words_used / 4);
        words_used += p.crc_len;
        data_used += data_len;
        if (data_len % chunk_size) sealed = true;  // a short chunk ends the contiguous chunk run
    }

    // A non-zero verify result word -> the batch's first bad packet
    int64_t bad_packet(unsigned long long r) const {
        if (!dense) {
            int64_t pkt = -1;
            split_result_key(r, &pkt, nullptr);
            return pkt;
        }
        const uint64_t chunk = ~r;  // the first bad chunk of the batch
        return int64_t(std::upper_bound(chunk0.begin(), chunk0.end(), chunk) - chunk0.begin()) - 1;
    }
};

// Where delivery stands in a batch: packet and offset into its deliverable bytes
struct DeliveryCursor {
    size_t pkt = 0, off = 0;
    struct Piece { uint64_t src; size_t n; };  // arena offset, bytes

    bool done(size_t limit) const { return pkt >= limit; }
    // the next piece, at most n bytes of one packet; the caller stops at done(limit)
    Piece take(const std::vector<PacketRef> &pk, size_t n) {
        const PacketRef &p = pk[pkt];
        const Piece piece{p.data_off + p.skip + off, std::min<size_t>(p.deliver - off, n)};
        off += piece.n;
        if (off == p.deliver) {
            ++pkt;
            off = 0;
        }
        return piece;
    }
    // bytes the takes up to `limit` will deliver
    int64_t remaining(const std::vector<PacketRef> &pk, size_t limit) const {
        int64_t a = 0;
        for (size_t i = pkt; i < limit; ++i) a += pk[i].deliver - (i == pkt ? off : 0);
        return a;
    }
};

}  // namespace hdfs3crc
