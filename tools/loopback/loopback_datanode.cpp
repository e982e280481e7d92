// TEST / BENCH INFRASTRUCTURE — a loopback "datanode" serving in-memory blocks over the
// HDFS data-transfer protocol, so the GPU block reader can be exercised end to end
// without a cluster (the reference has no in-process datanode either: SURVEY.md §4).
// Server side of the exchange the reference client drives in RemoteBlockReader.cpp:
//   request  BE16 version | u8 op | varint len | OpReadBlockProto
//   response varint len | BlockOpResponseProto {SUCCESS, ChecksumProto, chunkOffset}
//   packets  [31 B PacketHeader][chunks x BE32 CRC][data] ..., then an empty last packet
//   status   varint len | ClientReadStatusProto (CHECKSUM_OK / SUCCESS) from the client
// CRC words are served as given (the caller computes them; corrupt ones for negative
// tests). Data and CRC buffers are referenced, not copied.
//
// Write side (the datanode end of PipelineImpl, src/client/Pipeline.cpp): OP_WRITE_BLOCK
// with targets forwards the request to the next node and answers with that node's outcome
// (firstBadLink on failure), then receives packets, mirrors each downstream, verifies the
// CRC words when it is the last node of the pipeline (as HDFS's BlockReceiver does), stores
// the block and acks every packet with PipelineAckProto{seqno, [own status] + downstream
// statuses} from a responder thread. After the last packet's ack the block is readable
// through OP_READ_BLOCK. PIPELINE_SETUP_APPEND continues a replica this node holds (length and
// stamp checked; the appended block takes the new generation stamp; a packet completing a partial
// chunk gets that chunk's stored word recomputed over the whole chunk). Fault injection: refuse the
// setup, an error status or a dropped connection at a seqno, bytes corrupted in transit at a seqno.
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <vector>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <sys/uio.h>
#include <thread>
#include <unistd.h>

#include "../../include/hdfs3_client.h"
#include "../../libhdfs3_amd/csrc/client/net.h"
#include "../../libhdfs3_amd/csrc/client/wire.h"
#include "../../libhdfs3_amd/csrc/md5.h"

using namespace hdfs3crc;

namespace {

struct Stored {                     // a block received through OP_WRITE_BLOCK
    std::vector<uint8_t> data, crc_be;
};

struct Block {
    const uint8_t *data;
    uint64_t len;
    const uint8_t *crc_be;  // ceil(len/bpc) words
    uint32_t bpc;
    int type;
    std::shared_ptr<Stored> keep;  // owner of data/crc_be for written blocks
    uint64_t gs = 0;               // generation stamp (0: not tracked, as for blocks added to serve)
};

enum WriteFault : int { kNoFault = 0, kRefuseSetup = 1, kAckError = 2, kCorruptInTransit = 3, kDropAt = 4 };

// the datanode's own CRC32C (SSE4.2 crc32q, the engine HDFS datanodes use on x86), used to
// verify received packets; independent of the GPU path under test
struct SwCrc32c {
    __attribute__((target("sse4.2"))) uint32_t operator()(const uint8_t *p, size_t n) const {
        uint64_t c = 0xFFFFFFFFu;
        while (n >= 8) {
            uint64_t w;
            std::memcpy(&w, p, 8);
            c = __builtin_ia32_crc32di(c, w);
            p += 8;
            n -= 8;
        }
        uint32_t c32 = uint32_t(c);
        while (n--) c32 = __builtin_ia32_crc32qi(c32, *p++);
        return ~c32;
    }
};
const SwCrc32c g_crc;

// one loopback datanode, identified by its port; several run side by side to act as the
// replicas of a block (InputStreamImpl failover)
struct Server {
    int listen_fd = -1;
    std::atomic<bool> stop{false};
    std::mutex mu;
    std::map<uint64_t, Block> blocks;
    std::atomic<int> packet_bytes{64 * 1024};
    std::atomic<int64_t> fail_after{-1};  // drop the connection after this many data bytes
    std::atomic<uint64_t> served{0};
    std::atomic<uint64_t> requests{0};
    std::atomic<int> last_status{-1};
    std::atomic<int> active{0};
    std::thread accept;
    // write side
    std::atomic<int> write_fault{kNoFault};
    std::atomic<int64_t> fault_seqno{-1};
    std::atomic<bool> store_written{true};  // false: verify + ack only (rate measurements)
    std::atomic<uint64_t> write_packets{0}, write_bytes{0}, checksum_errors{0}, blocks_finalized{0};
};

std::mutex g_mu;
std::map<int, Server *> g_servers;

Server *find(int port) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_servers.find(port);
    return it == g_servers.end() ? nullptr : it->second;
}

int send_all_iov(int fd, iovec *iov, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += iov[i].iov_len;
    while (total) {
        msghdr m{};
        m.msg_iov = iov;
        m.msg_iovlen = size_t(n);
        // MSG_NOSIGNAL: a client that stops early (ChecksumException) must not SIGPIPE the host
        ssize_t w = sendmsg(fd, &m, MSG_NOSIGNAL);
        if (w < 0) {
            if (errno == EINTR || errno == EAGAIN) continue;
            return -errno;
        }
        total -= size_t(w);
        while (n && size_t(w) >= iov->iov_len) {
            w -= ssize_t(iov->iov_len);
            ++iov;
            --n;
        }
        if (n) {
            iov->iov_base = static_cast<char *>(iov->iov_base) + w;
            iov->iov_len -= size_t(w);
        }
    }
    return 0;
}

// OP_BLOCK_CHECKSUM: the datanode's answer is the MD5 of the block's stored CRC words
// (the .meta file after its header), with bytesPerCrc and crcPerBlock beside it
void serve_block_checksum(Server *sv, int fd, const std::string &proto, int version, int to) {
    wire::ExtendedBlock eb;
    wire::BlockOpResponse resp;
    Block b{};
    bool found = false;
    const bool ok = version == wire::kDataTransferVersion && wire::decode_block_checksum(proto.data(), proto.size(), eb);
    if (ok) {
        std::lock_guard<std::mutex> lk(sv->mu);
        auto it = sv->blocks.find(eb.block_id);
        if (it != sv->blocks.end()) b = it->second, found = true;
    }
    if (!ok || !found || b.type == wire::kChecksumNull) {
        resp.status = wire::kErrorInvalid;
        resp.message = !ok ? "bad request" : !found ? "block not found" : "block has no checksums";
    } else {
        const uint64_t n = (b.len + b.bpc - 1) / b.bpc;
        Md5 md5;
        md5.update(b.crc_be, size_t(n) * 4);
        uint8_t d[16];
        md5.finish(d);
        resp.status = wire::kSuccess;
        resp.has_checksum_response = true;
        resp.checksum_response.bytes_per_crc = b.bpc;
        resp.checksum_response.crc_per_block = n;
        resp.checksum_response.md5.assign(reinterpret_cast<const char *>(d), 16);
        resp.checksum_response.crc_type = b.type;
    }
    (void)net::write_delimited(fd, wire::encode_block_op_response(resp), to);
    net::close_fd(fd);
}

int own_port(Server *sv) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto &kv : g_servers)
        if (kv.second == sv) return kv.first;
    return 0;
}

// one entry per received packet, acked in order by the responder
struct AckItem {
    int64_t seqno;
    int status;
    bool last;
    bool drop;   // injected: close the connection instead of acking
};

// OP_WRITE_BLOCK: BlockReceiver + PacketResponder of one datanode of the pipeline
void serve_write(Server *sv, int fd, const std::string &proto, int version, int to) {
    wire::WriteBlockRequest req;
    wire::BlockOpResponse resp;
    const std::string self = "127.0.0.1:" + std::to_string(own_port(sv));
    if (version != wire::kDataTransferVersion || !wire::decode_write_block(proto.data(), proto.size(), req) ||
        req.bytes_per_checksum == 0) {
        resp.status = wire::kErrorInvalid;
        resp.message = "bad write request";
        (void)net::write_delimited(fd, wire::encode_block_op_response(resp), to);
        net::close_fd(fd);
        return;
    }
    if (sv->write_fault == kRefuseSetup) {
        resp.status = wire::kError;
        resp.first_bad_link = self;
        (void)net::write_delimited(fd, wire::encode_block_op_response(resp), to);
        net::close_fd(fd);
        return;
    }
    // PIPELINE_SETUP_APPEND: this node must hold the replica at the client's length and stamp; the
    // block continues from its bytes and takes the new generation stamp (BlockReceiver append)
    std::shared_ptr<Stored> base;
    if (req.stage == wire::kPipelineSetupAppend) {
        Block b{};
        bool found = false;
        {
            std::lock_guard<std::mutex> lk(sv->mu);
            auto it = sv->blocks.find(req.block.block_id);
            if (it != sv->blocks.end()) b = it->second, found = true;
        }
        const char *why = !found ? "replica not found"
                          : b.len != req.min_bytes_rcvd || b.len != req.block.num_bytes ? "replica length mismatch"
                          : b.gs && b.gs != req.block.generation_stamp ? "replica generation stamp mismatch"
                          : req.latest_generation_stamp <= req.block.generation_stamp ? "stale new generation stamp"
                          : b.bpc != req.bytes_per_checksum ? "bytes per checksum mismatch"
                                                            : nullptr;
        if (why) {
            resp.status = wire::kErrorInvalid;
            resp.message = why;
            resp.first_bad_link = self;
            (void)net::write_delimited(fd, wire::encode_block_op_response(resp), to);
            net::close_fd(fd);
            return;
        }
        base = std::make_shared<Stored>();
        base->data.assign(b.data, b.data + b.len);
        base->crc_be.assign(b.crc_be, b.crc_be + 4 * ((b.len + b.bpc - 1) / b.bpc));
    }
    int down = -1;  // mirror to the next node of the pipeline
    if (!req.targets.empty()) {
        const wire::DatanodeAddr next = req.targets[0];
        wire::WriteBlockRequest fwd = req;
        fwd.targets.erase(fwd.targets.begin());
        fwd.pipeline_size = uint32_t(fwd.targets.size());
        down = net::connect_tcp(next.ip_addr.c_str(), int(next.xfer_port), to);
        std::string rb;
        wire::BlockOpResponse dresp;
        const std::string msg = wire::encode_write_block(fwd);
        if (down < 0 || net::write_fully(down, msg.data(), msg.size(), to) ||
            net::read_delimited(down, rb, 1 << 20, to) || !wire::decode_block_op_response(rb.data(), rb.size(), dresp) ||
            dresp.status != wire::kSuccess) {
            resp.status = wire::kError;
            resp.first_bad_link = dresp.first_bad_link.empty() ? next.ip_addr + ":" + std::to_string(next.xfer_port)
                                                               : dresp.first_bad_link;
            (void)net::write_delimited(fd, wire::encode_block_op_response(resp), to);
            net::close_fd(down);
            net::close_fd(fd);
            return;
        }
    }
    resp.status = wire::kSuccess;
    if (net::write_delimited(fd, wire::encode_block_op_response(resp), to)) {
        net::close_fd(down);
        net::close_fd(fd);
        return;
    }
    const uint32_t bpc = req.bytes_per_checksum;
    const bool verify = down < 0 && req.checksum_type == wire::kChecksumCrc32c;  // the last node verifies
    auto stored = base ? base : std::make_shared<Stored>();
    const uint64_t final_gs = base ? req.latest_generation_stamp : req.block.generation_stamp;

    std::mutex qmu;
    std::condition_variable qcv;
    std::deque<AckItem> q;
    bool closing = false;
    std::atomic<bool> broken{false};
    std::thread responder([&] {
        for (;;) {
            AckItem it;
            {
                std::unique_lock<std::mutex> lk(qmu);
                qcv.wait(lk, [&] { return !q.empty() || closing; });
                if (q.empty()) return;
                it = q.front();
                q.pop_front();
            }
            if (it.drop) {
                broken = true;
                shutdown(fd, SHUT_RDWR);
                return;
            }
            wire::PipelineAck ack;
            ack.seqno = it.seqno;
            ack.status.push_back(it.status);
            if (down >= 0) {  // wait for the downstream ack of the same packet
                std::string ab;
                wire::PipelineAck dack;
                if (net::read_delimited(down, ab, 1 << 16, to) || !wire::decode_pipeline_ack(ab.data(), ab.size(), dack) ||
                    dack.seqno != it.seqno) {
                    ack.status.push_back(wire::kError);
                } else {
                    ack.status.insert(ack.status.end(), dack.status.begin(), dack.status.end());
                }
            }
            if (net::write_delimited(fd, wire::encode_pipeline_ack(ack), to)) {
                broken = true;
                return;
            }
            if (it.last && ack.success() && sv->store_written) {  // finalize: the block becomes readable
                std::lock_guard<std::mutex> lk(sv->mu);
                const uint64_t len = stored->data.size();
                sv->blocks[req.block.block_id] =
                    Block{stored->data.data(), len, stored->crc_be.data(), bpc, req.checksum_type, stored, final_gs};
                ++sv->blocks_finalized;
            }
            if (it.last) return;
        }
    });

    std::vector<uint8_t> pkt;
    for (;;) {
        uint8_t pre[6];
        if (broken || net::read_fully(fd, pre, 6, to)) break;
        const int32_t packet_len = int32_t(wire::rd_be32(pre));
        const int hdr_len = wire::rd_be16(pre + 4);
        if (packet_len < 4 || packet_len > (64 << 20) || hdr_len > 1024) break;
        pkt.resize(6 + size_t(hdr_len) + size_t(packet_len) - 4);
        std::memcpy(pkt.data(), pre, 6);
        if (net::read_fully(fd, pkt.data() + 6, pkt.size() - 6, to)) break;
        wire::PacketHeader h;
        if (!h.decode(pkt.data(), pkt.size())) break;
        const uint64_t chunks = (uint64_t(h.data_len) + bpc - 1) / bpc;
        if (h.data_len < 0 || uint64_t(packet_len) != 4 + uint64_t(h.data_len) + 4 * chunks) break;
        const int64_t fault_at = sv->fault_seqno.load();
        const int fault = fault_at == h.seqno ? sv->write_fault.load() : kNoFault;
        if (fault == kCorruptInTransit && h.data_len > 0) pkt[pkt.size() - 1] ^= 0x40;  // last data byte
        if (down >= 0 && net::write_fully(down, pkt.data(), pkt.size(), to)) {
            std::lock_guard<std::mutex> lk(qmu);
            q.push_back(AckItem{h.seqno, wire::kError, h.last_packet_in_block, false});
            qcv.notify_one();
            break;
        }
        const uint8_t *sums = pkt.data() + 6 + hdr_len;
        const uint8_t *data = sums + 4 * chunks;
        int status = wire::kSuccess;
        if (verify)
            for (uint64_t c = 0; c < chunks; ++c) {
                const uint64_t off = c * bpc;
                const size_t n = size_t(std::min<uint64_t>(bpc, uint64_t(h.data_len) - off));
                if (g_crc(data + off, n) != wire::rd_be32(sums + 4 * c)) {
                    status = wire::kErrorChecksum;
                    ++sv->checksum_errors;
                    break;
                }
            }
        if (fault == kAckError) status = wire::kError;
        if (status == wire::kSuccess && h.data_len > 0 && sv->store_written) {
            // a re-sent partial chunk (after hflush) overwrites from offsetInBlock
            const uint64_t off = uint64_t(h.offset_in_block);
            if (off > stored->data.size() || (off % bpc && !base)) {
                status = wire::kErrorInvalid;
            } else if (off % bpc == 0) {
                stored->data.resize(off);
                stored->crc_be.resize(off / bpc * 4);
                stored->data.insert(stored->data.end(), data, data + h.data_len);
                stored->crc_be.insert(stored->crc_be.end(), sums, sums + 4 * chunks);
            } else {
                // appended bytes that complete a partial chunk: the packet's words cover the new
                // bytes only, so the stored word of every chunk touched is recomputed over the
                // whole chunk (the datanode's partial-chunk checksum handling)
                stored->data.resize(off);
                stored->data.insert(stored->data.end(), data, data + h.data_len);
                const uint64_t c0 = off / bpc, n = stored->data.size();
                stored->crc_be.resize(c0 * 4);
                for (uint64_t c = c0; c * bpc < n; ++c) {
                    const uint32_t w = g_crc(stored->data.data() + c * bpc, size_t(std::min<uint64_t>(bpc, n - c * bpc)));
                    const uint8_t be[4] = {uint8_t(w >> 24), uint8_t(w >> 16), uint8_t(w >> 8), uint8_t(w)};
                    stored->crc_be.insert(stored->crc_be.end(), be, be + 4);
                }
            }
        }
        ++sv->write_packets;
        sv->write_bytes += uint64_t(h.data_len);
        {
            std::lock_guard<std::mutex> lk(qmu);
            q.push_back(AckItem{h.seqno, status, h.last_packet_in_block, fault == kDropAt});
            qcv.notify_one();
        }
        if (fault == kDropAt || h.last_packet_in_block) break;
    }
    {
        std::lock_guard<std::mutex> lk(qmu);
        closing = true;
        qcv.notify_one();
    }
    responder.join();
    net::close_fd(down);
    net::close_fd(fd);
}

void serve(Server *sv, int fd) {
    const int to = 60000;
    uint8_t head[3];
    std::string proto;
    wire::ReadBlockRequest req;
    if (net::read_fully(fd, head, 3, to) || net::read_delimited(fd, proto, 1 << 20, to)) {
        net::close_fd(fd);
        return;
    }
    if (head[2] == wire::kOpBlockChecksum) {
        ++sv->requests;
        serve_block_checksum(sv, fd, proto, (head[0] << 8) | head[1], to);
        return;
    }
    if (head[2] == wire::kOpWriteBlock) {
        ++sv->requests;
        serve_write(sv, fd, proto, (head[0] << 8) | head[1], to);
        return;
    }
    if (!wire::decode_read_block(proto.data(), proto.size(), req)) {
        net::close_fd(fd);
        return;
    }
    ++sv->requests;
    wire::BlockOpResponse resp;
    Block b{};
    bool found = false;
    {
        std::lock_guard<std::mutex> lk(sv->mu);
        auto it = sv->blocks.find(req.block.block_id);
        if (it != sv->blocks.end()) b = it->second, found = true;
    }
    const int version = (head[0] << 8) | head[1];
    if (version != wire::kDataTransferVersion || head[2] != wire::kOpReadBlock || !found ||
        req.offset > b.len) {
        resp.status = wire::kErrorInvalid;
        resp.message = found ? "bad request" : "block not found";
        net::write_delimited(fd, wire::encode_block_op_response(resp), to);
        net::close_fd(fd);
        return;
    }
    const uint64_t first = req.offset - req.offset % b.bpc;  // reads align back to a chunk
    uint64_t end = req.offset + req.len;
    if (end > b.len) end = b.len;
    resp.status = wire::kSuccess;
    resp.has_checksum_info = true;
    resp.checksum_type = b.type;
    resp.bytes_per_checksum = b.bpc;
    resp.chunk_offset = first;
    if (net::write_delimited(fd, wire::encode_block_op_response(resp), to)) {
        net::close_fd(fd);
        return;
    }
    const uint64_t per = std::max<uint64_t>(b.bpc, uint64_t(sv->packet_bytes.load()) / b.bpc * b.bpc);
    const uint32_t csize = b.type == wire::kChecksumNull ? 0 : 4;
    const int64_t fail_after = sv->fail_after.load();
    uint64_t sent = 0;
    int64_t seq = 0;
    for (uint64_t pos = first; pos < end; pos += per) {
        uint64_t n = end - pos < per ? end - pos : per;
        n = std::min<uint64_t>(((n + b.bpc - 1) / b.bpc) * b.bpc, b.len - pos);  // whole chunks
        const uint64_t chunks = (n + b.bpc - 1) / b.bpc;
        if (fail_after >= 0 && sent + n > uint64_t(fail_after)) {  // injected datanode failure
            net::close_fd(fd);
            return;
        }
        wire::PacketHeader h;
        h.packet_len = int32_t(4 + n + chunks * csize);
        h.offset_in_block = int64_t(pos);
        h.seqno = seq++;
        h.last_packet_in_block = false;
        h.data_len = int32_t(n);
        uint8_t hb[wire::kPacketHeaderSize];
        h.encode(hb);
        iovec iov[3] = {{hb, sizeof(hb)},
                        {const_cast<uint8_t *>(b.crc_be + 4 * (pos / b.bpc)), size_t(chunks * csize)},
                        {const_cast<uint8_t *>(b.data + pos), size_t(n)}};
        if (send_all_iov(fd, iov, 3)) {
            net::close_fd(fd);
            return;
        }
        sv->served += n;
        sent += n;
        if (pos + n >= end) break;
    }
    wire::PacketHeader last;
    last.packet_len = 4;
    last.offset_in_block = int64_t(end);
    last.seqno = seq;
    last.last_packet_in_block = true;
    last.data_len = 0;
    uint8_t lb[wire::kPacketHeaderSize];
    last.encode(lb);
    if (net::write_fully(fd, lb, sizeof(lb), to) == 0) {
        std::string st;
        int status = -1;
        if (net::read_delimited(fd, st, 1024, 10000) == 0 &&
            wire::decode_client_read_status(st.data(), st.size(), status))
            sv->last_status = status;
    }
    net::close_fd(fd);
}

void accept_loop(Server *sv) {
    while (!sv->stop) {
        const int fd = accept(sv->listen_fd, nullptr, nullptr);
        if (fd < 0) {
            if (sv->stop) return;
            continue;
        }
        const int one = 1;  // acks are small writes: no Nagle delay behind the previous one
        setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
        ++sv->active;
        std::thread([sv, fd] {
            serve(sv, fd);
            --sv->active;
        }).detach();
    }
}

}  // namespace

extern "C" {

/* start a datanode on 127.0.0.1 (ephemeral port); the port identifies it afterwards */
int hdfs3_loopback_start(int *port) {
    int p = 0;
    const int fd = net::listen_tcp(0, &p);
    if (fd < 0) return fd;
    Server *sv = new Server();
    sv->listen_fd = fd;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_servers[p] = sv;
    }
    sv->accept = std::thread(accept_loop, sv);
    if (port) *port = p;
    return 0;
}

/* serve block_id from (data, crc_be); the buffers are referenced, not copied */
int hdfs3_loopback_add_block(int port, uint64_t block_id, const void *data, uint64_t len, const void *crc_be,
                             uint32_t bpc, int checksum_type) {
    Server *sv = find(port);
    if (!sv || !bpc) return -EINVAL;
    std::lock_guard<std::mutex> lk(sv->mu);
    sv->blocks[block_id] = Block{static_cast<const uint8_t *>(data), len, static_cast<const uint8_t *>(crc_be), bpc,
                                 checksum_type, nullptr};
    return 0;
}

int hdfs3_loopback_clear_blocks(int port) {
    Server *sv = find(port);
    if (!sv) return -EINVAL;
    std::lock_guard<std::mutex> lk(sv->mu);
    sv->blocks.clear();
    return 0;
}

int hdfs3_loopback_set_packet_bytes(int port, int n) {
    Server *sv = find(port);
    if (!sv) return -EINVAL;
    sv->packet_bytes = n > 0 ? n : 64 * 1024;
    return 0;
}

/* drop every later connection after `bytes` data bytes (-1: never) */
int hdfs3_loopback_set_fail_after(int port, int64_t bytes) {
    Server *sv = find(port);
    if (!sv) return -EINVAL;
    sv->fail_after = bytes;
    return 0;
}

uint64_t hdfs3_loopback_served_bytes(int port) {
    Server *sv = find(port);
    return sv ? sv->served.load() : 0;
}

uint64_t hdfs3_loopback_requests(int port) {
    Server *sv = find(port);
    return sv ? sv->requests.load() : 0;
}

int hdfs3_loopback_last_status(int port) {
    Server *sv = find(port);
    return sv ? sv->last_status.load() : -1;
}

/* Test/bench packet sink for hdfs3_output_open: counts packets and bytes into
 * user = uint64_t[3] {packets, wire bytes, data bytes} and touches every byte (a stand-in
 * for the socket write of PipelineImpl::send). */
int hdfs3_loopback_count_sink(void *user, const void *pkt, size_t len, const void *info) {
    (void)info;
    uint64_t *c = static_cast<uint64_t *>(user);
    const uint8_t *p = static_cast<const uint8_t *>(pkt);
    uint64_t x = 0;
    for (size_t i = 0; i < len; i += 64) x += p[i];
    c[0] += 1;
    c[1] += len;
    c[2] += x & 1;  // keeps the loop
    return 0;
}

/* Test/bench packet sink that checks what it is handed: user = uint64_t[6] {address of the source bytes,
 * position in them, packets, wire bytes, packets whose data differ from the source at the position,
 * their first seqno + 1}. Every packet's data region is compared whole (tools/write_dev_ab.py). */
int hdfs3_loopback_compare_sink(void *user, const void *pkt, size_t len, const hdfs3_packet_info *info) {
    uint64_t *c = static_cast<uint64_t *>(user);
    const uint8_t *src = reinterpret_cast<const uint8_t *>(uintptr_t(c[0]));
    const size_t head = size_t(wire::kPacketHeaderSize) + 4u * size_t(info->num_chunks);
    const bool ok = len == head + size_t(info->data_len) &&
                    std::memcmp(static_cast<const uint8_t *>(pkt) + head, src + c[1], size_t(info->data_len)) == 0;
    c[1] += uint64_t(info->data_len);
    c[2] += 1;
    c[3] += len;
    if (!ok && !c[4]++) c[5] = uint64_t(info->seqno) + 1;
    return 0;
}

/* write-side fault injection: mode 0 none, 1 refuse the pipeline setup (ERROR +
 * firstBadLink = this node), 2 error status in the ack of `seqno`, 3 flip a data bit of
 * packet `seqno` on arrival (the last node's verify then reports ERROR_CHECKSUM),
 * 4 drop the connection instead of acking `seqno` */
int hdfs3_loopback_set_write_fault(int port, int mode, int64_t seqno) {
    Server *sv = find(port);
    if (!sv) return -EINVAL;
    sv->fault_seqno = seqno;
    sv->write_fault = mode;
    return 0;
}

/* keep written blocks (default) or only verify and ack them: fresh-memory page faults of
 * the in-memory store, not the client, bound a write-rate measurement otherwise */
int hdfs3_loopback_set_store_written(int port, int store) {
    Server *sv = find(port);
    if (!sv) return -EINVAL;
    sv->store_written = store != 0;
    return 0;
}

/* packets and data bytes received by OP_WRITE_BLOCK, chunks that failed verification,
 * blocks finalized */
int hdfs3_loopback_write_stats(int port, uint64_t *packets, uint64_t *bytes, uint64_t *checksum_errors,
                               uint64_t *finalized) {
    Server *sv = find(port);
    if (!sv) return -EINVAL;
    if (packets) *packets = sv->write_packets;
    if (bytes) *bytes = sv->write_bytes;
    if (checksum_errors) *checksum_errors = sv->checksum_errors;
    if (finalized) *finalized = sv->blocks_finalized;
    return 0;
}

/* a block this node holds (served or written): pointers stay valid until the block is
 * replaced or the node stops. 0, or -ENOENT */
int hdfs3_loopback_get_block(int port, uint64_t block_id, const void **data, uint64_t *len, const void **crc_be,
                             uint32_t *bpc) {
    Server *sv = find(port);
    if (!sv) return -EINVAL;
    std::lock_guard<std::mutex> lk(sv->mu);
    auto it = sv->blocks.find(block_id);
    if (it == sv->blocks.end()) return -ENOENT;
    if (data) *data = it->second.data;
    if (len) *len = it->second.len;
    if (crc_be) *crc_be = it->second.crc_be;
    if (bpc) *bpc = it->second.bpc;
    return 0;
}

/* the generation stamp a written block was finalized with (0 for blocks added to serve) */
int hdfs3_loopback_block_gs(int port, uint64_t block_id, uint64_t *gs) {
    Server *sv = find(port);
    if (!sv || !gs) return -EINVAL;
    std::lock_guard<std::mutex> lk(sv->mu);
    auto it = sv->blocks.find(block_id);
    if (it == sv->blocks.end()) return -ENOENT;
    *gs = it->second.gs;
    return 0;
}

int hdfs3_loopback_stop(int port) {
    Server *sv = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_servers.find(port);
        if (it == g_servers.end()) return -EINVAL;
        sv = it->second;
        g_servers.erase(it);
    }
    sv->stop = true;
    shutdown(sv->listen_fd, SHUT_RDWR);
    net::close_fd(sv->listen_fd);
    if (sv->accept.joinable()) sv->accept.join();
    // connection threads reference the server; wait for them before freeing it
    for (int i = 0; i < 6000 && sv->active.load() > 0; ++i) usleep(10000);
    if (sv->active.load() == 0) delete sv;  // else leak rather than free under a live thread
    return 0;
}

}  // extern "C"
