// hdfs3_input_stream: InputStreamImpl's read/pread/seek over located blocks with replica
// failover (src/client/InputStreamImpl.cpp), every block read through the GPU-verifying
// hdfs3_block_reader. The C entry points keep hdfs.h's -1/errno convention (Hdfs.cpp:826-862).
//
// Block read-ahead (opt-in, hdfs3_input_set_readahead; the reference opens a block's reader
// only when the cursor reaches the block): entering block i opens the readers of blocks
// i+1 .. i+D as well, each on its own pooled GPU context and with a ring deep enough for
// max_bytes of the block, so their receiver threads read and verify ahead while block i is
// consumed. When the cursor reaches block i+1 its reader simply becomes the current one:
// read(), failover and EIO behave exactly as for a reader opened on demand.
//
// Short-circuit replicas (hdfs3_input_set_local_replicas; setupBlockReader's LocalBlockReader branch,
// :392-416): when the chosen node has a registered, still-valid local replica the block is read through
// hdfs3_local_reader instead. A local reader that cannot be opened or fails while reading invalidates
// that replica for the stream's life (info->setValid(false), :410-413) and the SAME node is read through
// the remote reader from the cursor on; the node is not failed (temporaryDisableLocalRead, :690-706).
// Stricter than the reference in one place: a forward seek skips through the local reader by reading and
// discarding, so the buffers skipped over are verified (LocalBlockReader::skip, :233-280, does not verify
// them); a bad one abandons the local replica at the seek's target.
#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <vector>

#include "../ctx.h"
#include "block_reader.h"
#include "hdfs3_client.h"
#include "hdfs3_crc.h"
#include "local_reader.h"

using namespace hdfs3crc;

namespace {

constexpr int64_t kMaxSkip = 128 * 1024;  // InputStreamImpl.cpp:1146

struct Node {
    std::string host;
    int port;
    bool operator==(const Node &o) const { return port == o.port && host == o.host; }
};

struct Block {
    std::string pool;
    hdfs3_block_id id;
    int64_t offset, length;
    std::vector<Node> replicas;
};

// a reader opened ahead of the cursor (block read-ahead) and the pooled ctx it verifies on
struct Ahead {
    int block;
    hdfs3_block_reader *reader;
    hdfs3_crc_ctx *ctx;
    Node node;
};

// a short-circuit replica the caller registered (what ReadShortCircuitInfoBuilder::fetchOrCreate returns)
struct LocalReplica {
    int block, replica;
    std::string data, meta;
    bool valid = true;  // ReadShortCircuitInfo::isValid: cleared when a local reader on it failed
};

// The stream's reader on one block: a remote block reader or a local one, never both.
struct Reader {
    hdfs3_block_reader *remote = nullptr;
    hdfs3_local_reader *local = nullptr;
    int block = -1, replica = -1;  // local: the table entry it was opened on

    explicit operator bool() const { return remote || local; }
    // into host memory, or (dev) into device memory
    int32_t read(uint8_t *buf, int32_t size, bool dev) const {
        if (local) return dev ? hdfs3_local_reader_read_dev(local, buf, size) : hdfs3_local_reader_read(local, buf, size);
        return dev ? hdfs3_block_reader_read_dev(remote, buf, size) : hdfs3_block_reader_read(remote, buf, size);
    }
    int64_t available() const {
        return local ? hdfs3_local_reader_available(local) : remote ? hdfs3_block_reader_available(remote) : 0;
    }
    // the failure is this host's GPU or memory, not the replica's
    bool host_fault() const { return local ? local_reader_host_fault(local) : block_reader_local_fault(remote); }
    void close() {
        if (remote) hdfs3_block_reader_close(remote);
        if (local) hdfs3_local_reader_close(local);
        *this = Reader();
    }
};

// hdfs.h convention: errno + -1; the message goes where hdfs3_crc_last_error reads it
int posix_fail(int err, const std::string &msg) {
    fail(-err, "%s", msg.c_str());
    errno = err;
    return -1;
}

}  // namespace

struct hdfs3_input_stream {
    std::vector<Block> blocks;
    int64_t file_length = 0;
    hdfs3_reader_opts opts{0, 1, 0, 0};
    std::string client_name;
    hdfs3_crc_ctx *ctx = nullptr;
    int64_t cursor = 0;
    int64_t end_of_cur_block = 0;
    int cur = -1;
    Reader reader;
    Node cur_node;
    std::vector<Node> failed;  // failedNodes
    uint64_t failovers = 0, opened = 0;
    std::vector<LocalReplica> local;  // hdfs3_input_set_local_replicas
    hdfs3_local_opts local_opts{0, 1, 0, 0, 0};  // buffer_size, window_buffers, flags; 0: the reader's defaults
    uint64_t local_opened = 0, local_fallbacks = 0, local_bytes = 0;
    std::string last_error;
    int ahead_blocks = 0;           // hdfs3_input_set_readahead
    int64_t ahead_bytes = 0;
    std::deque<Ahead> ahead;        // readers of blocks after `cur`, by block
    hdfs3_crc_ctx *reader_ctx = nullptr;  // the current reader's own ctx when it came from `ahead`
    uint64_t ahead_opened = 0;
    uint64_t ahead_faults = 0;      // read-ahead readers dropped on a local fault and re-read on demand

    ~hdfs3_input_stream() {
        drop_ahead(-1);
        drop_reader();
        if (ctx) ctx_release(ctx);
    }

    void drop_reader() {
        reader.close();
        if (reader_ctx) ctx_release(reader_ctx);  // after the reader: its arenas go back into it
        reader_ctx = nullptr;
    }

    // the registered local replica of block i's replica k while it is still valid
    LocalReplica *local_replica(int i, int k) {
        for (LocalReplica &l : local)
            if (l.block == i && l.replica == k) return l.valid ? &l : nullptr;
        return nullptr;
    }

    // a local reader could not be opened or failed while reading: the replica is not tried again by this
    // stream, and its node is read remotely (the table may have been replaced since the reader opened)
    void abandon_local(int i, int k) {
        if (LocalReplica *l = local_replica(i, k)) l->valid = false;
        ++local_fallbacks;
    }

    static void close_ahead(Ahead &a) {
        hdfs3_block_reader_close(a.reader);
        ctx_release(a.ctx);
    }

    // close the read-ahead readers not in (keep_from, keep_from + ahead_blocks]
    void drop_ahead(int keep_from) {
        for (auto it = ahead.begin(); it != ahead.end();) {
            if (keep_from >= 0 && it->block > keep_from && it->block <= keep_from + ahead_blocks) {
                ++it;
                continue;
            }
            close_ahead(*it);
            it = ahead.erase(it);
        }
    }

    // entering block i: its read-ahead reader (if any) becomes the current reader; readers
    // of i+1 .. i+ahead_blocks are opened where missing. A block whose reader cannot be
    // opened ahead is left to the on-demand path, which owns replica choice and failover.
    void schedule_ahead(int i) {
        for (auto it = ahead.begin(); it != ahead.end(); ++it) {
            if (it->block != i) continue;
            reader.remote = it->reader;
            reader_ctx = it->ctx;
            cur_node = it->node;
            ahead.erase(it);
            break;
        }
        drop_ahead(i);
        if (ahead_blocks <= 0) return;
        const int64_t unit = block_reader_batch_bytes(&opts);
        for (int j = i + 1; j <= i + ahead_blocks && j < int(blocks.size()); ++j) {
            auto at = std::find_if(ahead.begin(), ahead.end(), [&](const Ahead &a) { return a.block >= j; });
            if (at != ahead.end() && at->block == j) continue;
            const Block &b = blocks[size_t(j)];
            if (b.length <= 0 || b.replicas.empty()) continue;
            // a block that will be read from a local replica is not fetched over the socket as well: the
            // local reader's own loader thread reads its windows ahead
            if (local_replica(j, 0)) continue;
            const int64_t want = std::min<int64_t>(b.length, ahead_bytes > 0 ? ahead_bytes : b.length);
            // the stream's rings (ahead_blocks of them plus the current reader's) fit the pool's pinned
            // cap, so the pool can keep them for the stream's next blocks and the next stream: with
            // whole-block rings, read-ahead 7 over a 1 GiB file pinned new rings on every open
            // (2.8-3.1 GiB/s against 12.6-13.2 with an uncapped pool, profiles/r03/reentry/r3e2e_fix_*)
            // counted in the arenas' real pinned size (block_reader_arena_bytes), after the few arenas
            // every shallow pooled ctx keeps (the stream's own on-demand reader's among them)
            const int64_t arena = block_reader_arena_bytes(&opts);
            const int64_t cap = int64_t(pool_pinned_cap_bytes());
            const int64_t fit = std::max<int64_t>(0, cap - int64_t(kArenaCacheKeep) * arena) /
                                int64_t(ahead_blocks + 1) / arena;
            const int slots = int(std::max<int64_t>(3, std::min<int64_t>({(want + unit - 1) / unit + 1, 64, fit})));
            hdfs3_crc_ctx *c = nullptr;
            if (ctx_acquire(opts.device, &c, true)) break;  // no context to spare: read on demand
            hdfs3_block_id id = b.id;
            id.pool_id = b.pool.c_str();
            hdfs3_block_reader *r = nullptr;
            const Node &n = b.replicas.front();  // choseBestNode with a fresh failed list
            if (open_block_reader(n.host.c_str(), n.port, &id, 0, b.length, client_name.c_str(), &opts, c, &r,
                                  slots)) {
                ctx_release(c);
                continue;
            }
            ++ahead_opened;
            ahead.insert(at, Ahead{j, r, c, n});
        }
    }

    int find_block(int64_t pos) const {  // LocatedBlocks::findBlock
        auto it = std::upper_bound(blocks.begin(), blocks.end(), pos,
                                   [](int64_t p, const Block &b) { return p < b.offset; });
        if (it == blocks.begin()) return -1;
        const int i = int(it - blocks.begin()) - 1;
        return pos < blocks[i].offset + blocks[i].length ? i : -1;
    }

    // choseBestNode (InputStreamImpl.cpp:322-335): first replica not yet failed
    const Node *best_node(const Block &b) const {
        for (const Node &n : b.replicas)
            if (std::find(failed.begin(), failed.end(), n) == failed.end()) return &n;
        return nullptr;
    }

    // setupBlockReader (:364-450) for [start, start+len) of block b; -errno
    int setup(const Block &b, int64_t start, int64_t len, Reader *out, Node *node, uint8_t *dest = nullptr) {
        std::string why;
        const int bi = int(&b - blocks.data());
        for (;;) {
            const Node *n = best_node(b);
            if (!n) {
                last_error = "InputStreamImpl: all nodes have been tried and no valid replica can be read for Block: " +
                             std::to_string(b.id.block_id) + (why.empty() ? "" : " (last: " + why + ")");
                return -EIO;
            }
            const int k = int(n - b.replicas.data());
            if (const LocalReplica *l = local_replica(bi, k)) {
                hdfs3_local_opts lo = local_opts;
                lo.device = opts.device;
                lo.verify = opts.verify;
                LocalOpenExtra extra;
                extra.range_end = start + len;
                extra.replica = true;
                const int rc = open_local_reader(l->data.c_str(), l->meta.c_str(), b.length, start, &lo, &extra, &out->local);
                if (rc == 0) {
                    out->block = bi;
                    out->replica = k;
                    *node = *n;
                    ++local_opened;
                    return 0;
                }
                // this host's GPU or memory: neither the replica's fault nor the node's
                if (extra.host_fault || rc == -ENOMEM || rc == -ENODEV || rc == -ENOTSUP) {
                    last_error = hdfs3_crc_last_error();
                    return rc;
                }
                // the same node again, through the remote reader; it does not go on the failed list
                why = hdfs3_crc_last_error();
                abandon_local(bi, k);
                continue;
            }
            hdfs3_block_id id = b.id;
            id.pool_id = b.pool.c_str();
            const int rc = open_block_reader(n->host.c_str(), n->port, &id, start, len, client_name.c_str(), &opts,
                                             ctx, &out->remote, 0, dest);
            if (rc == 0) {
                *node = *n;
                ++opened;
                return 0;
            }
            if (rc == -ENOTSUP || rc == -ENOMEM || rc == -ENODEV) {  // not a replica problem: another node cannot help
                last_error = hdfs3_crc_last_error();
                return rc;
            }
            why = hdfs3_crc_last_error();
            failed.push_back(*n);
        }
    }

    void seek_to_block(int i) {  // seekToBlock: new block, fresh failed list
        drop_reader();
        cur = i;
        end_of_cur_block = blocks[i].offset + blocks[i].length;
        failed.clear();
        // a read-ahead reader starts at the block's first byte: usable on sequential entry
        if ((ahead_blocks > 0 || !ahead.empty()) && cursor == blocks[i].offset) schedule_ahead(i);
        else if (!ahead.empty()) drop_ahead(i);
    }

    // readOneBlock (:616-712); dev: buf is device memory (the readers' read_dev)
    int32_t read_one_block(uint8_t *buf, int32_t size, bool dev) {
        const Block &b = blocks[cur];
        for (;;) {
            if (!reader) {
                const int64_t off = cursor - b.offset;
                if (int rc = setup(b, off, b.length - off, &reader, &cur_node)) return rc;
            }
            const int32_t todo = int32_t(std::min<int64_t>(size, end_of_cur_block - cursor));
            const int32_t n = reader.read(buf, todo, dev);
            if (n > 0) {
                cursor += n;
                if (reader.local) local_bytes += uint64_t(n);
                return n;
            }
            // a destination that is not this device's memory is the caller's mistake, not the replica's
            if (dev && n == -EINVAL) {
                last_error = hdfs3_crc_last_error();
                return n;
            }
            // a local GPU/memory fault is not the replica's: report it, do not burn the replicas.
            // A read-ahead reader faults on its own pooled ctx and deep ring, which an on-demand
            // reader does not need: that block is read again on demand from the cursor on the
            // stream's ctx, and only a fault there is reported (same bytes and errors as with
            // read-ahead off)
            if (reader.host_fault()) {
                last_error = hdfs3_crc_last_error();
                const bool prefetched = reader_ctx != nullptr;
                drop_reader();
                if (prefetched) {
                    ++ahead_faults;
                    continue;
                }
                return n < 0 ? n : -EIO;
            }
            // a local reader's ChecksumException or file error (:690-706): what it returned before stays
            // delivered; the same node is read remotely from the cursor on, and is not failed
            if (reader.local) {
                abandon_local(reader.block, reader.replica);
                drop_reader();
                continue;
            }
            // ChecksumException or I/O failure: this replica is bad, try another (:682-708)
            ++failovers;
            failed.push_back(cur_node);
            drop_reader();
        }
    }

    int32_t read(uint8_t *buf, int32_t size, bool dev = false) {
        if (cursor >= file_length) return 0;  // HdfsEndOfStream -> hdfsRead returns 0
        if (cursor >= end_of_cur_block || cur < 0) {
            const int i = find_block(cursor);
            if (i < 0) return -EIO;
            seek_to_block(i);
        }
        return read_one_block(buf, size, dev);
    }

    // fetchBlockByteRange (:955-1061): the whole range from one replica, else the next
    // dev: `out` is device memory: no eager destination goes to the reader (its receiver would memcpy
    // into a device pointer), and a replica that fails is read again from `out` on, as on the host
    int fetch_range(const Block &b, int64_t start, int64_t len, uint8_t *out, bool dev) {
        std::vector<Node> saved;
        saved.swap(failed);
        int rc = 0;
        for (;;) {
            Reader r;
            Node node;
            // the range's one destination goes to the reader, which copies each packet there while it is hot
            // (round 6; 8 concurrent preads: client CPU per GiB 1.28-1.41x -> 0.98-1.16x the reference
            // loop's, rate within the spread, profiles/r06/r6eg_config5_eager_ab.jsonl).
            // HDFS3_READER_EAGER_COPY=0 (measurement knob) leaves the copy to read()
            const char *ev = getenv("HDFS3_READER_EAGER_COPY");
            const bool eager = !dev && !(ev && ev[0] == '0');
            if ((rc = setup(b, start, len, &r, &node, eager ? out : nullptr))) break;
            int64_t got = 0;
            int32_t n = 0;
            while (got < len) {
                n = r.read(out + got, int32_t(std::min<int64_t>(len - got, 1 << 30)), dev);
                if (n <= 0) break;
                got += n;
            }
            const bool local = r.host_fault();
            if (local) last_error = hdfs3_crc_last_error();
            const bool short_circuit = r.local != nullptr;
            const int lb = r.block, lk = r.replica;
            r.close();
            if (got == len) {
                if (short_circuit) local_bytes += uint64_t(len);
                break;
            }
            if (local || (dev && n == -EINVAL)) {  // this host's GPU or the caller's pointer, not the replica: no failover
                if (!local) last_error = hdfs3_crc_last_error();
                rc = n < 0 ? n : -EIO;
                break;
            }
            if (short_circuit) {  // the range again from its first byte, from the same node's remote reader
                abandon_local(lb, lk);
                continue;
            }
            ++failovers;
            failed.push_back(node);
        }
        failed.swap(saved);
        return rc;
    }

    int32_t pread(int64_t pos, uint8_t *buf, int32_t size, bool dev = false) {
        if (pos < 0 || pos >= file_length) return -EINVAL;
        const int32_t real = int32_t(std::min<int64_t>(size, file_length - pos));
        int64_t done = 0;
        while (done < real) {
            const int i = find_block(pos + done);
            if (i < 0) return -EIO;
            const Block &b = blocks[i];
            const int64_t start = pos + done - b.offset;
            const int64_t n = std::min<int64_t>(real - done, b.length - start);
            if (int rc = fetch_range(b, start, n, buf + done, dev)) return rc;
            done += n;
        }
        return real;
    }

    int seek(int64_t pos) {  // seekInternal (:1133-1170)
        if (pos == cursor) return 0;
        if (pos > file_length) return -EOVERFLOW;
        if (reader && pos > cursor && pos < end_of_cur_block && pos - cursor <= kMaxSkip) {
            uint8_t scratch[16384];
            bool ok = true;
            while (cursor < pos) {
                const int32_t n = reader.read(scratch, int32_t(std::min<int64_t>(sizeof(scratch), pos - cursor)), false);
                if (n <= 0) {
                    ok = false;
                    break;
                }
                cursor += n;
            }
            if (ok) return 0;
            // a local reader met a bad buffer (or a file error) on the way: the replica is abandoned, and the
            // read at the target opens the same node's remote reader
            if (reader.local && !reader.host_fault()) abandon_local(reader.block, reader.replica);
        }
        drop_reader();
        end_of_cur_block = 0;
        cursor = pos;
        return 0;
    }
};

extern "C" {

int hdfs3_input_open(const hdfs3_located_block *blocks, int n_blocks, const char *client_name,
                     const hdfs3_reader_opts *opts, hdfs3_input_stream **out) {
    if (!out || n_blocks < 0 || (n_blocks && !blocks)) return fail(-EINVAL, "invalid argument");
    *out = nullptr;
    hdfs3_input_stream *s = new (std::nothrow) hdfs3_input_stream();
    if (!s) return fail(-ENOMEM, "input stream allocation");
    if (opts) s->opts = *opts;
    s->client_name = client_name ? client_name : "libhdfs3_amd";
    int64_t expect = n_blocks ? blocks[0].offset : 0;
    for (int i = 0; i < n_blocks; ++i) {
        const hdfs3_located_block &lb = blocks[i];
        if (lb.offset != expect || int64_t(lb.block.num_bytes) < 0 || lb.n_replicas < 0 ||
            (lb.n_replicas && !lb.replicas)) {
            delete s;
            return fail(-EINVAL, "located block %d is not contiguous with its predecessor or malformed", i);
        }
        Block b;
        b.pool = lb.block.pool_id ? lb.block.pool_id : "";
        b.id = lb.block;
        b.id.pool_id = nullptr;
        b.offset = lb.offset;
        b.length = int64_t(lb.block.num_bytes);
        for (int k = 0; k < lb.n_replicas; ++k) {
            if (!lb.replicas[k].host) {
                delete s;
                return fail(-EINVAL, "replica %d of block %d has no host", k, i);
            }
            b.replicas.push_back(Node{lb.replicas[k].host, lb.replicas[k].port});
        }
        expect += b.length;
        s->blocks.push_back(std::move(b));
    }
    if (n_blocks && blocks[0].offset != 0) {
        delete s;
        return fail(-EINVAL, "the first block must start at file offset 0");
    }
    s->file_length = expect;
    if (int rc = ctx_acquire(s->opts.device, &s->ctx)) {
        delete s;
        return rc;
    }
    *out = s;
    return 0;
}

int32_t hdfs3_input_read(hdfs3_input_stream *s, void *buf, int32_t len) {
    if (!s || !buf || len <= 0) return posix_fail(EINVAL, "hdfsRead: invalid argument");
    s->last_error.clear();
    const int32_t rc = s->read(static_cast<uint8_t *>(buf), len);
    if (rc < 0) return posix_fail(-rc, s->last_error.empty() ? hdfs3_crc_last_error() : s->last_error);
    return rc;
}

int32_t hdfs3_input_pread(hdfs3_input_stream *s, int64_t pos, void *buf, int32_t len) {
    if (!s || !buf || len <= 0 || pos < 0) return posix_fail(EINVAL, "hdfsPread: invalid argument");
    s->last_error.clear();
    const int32_t rc = s->pread(pos, static_cast<uint8_t *>(buf), len);
    if (rc == -EINVAL) return posix_fail(EINVAL, "hdfsPread: position outside the file");
    if (rc < 0) return posix_fail(-rc, s->last_error.empty() ? hdfs3_crc_last_error() : s->last_error);
    return rc;
}

int32_t hdfs3_input_read_dev(hdfs3_input_stream *s, void *d_buf, int32_t len) {
    if (!s || !d_buf || len <= 0) return posix_fail(EINVAL, "hdfs3_input_read_dev: invalid argument");
    s->last_error.clear();
    const int32_t rc = s->read(static_cast<uint8_t *>(d_buf), len, true);
    if (rc < 0) return posix_fail(-rc, s->last_error.empty() ? hdfs3_crc_last_error() : s->last_error);
    return rc;
}

int32_t hdfs3_input_pread_dev(hdfs3_input_stream *s, int64_t pos, void *d_buf, int32_t len) {
    if (!s || !d_buf || len <= 0 || pos < 0) return posix_fail(EINVAL, "hdfs3_input_pread_dev: invalid argument");
    if (pos >= s->file_length) return posix_fail(EINVAL, "hdfs3_input_pread_dev: position outside the file");
    s->last_error.clear();
    const int32_t rc = s->pread(pos, static_cast<uint8_t *>(d_buf), len, true);
    if (rc < 0) return posix_fail(-rc, s->last_error.empty() ? hdfs3_crc_last_error() : s->last_error);
    return rc;
}

int hdfs3_input_seek(hdfs3_input_stream *s, int64_t pos) {
    if (!s || pos < 0) return posix_fail(EINVAL, "hdfsSeek: invalid argument");
    if (int rc = s->seek(pos))
        return posix_fail(-rc, "InputStreamImpl: seek over EOF, seek target: " + std::to_string(pos));
    return 0;
}

int64_t hdfs3_input_tell(hdfs3_input_stream *s) {
    if (!s) return posix_fail(EINVAL, "hdfsTell: invalid argument");
    return s->cursor;
}

int hdfs3_input_available(hdfs3_input_stream *s) {
    if (!s) return posix_fail(EINVAL, "hdfsAvailable: invalid argument");
    const int64_t a = s->reader.available();
    return int(std::min<int64_t>(a, 0x7FFFFFFF));
}

int64_t hdfs3_input_length(hdfs3_input_stream *s) { return s ? s->file_length : -1; }

int hdfs3_input_stats(hdfs3_input_stream *s, uint64_t *failovers, uint64_t *readers_opened) {
    if (!s) return fail(-EINVAL, "null stream");
    if (failovers) *failovers = s->failovers;
    if (readers_opened) *readers_opened = s->opened;
    return 0;
}

int hdfs3_input_set_local_replicas(hdfs3_input_stream *s, const hdfs3_local_replica *local, int n,
                                   const hdfs3_local_opts *lopts) {
    if (!s || n < 0 || (n && !local)) return fail(-EINVAL, "invalid argument");
    if (int rc = local_opts_check(lopts)) return rc;
    std::vector<LocalReplica> table;
    for (int i = 0; i < n; ++i) {
        const hdfs3_local_replica &l = local[i];
        if (l.block < 0 || l.block >= int(s->blocks.size()) || l.replica < 0 ||
            l.replica >= int(s->blocks[size_t(l.block)].replicas.size()))
            return fail(-EINVAL, "local replica %d names block %d replica %d, which the stream does not have", i, l.block,
                        l.replica);
        if (!l.data_path || !l.meta_path) return fail(-EINVAL, "local replica %d has no data or meta path", i);
        for (const LocalReplica &t : table)
            if (t.block == l.block && t.replica == l.replica)
                return fail(-EINVAL, "block %d replica %d is named twice", l.block, l.replica);
        table.push_back(LocalReplica{l.block, l.replica, l.data_path, l.meta_path});
    }
    s->local.swap(table);
    s->local_opts = hdfs3_local_opts{0, 1, 0, 0, 0};
    if (lopts) {
        s->local_opts.buffer_size = lopts->buffer_size;
        s->local_opts.window_buffers = lopts->window_buffers;
        s->local_opts.flags = lopts->flags;
    }
    return 0;
}

int hdfs3_input_local_stats(hdfs3_input_stream *s, uint64_t *local_readers_opened, uint64_t *local_fallbacks,
                            uint64_t *local_bytes) {
    if (!s) return fail(-EINVAL, "null stream");
    if (local_readers_opened) *local_readers_opened = s->local_opened;
    if (local_fallbacks) *local_fallbacks = s->local_fallbacks;
    if (local_bytes) *local_bytes = s->local_bytes;
    return 0;
}

int hdfs3_input_set_readahead(hdfs3_input_stream *s, int blocks, int64_t max_bytes_per_block) {
    if (!s || blocks < 0 || max_bytes_per_block < 0) return fail(-EINVAL, "invalid argument");
    // every block opened ahead holds a pooled ctx, a connection and a pinned ring at once
    if (blocks > HDFS3_READAHEAD_MAX_BLOCKS)
        return fail(-EINVAL, "read-ahead of %d blocks: at most %d", blocks, HDFS3_READAHEAD_MAX_BLOCKS);
    s->ahead_blocks = blocks;
    s->ahead_bytes = max_bytes_per_block;
    if (blocks == 0) s->drop_ahead(-1);
    return 0;
}

int hdfs3_input_readahead_stats(hdfs3_input_stream *s, uint64_t *prefetch_readers_opened,
                                uint64_t *prefetch_local_faults) {
    if (!s) return fail(-EINVAL, "null stream");
    if (prefetch_readers_opened) *prefetch_readers_opened = s->ahead_opened;
    if (prefetch_local_faults) *prefetch_local_faults = s->ahead_faults;
    return 0;
}

int hdfs3_input_close(hdfs3_input_stream *s) {
    delete s;
    return 0;
}

}  // extern "C"
