// hdfs.h file-I/O surface (include/hdfs3_hdfs.h) over hdfs3_input_* / hdfs3_output_*.
//
// Mirrors src/client/Hdfs.cpp function by function: the PARAMETER_ASSERT checks and their
// errno (Hdfs.cpp:75-80), hdfsRead/hdfsPread returning 0 at end of file and -1 + errno on
// error (:826-862), hdfsWrite returning `length` (:864-881), hdfsFlush = hdfsHFlush
// (:883-904), a thread-local last-error string initialised to "Success" (:59, :329).
// Host code only: the GPU work happens inside the streams.
#include "hdfs3_hdfs.h"

#include "hdfs3_crc.h"

#include <cerrno>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

namespace {

thread_local char g_msg[4096] = "Success";

void set_msg(const char *m) {
    std::strncpy(g_msg, m ? m : "", sizeof(g_msg) - 1);
    g_msg[sizeof(g_msg) - 1] = 0;
}

// PARAMETER_ASSERT (Hdfs.cpp:75-80): message = strerror(eno), errno = eno
#define PARAMETER_ASSERT(para, retval, eno) \
    if (!(para)) {                          \
        set_msg(std::strerror(eno));        \
        errno = eno;                        \
        return retval;                      \
    }

// a failed stream call already set errno; keep its message for hdfsGetLastError
template <typename T>
T stream_failed(T rv) {
    const int e = errno;
    set_msg(hdfs3_crc_last_error());
    errno = e;
    return rv;
}

// a deep copy of a LocatedBlocks table: the caller's strings and replica tables may go away
struct BlockTable {
    std::vector<hdfs3_located_block> blocks;
    std::vector<std::vector<hdfs3_datanode>> replicas;
    std::vector<std::string> strings;  // pool ids and host names the tables point into

    bool assign(const hdfs3_located_block *b, int n) {
        blocks.assign(b, b + n);
        replicas.assign(size_t(n), {});
        strings.clear();
        size_t nstr = 0;
        for (int i = 0; i < n; ++i) nstr += 1 + size_t(b[i].n_replicas > 0 ? b[i].n_replicas : 0);
        strings.reserve(nstr);  // no reallocation: the c_str() pointers below stay valid
        for (int i = 0; i < n; ++i) {
            if (b[i].n_replicas < 0 || (b[i].n_replicas > 0 && !b[i].replicas)) return false;
            strings.emplace_back(b[i].block.pool_id ? b[i].block.pool_id : "");
            blocks[size_t(i)].block.pool_id = strings.back().c_str();
            for (int k = 0; k < b[i].n_replicas; ++k) {
                if (!b[i].replicas[k].host) return false;
                strings.emplace_back(b[i].replicas[k].host);
                replicas[size_t(i)].push_back(hdfs3_datanode{strings.back().c_str(), b[i].replicas[k].port});
            }
            blocks[size_t(i)].replicas = replicas[size_t(i)].data();
        }
        return true;
    }
    BlockTable() = default;
    BlockTable(const BlockTable &o) { assign(o.blocks.data(), int(o.blocks.size())); }
    BlockTable &operator=(const BlockTable &o) {
        if (this != &o) assign(o.blocks.data(), int(o.blocks.size()));
        return *this;
    }
};

// hdfs3_fs_add_local_replica: a replica of one of the file's blocks that is on this machine
struct LocalFiles {
    int block, replica;
    std::string data, meta;
};

struct FileEntry {
    BlockTable located_blocks;
    bool located = false;  // registered by hdfs3_fs_add_file (a file of 0 blocks is empty)
    std::vector<LocalFiles> local;  // dropped whenever located_blocks is replaced
    hdfs3_packet_sink sink = nullptr;
    void *user = nullptr;
    BlockTable pipeline_blocks;  // hdfs3_fs_set_pipeline: the blocks addBlock would allocate
    bool pipeline = false;
    uint64_t append_gs = 0;      // hdfs3_fs_set_append_stamp (0: the last block's stamp + 1)
    // FileStatus::getBlockSize (hdfs3_fs_set_block_size, or the size a write through this table used;
    // 0: unknown, then a file of two or more blocks states it by its first block)
    int64_t block_size = 0;
};

}  // namespace

struct HdfsFileSystemInternalWrapper {
    std::string client_name;
    hdfs3_reader_opts ropts{0, 1, 64, 0};
    hdfs3_writer_opts wopts{0, 512, 65536, int64_t(128) << 20, 64};
    int readahead_blocks = 0;         // hdfs3_fs_set_readahead: for files opened for reading
    int64_t readahead_bytes = 0;
    bool local_read = true;           // hdfs3_fs_set_local_read (dfs.client.read.shortcircuit)
    hdfs3_local_opts lopts{0, 1, 0, 0, 0};  // buffer_size, window_buffers, flags of the local readers
    std::mutex mu;
    std::map<std::string, FileEntry> files;
};

struct HdfsFileInternalWrapper {
    bool input = true;
    hdfs3_input_stream *in = nullptr;
    hdfs3_output_stream *out = nullptr;
    hdfs3_pipeline *pipe = nullptr;  // writes through datanodes (hdfs3_fs_set_pipeline)
    BlockTable written;              // the pipeline's blocks, for completeFile
    BlockTable prefix;               // append: the file's blocks before the pipeline's first one
    std::string path;
    int64_t block_size = 0;          // the write's block size (the file's, for FileStatus)
    // the size is the file's own: a create, a size registered for the path, or one a file of two or
    // more blocks states; an append to a one-block file of unknown size only guessed it,
    // and a guess is not recorded as the file's block size
    bool block_size_known = false;
};

extern "C" {

const char *hdfsGetLastError() { return g_msg; }

int hdfsFileIsOpenForRead(hdfsFile file) {
    PARAMETER_ASSERT(file, 0, EINVAL);
    return file->input ? 1 : 0;
}

int hdfsFileIsOpenForWrite(hdfsFile file) {
    PARAMETER_ASSERT(file, 0, EINVAL);
    return !file->input ? 1 : 0;
}

hdfsFS hdfs3_fs_new(const char *client_name, const hdfs3_reader_opts *read_opts,
                    const hdfs3_writer_opts *write_opts) {
    hdfsFS fs = new (std::nothrow) HdfsFileSystemInternalWrapper();
    if (!fs) {
        set_msg("Out of memory");
        errno = ENOMEM;
        return nullptr;
    }
    fs->client_name = client_name && *client_name ? client_name : "libhdfs3_amd";
    if (read_opts) fs->ropts = *read_opts;
    if (write_opts) fs->wopts = *write_opts;
    return fs;
}

int hdfs3_fs_add_file(hdfsFS fs, const char *path, const hdfs3_located_block *blocks, int n_blocks) {
    PARAMETER_ASSERT(fs && path && std::strlen(path) > 0 && n_blocks >= 0 && (n_blocks == 0 || blocks), -1,
                     EINVAL);
    BlockTable t;
    PARAMETER_ASSERT(t.assign(blocks, n_blocks), -1, EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    FileEntry &slot = fs->files[path];
    slot.located_blocks = t;
    slot.located = true;
    slot.local.clear();
    return 0;
}

int hdfs3_fs_add_local_replica(hdfsFS fs, const char *path, int block, int replica, const char *data_path,
                               const char *meta_path) {
    PARAMETER_ASSERT(fs && path && std::strlen(path) > 0, -1, EINVAL);
    PARAMETER_ASSERT(data_path && std::strlen(data_path) > 0 && meta_path && std::strlen(meta_path) > 0, -1, EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    auto it = fs->files.find(path);
    PARAMETER_ASSERT(it != fs->files.end() && it->second.located, -1, ENOENT);
    FileEntry &e = it->second;
    const auto &lbs = e.located_blocks.blocks;
    PARAMETER_ASSERT(block >= 0 && size_t(block) < lbs.size() && replica >= 0 &&
                         replica < lbs[size_t(block)].n_replicas,
                     -1, EINVAL);
    for (const LocalFiles &l : e.local) PARAMETER_ASSERT(l.block != block || l.replica != replica, -1, EINVAL);
    e.local.push_back(LocalFiles{block, replica, data_path, meta_path});
    return 0;
}

int hdfs3_fs_set_local_read(hdfsFS fs, int on, const hdfs3_local_opts *lopts) {
    PARAMETER_ASSERT(fs, -1, EINVAL);
    PARAMETER_ASSERT(!lopts || (!(lopts->flags & ~HDFS3_LOCAL_CRC32_AS_ZLIB) && lopts->buffer_size <= (1 << 30)), -1,
                     EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    fs->local_read = on != 0;
    fs->lopts = lopts ? *lopts : hdfs3_local_opts{0, 1, 0, 0, 0};
    return 0;
}

int hdfs3_fs_set_pipeline(hdfsFS fs, const char *path, const hdfs3_located_block *blocks, int n_blocks) {
    PARAMETER_ASSERT(fs && path && std::strlen(path) > 0 && n_blocks > 0 && blocks, -1, EINVAL);
    BlockTable t;
    PARAMETER_ASSERT(t.assign(blocks, n_blocks), -1, EINVAL);
    for (int i = 0; i < n_blocks; ++i) PARAMETER_ASSERT(blocks[i].n_replicas > 0, -1, EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    FileEntry &slot = fs->files[path];
    slot.pipeline_blocks = t;
    slot.pipeline = true;
    return 0;
}

int hdfs3_fs_set_block_size(hdfsFS fs, const char *path, int64_t block_size) {
    PARAMETER_ASSERT(fs && path && std::strlen(path) > 0 && block_size > 0, -1, EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    fs->files[path].block_size = block_size;
    return 0;
}

int hdfs3_fs_set_append_stamp(hdfsFS fs, const char *path, uint64_t new_generation_stamp) {
    PARAMETER_ASSERT(fs && path && std::strlen(path) > 0 && new_generation_stamp > 0, -1, EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    fs->files[path].append_gs = new_generation_stamp;
    return 0;
}

int hdfs3_fs_set_sink(hdfsFS fs, const char *path, hdfs3_packet_sink sink, void *user) {
    PARAMETER_ASSERT(fs && path && std::strlen(path) > 0 && sink, -1, EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    FileEntry &e = fs->files[path];
    e.sink = sink;
    e.user = user;
    return 0;
}

int hdfs3_fs_set_readahead(hdfsFS fs, int blocks, int64_t max_bytes_per_block) {
    PARAMETER_ASSERT(fs && blocks >= 0 && blocks <= HDFS3_READAHEAD_MAX_BLOCKS && max_bytes_per_block >= 0, -1,
                     EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    fs->readahead_blocks = blocks;
    fs->readahead_bytes = max_bytes_per_block;
    return 0;
}

int hdfsDisconnect(hdfsFS fs) {
    delete fs;  // Hdfs.cpp:629-636: a null fs is not an error
    return 0;
}

hdfsFile hdfsOpenFile(hdfsFS fs, const char *path, int flags, int bufferSize, short replication,
                      tOffset blocksize) {
    PARAMETER_ASSERT(fs && path && std::strlen(path) > 0, nullptr, EINVAL);
    PARAMETER_ASSERT(bufferSize >= 0 && replication >= 0 && blocksize >= 0, nullptr, EINVAL);
    PARAMETER_ASSERT(!(flags & O_RDWR) && !((flags & O_EXCL) && (flags & O_CREAT)), nullptr, ENOTSUP);
    const bool append = (flags & O_APPEND) != 0;
    const bool write = (flags & O_CREAT) || (flags & O_WRONLY) || append;
    hdfsFile file = new (std::nothrow) HdfsFileInternalWrapper();
    if (!file) {
        set_msg("Out of memory");
        errno = ENOMEM;
        return nullptr;
    }
    file->input = !write;
    int rc;
    {
        // held across the open: hdfs3_input_open copies the located blocks out of the table
        std::lock_guard<std::mutex> lk(fs->mu);
        auto it = fs->files.find(path);
        // append() needs the file (its located blocks stand in for the namenode's reply); a new file
        // needs somewhere to write (a sink or the blocks addBlock would allocate)
        const bool exists = it != fs->files.end() && it->second.located;
        const bool missing = append ? !exists
                             : write ? it == fs->files.end() || (!it->second.sink && !it->second.pipeline)
                                     : !exists;
        if (missing) {
            delete file;
            set_msg((std::string(write && !append ? "no write pipeline registered for " : "file does not exist: ") +
                     path)
                        .c_str());
            errno = ENOENT;  // FileNotFoundException -> ENOENT (Hdfs.cpp:243-327)
            return nullptr;
        }
        FileEntry &e = it->second;
        if (write) {
            hdfs3_writer_opts o = fs->wopts;
            if (blocksize > 0) o.block_size = blocksize;
            bool size_known = !append;  // a create sets the file's block size
            if (append) {
                // the reference appends with the file's own block size (FileStatus::getBlockSize,
                // OutputStreamImpl.cpp:196-230): the size registered for the path (hdfs3_fs_set_block_size,
                // or recorded by the write that created it), else a file of two or more blocks states
                // it by its first (every block but the last is full); a caller's size that disagrees is
                // refused, and no registered block may hold more than the size the stream will use.
                // A one-block file of unknown block size appends with the caller's (or the session's).
                const auto &lbs = e.located_blocks.blocks;
                if (e.block_size > 0 || lbs.size() >= 2) {
                    const int64_t fbs = e.block_size > 0 ? e.block_size : int64_t(lbs[0].block.num_bytes);
                    if (blocksize > 0 && blocksize != fbs) {
                        delete file;
                        set_msg("append: block size differs from the file's block size");
                        errno = EINVAL;
                        return nullptr;
                    }
                    o.block_size = fbs;
                    size_known = true;
                }
                for (size_t i = 0; i < lbs.size(); ++i) {
                    const int64_t nb = int64_t(lbs[i].block.num_bytes);
                    if (nb > o.block_size || (i + 1 < lbs.size() && nb != o.block_size)) {
                        delete file;
                        set_msg("append: the file's blocks do not match its block size");
                        errno = EINVAL;
                        return nullptr;
                    }
                }
                // addBlock never hands out a block the file already has: a pipeline table still
                // naming one of the file's blocks was left from an earlier write (the table is
                // consumed by each write, so appends register fresh blocks)
                if (e.pipeline)
                    for (const hdfs3_located_block &pbk : e.pipeline_blocks.blocks)
                        for (const hdfs3_located_block &fb : lbs)
                            if (pbk.block.block_id == fb.block.block_id) {
                                delete file;
                                set_msg("append: the registered pipeline names a block the file already has");
                                errno = EINVAL;
                                return nullptr;
                            }
            }
            // OutputStreamImpl::open rejects a block size that is not a multiple of the chunk
            // size (Hdfs.cpp:686-696) before anything reaches the pipeline
            if (o.bytes_per_checksum == 0 || o.block_size % o.bytes_per_checksum != 0) {
                delete file;
                set_msg("OutputStreamImpl: block size is not the multiply of chunk size.");
                errno = EINVAL;
                return nullptr;
            }
            // append (OutputStreamImpl::initAppend, OutputStreamImpl.cpp:172-230): the file's located
            // blocks play append()'s reply — its length, and its last block when that is partial
            hdfs3_append_info ai{0, -1};
            const hdfs3_located_block *last = nullptr;
            if (append) {
                const auto &lbs = e.located_blocks.blocks;
                for (const hdfs3_located_block &b : lbs) ai.file_length += int64_t(b.block.num_bytes);
                if (!lbs.empty() && ai.file_length % o.block_size != 0) {
                    last = &lbs.back();
                    ai.last_block_bytes = int64_t(last->block.num_bytes);
                }
            }
            if (e.pipeline || (last && !e.sink)) {  // datanodes: PipelineImpl behind the stream
                file->path = path;
                file->block_size = o.block_size;
                file->block_size_known = size_known;
                BlockTable t;
                std::vector<hdfs3_located_block> pb;
                if (last) pb.push_back(*last);  // its replicas are the append pipeline's nodes
                if (e.pipeline) pb.insert(pb.end(), e.pipeline_blocks.blocks.begin(), e.pipeline_blocks.blocks.end());
                t.assign(pb.data(), int(pb.size()));
                file->written = t;
                if (append) file->prefix.assign(e.located_blocks.blocks.data(),
                                                int(e.located_blocks.blocks.size()) - (last ? 1 : 0));
                if (last) {
                    const uint64_t gs = e.append_gs ? e.append_gs : last->block.generation_stamp + 1;
                    rc = hdfs3_pipeline_open_append(file->written.blocks.data(), int(file->written.blocks.size()), gs,
                                                    fs->client_name.c_str(), o.bytes_per_checksum, nullptr, &file->pipe);
                } else {
                    rc = hdfs3_pipeline_open(file->written.blocks.data(), int(file->written.blocks.size()),
                                             fs->client_name.c_str(), o.bytes_per_checksum, nullptr, &file->pipe);
                }
                if (rc == 0) rc = hdfs3_output_open_pipeline_append(&o, append ? &ai : nullptr, file->pipe, &file->out);
                if (rc == 0) {
                    // addBlock's blocks and updateBlockForPipeline's stamp are one write's: the next
                    // write or append registers its own (hdfs3_fs_set_pipeline / _set_append_stamp)
                    e.pipeline = false;
                    e.pipeline_blocks = BlockTable();
                    if (last) e.append_gs = 0;
                }
            } else {
                rc = hdfs3_output_open_append(&o, append ? &ai : nullptr, e.sink, e.user, &file->out);
            }
        } else {
            rc = hdfs3_input_open(e.located_blocks.blocks.data(), int(e.located_blocks.blocks.size()),
                                  fs->client_name.c_str(), &fs->ropts, &file->in);
            if (rc == 0 && fs->readahead_blocks > 0)
                rc = hdfs3_input_set_readahead(file->in, fs->readahead_blocks, fs->readahead_bytes);
            if (rc == 0 && fs->local_read && !e.local.empty()) {
                std::vector<hdfs3_local_replica> lr;
                for (const LocalFiles &l : e.local)
                    lr.push_back(hdfs3_local_replica{l.block, l.replica, l.data.c_str(), l.meta.c_str()});
                rc = hdfs3_input_set_local_replicas(file->in, lr.data(), int(lr.size()), &fs->lopts);
            }
            if (rc < 0 && file->in) {
                hdfs3_input_close(file->in);
                file->in = nullptr;
            }
        }
    }
    if (rc < 0) {
        set_msg(hdfs3_crc_last_error());
        if (file->pipe) hdfs3_pipeline_close(file->pipe);
        delete file;
        errno = -rc;
        return nullptr;
    }
    return file;
}

namespace {
// completeFile: after a clean close through datanodes the file is readable at the length the
// pipeline had acked per block (lastBlock->setNumBytes(bytesAcked), Pipeline.cpp:836), from the
// nodes it was written to — what getBlockLocations returns after complete()
void complete_written_file(hdfsFS fs, hdfsFile file) {
    std::vector<int64_t> acked(file->written.blocks.size(), 0);
    hdfs3_pipeline_stats(file->pipe, acked.data(), int(acked.size()), nullptr, nullptr);
    // an appended file keeps its earlier blocks; the appended one carries its new stamp
    std::vector<hdfs3_located_block> all(file->prefix.blocks.begin(), file->prefix.blocks.end());
    int64_t off = 0;
    for (const hdfs3_located_block &b : all) off += int64_t(b.block.num_bytes);
    for (size_t n = 0; n < acked.size() && acked[n] > 0; ++n) {
        hdfs3_located_block b = file->written.blocks[n];
        b.block.num_bytes = uint64_t(acked[n]);
        b.offset = off;
        (void)hdfs3_pipeline_generation_stamp(file->pipe, int(n), &b.block.generation_stamp);
        off += acked[n];
        all.push_back(b);
    }
    std::lock_guard<std::mutex> lk(fs->mu);
    FileEntry &slot = fs->files[file->path];
    slot.located_blocks.assign(all.data(), int(all.size()));
    slot.located = true;
    slot.local.clear();  // the entry was replaced: its replicas are the pipeline's nodes now
    if (file->block_size_known) slot.block_size = file->block_size;  // what FileStatus reports from now on
}
}  // namespace

int hdfsCloseFile(hdfsFS fs, hdfsFile file) {
    PARAMETER_ASSERT(fs, -1, EINVAL);
    if (!file) return 0;
    int rc = 0;
    if (file->input) {
        rc = hdfs3_input_close(file->in);
    } else {
        rc = hdfs3_output_close(file->out);  // frees the stream even on error
        if (file->pipe) {
            const int e = errno;
            const int prc = hdfs3_pipeline_flush(file->pipe);
            if (rc == 0 && prc == 0) complete_written_file(fs, file);
            hdfs3_pipeline_close(file->pipe);
            if (rc == 0 && prc < 0) {
                rc = -1;
                errno = -prc;
            } else {
                errno = e;
            }
        }
    }
    delete file;  // freed even after an I/O error (hdfs.h:328-330)
    if (rc < 0) return stream_failed(-1);
    return 0;
}

int hdfsExists(hdfsFS fs, const char *path) {
    PARAMETER_ASSERT(fs && path && std::strlen(path) > 0, -1, EINVAL);
    std::lock_guard<std::mutex> lk(fs->mu);
    auto it = fs->files.find(path);
    return it != fs->files.end() && it->second.located ? 0 : -1;
}

int hdfsSeek(hdfsFS fs, hdfsFile file, tOffset desiredPos) {
    PARAMETER_ASSERT(fs && file && desiredPos >= 0, -1, EINVAL);
    PARAMETER_ASSERT(file->input, -1, EINVAL);
    if (hdfs3_input_seek(file->in, desiredPos) < 0) return stream_failed(-1);
    return 0;
}

tOffset hdfsTell(hdfsFS fs, hdfsFile file) {
    PARAMETER_ASSERT(fs && file, -1, EINVAL);
    const int64_t t = file->input ? hdfs3_input_tell(file->in) : hdfs3_output_tell(file->out);
    if (t < 0) return stream_failed(tOffset(-1));
    return t;
}

tSize hdfsRead(hdfsFS fs, hdfsFile file, void *buffer, tSize length) {
    PARAMETER_ASSERT(fs && file && buffer && length > 0, -1, EINVAL);
    PARAMETER_ASSERT(file->input, -1, EINVAL);
    const int32_t n = hdfs3_input_read(file->in, buffer, length);
    if (n < 0) return stream_failed(tSize(-1));
    return n;  // 0 at end of file (HdfsEndOfStream, Hdfs.cpp:831-832)
}

tSize hdfsPread(hdfsFS fs, hdfsFile file, void *buffer, tSize length, tOffset position) {
    PARAMETER_ASSERT(fs && file && buffer && length > 0 && position >= 0, -1, EINVAL);
    PARAMETER_ASSERT(file->input, -1, EINVAL);
    const int32_t n = hdfs3_input_pread(file->in, position, buffer, length);
    if (n < 0) return stream_failed(tSize(-1));
    return n;
}

// hdfsRead / hdfsPread into device memory (not in hdfs.h): same checks, returns and errno
tSize hdfs3_fs_read_dev(hdfsFS fs, hdfsFile file, void *d_buffer, tSize length) {
    PARAMETER_ASSERT(fs && file && d_buffer && length > 0, -1, EINVAL);
    PARAMETER_ASSERT(file->input, -1, EINVAL);
    const int32_t n = hdfs3_input_read_dev(file->in, d_buffer, length);
    if (n < 0) return stream_failed(tSize(-1));
    return n;
}

tSize hdfs3_fs_pread_dev(hdfsFS fs, hdfsFile file, void *d_buffer, tSize length, tOffset position) {
    PARAMETER_ASSERT(fs && file && d_buffer && length > 0 && position >= 0, -1, EINVAL);
    PARAMETER_ASSERT(file->input, -1, EINVAL);
    const int32_t n = hdfs3_input_pread_dev(file->in, position, d_buffer, length);
    if (n < 0) return stream_failed(tSize(-1));
    return n;
}

tSize hdfsWrite(hdfsFS fs, hdfsFile file, const void *buffer, tSize length) {
    PARAMETER_ASSERT(fs && file && buffer && length > 0, -1, EINVAL);
    PARAMETER_ASSERT(!file->input, -1, EINVAL);
    if (hdfs3_output_write(file->out, buffer, length) < 0) return stream_failed(tSize(-1));
    return length;
}

// hdfsWrite from device memory (not in hdfs.h): same checks, return and errno
tSize hdfs3_fs_write_dev(hdfsFS fs, hdfsFile file, const void *d_buffer, tSize length) {
    PARAMETER_ASSERT(fs && file && d_buffer && length > 0, -1, EINVAL);
    PARAMETER_ASSERT(!file->input, -1, EINVAL);
    if (hdfs3_output_write_dev(file->out, d_buffer, length) < 0) return stream_failed(tSize(-1));
    return length;
}

int64_t hdfs3_fs_writev_dev(hdfsFS fs, hdfsFile file, const hdfs3_dev_iovec *iov, int n) {
    PARAMETER_ASSERT(fs && file && n >= 0 && (iov || n == 0), -1, EINVAL);
    PARAMETER_ASSERT(!file->input, -1, EINVAL);
    const int64_t total = hdfs3_output_writev_dev(file->out, iov, n);
    if (total < 0) return stream_failed(int64_t(-1));
    return total;
}

int hdfsFlush(hdfsFS fs, hdfsFile file) {
    PARAMETER_ASSERT(fs && file, -1, EINVAL);
    return hdfsHFlush(fs, file);
}

int hdfsHFlush(hdfsFS fs, hdfsFile file) {
    PARAMETER_ASSERT(fs && file, -1, EINVAL);
    PARAMETER_ASSERT(!file->input, -1, EINVAL);
    if (hdfs3_output_flush(file->out) < 0) return stream_failed(-1);
    return 0;
}

int hdfsSync(hdfsFS fs, hdfsFile file) {
    PARAMETER_ASSERT(fs && file, -1, EINVAL);
    PARAMETER_ASSERT(!file->input, -1, EINVAL);
    if (hdfs3_output_sync(file->out) < 0) return stream_failed(-1);
    return 0;
}

int hdfsAvailable(hdfsFS fs, hdfsFile file) {
    PARAMETER_ASSERT(fs && file, -1, EINVAL);
    PARAMETER_ASSERT(file->input, -1, EINVAL);
    const int a = hdfs3_input_available(file->in);
    if (a < 0) return stream_failed(-1);
    return a < std::numeric_limits<int>::max() ? a : std::numeric_limits<int>::max();
}

}  // extern "C"
