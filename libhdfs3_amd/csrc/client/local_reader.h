// Internal entry points of the short-circuit reader shared with the input stream.
#pragma once

#include "hdfs3_client.h"

namespace hdfs3crc {

// what the input stream's open of a local replica adds to hdfs3_local_reader_open
struct LocalOpenExtra {
    // one past the last byte the caller will read, block-relative (<= 0: the block's end). The loader
    // stops at the end of the buffer_size buffer holding that byte (local_range.h): nothing beyond it is
    // read or verified, and the reader reports the end of the block there.
    int64_t range_end = 0;
    // the block length comes from the namenode, not from the file: a block file shorter than it opens and
    // fails when the loader reaches the missing bytes (-EIO, as the reference's read does), an offset
    // beyond the file fails the open
    bool replica = false;
    // out: the open failed on this host's GPU or memory (a context, the windows), not on the files
    bool host_fault = false;
};

int open_local_reader(const char *data_path, const char *meta_path, int64_t num_bytes, int64_t offset,
                      const hdfs3_local_opts *opts, LocalOpenExtra *extra, hdfs3_local_reader **out);

// true when the reader's failure came from this host's GPU or pinned memory (a HIP error), not from the
// block file, its .meta or their contents: the input stream must not abandon the replica for it
bool local_reader_host_fault(const hdfs3_local_reader *r);

// the limits hdfs3_local_reader_open puts on hdfs3_local_opts, for a caller that stores them for later
// opens; 0 or -EINVAL with the message set
int local_opts_check(const hdfs3_local_opts *opts);

}  // namespace hdfs3crc
