// The output stream's per-batch bookkeeping of who wrote which bytes of the batch arena: the host
// (hdfs3_output_write's memcpy, the re-sent partial chunk) or the device (hdfs3_output_write_dev's
// placement launches into the arena's device copy). At dispatch it answers what to upload (the host's
// ranges: an upload across a placed range would overwrite it with stale host memory) and what to copy
// back (the placed ranges: the sink is handed host packets). Plain host arithmetic, no GPU runtime
// (tests/native/write_ledger_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace hdfs3crc {

struct ByteRange {
    uint64_t off, len;  // arena offsets
};

class BatchLedger {
public:
    // [off, off + len) was written by the host / placed from the device. Empty ranges are dropped; a
    // range that continues the one before it of the same kind extends it (a packet filled by many
    // small writes stays one range).
    void host(uint64_t off, uint64_t len) { add(host_, host_sorted_, off, len); }
    void device(uint64_t off, uint64_t len) { add(dev_, dev_sorted_, off, len); }
    // the batch went to the sink: its slots are reused from the first on
    void clear() {
        host_.clear();
        dev_.clear();
        host_sorted_ = dev_sorted_ = true;
    }
    bool any_host() const { return !host_.empty(); }
    bool any_device() const { return !dev_.empty(); }  // a copy back to the host is needed
    // The copies to the device: the host's ranges in ascending order, overlapping and abutting ones
    // merged, and two neighbours joined across the gap between them when no placed byte lies in it (the
    // gap is then a slot's lead or stale host bytes nothing reads). A batch without placed bytes is
    // therefore ONE range from its first host byte to its last, the upload it always was.
    void uploads(std::vector<ByteRange> *out) const { coalesce(host_, host_sorted_, dev_, dev_sorted_, out); }
    // The copies back to the host: the placed ranges, treated the same way against the host's.
    void downloads(std::vector<ByteRange> *out) const { coalesce(dev_, dev_sorted_, host_, host_sorted_, out); }

private:
    static void add(std::vector<ByteRange> &v, bool &sorted, uint64_t off, uint64_t len);
    static void merged(const std::vector<ByteRange> &v, bool sorted, std::vector<ByteRange> *out);
    static void coalesce(const std::vector<ByteRange> &mine, bool mine_sorted, const std::vector<ByteRange> &other,
                         bool other_sorted, std::vector<ByteRange> *out);
    std::vector<ByteRange> host_, dev_;
    bool host_sorted_ = true, dev_sorted_ = true;  // recorded in ascending, non-overlapping order so far
};

}  // namespace hdfs3crc
