#include "batch_ledger.h"

#include <algorithm>

namespace hdfs3crc {

void BatchLedger::add(std::vector<ByteRange> &v, bool &sorted, uint64_t off, uint64_t len) {
    if (!len) return;
    if (!v.empty()) {
        ByteRange &b = v.back();
        if (b.off + b.len == off) {
            b.len += len;
            return;
        }
        if (off < b.off + b.len) sorted = false;
    }
    v.push_back(ByteRange{off, len});
}

// ascending, overlapping and abutting ranges merged
void BatchLedger::merged(const std::vector<ByteRange> &v, bool sorted, std::vector<ByteRange> *out) {
    out->assign(v.begin(), v.end());
    if (!sorted)
        std::sort(out->begin(), out->end(), [](const ByteRange &a, const ByteRange &b) { return a.off < b.off; });
    size_t n = 0;
    for (const ByteRange &r : *out) {
        if (n && r.off <= (*out)[n - 1].off + (*out)[n - 1].len) {
            ByteRange &b = (*out)[n - 1];
            b.len = std::max(b.off + b.len, r.off + r.len) - b.off;
        } else {
            (*out)[n++] = r;
        }
    }
    out->resize(n);
}

void BatchLedger::coalesce(const std::vector<ByteRange> &mine, bool mine_sorted, const std::vector<ByteRange> &other,
                           bool other_sorted, std::vector<ByteRange> *out) {
    out->clear();
    if (mine.empty()) return;
    if (other.empty()) {  // nothing to step around: first byte to last
        uint64_t lo = UINT64_MAX, hi = 0;
        for (const ByteRange &r : mine) {
            lo = std::min(lo, r.off);
            hi = std::max(hi, r.off + r.len);
        }
        out->push_back(ByteRange{lo, hi - lo});
        return;
    }
    std::vector<ByteRange> a, b;
    merged(mine, mine_sorted, &a);
    merged(other, other_sorted, &b);
    size_t j = 0;
    for (const ByteRange &r : a) {
        if (!out->empty()) {
            ByteRange &last = out->back();
            const uint64_t gap_lo = last.off + last.len, gap_hi = r.off;
            while (j < b.size() && b[j].off + b[j].len <= gap_lo) ++j;
            if (j == b.size() || b[j].off >= gap_hi) {  // no byte of the other kind in the gap
                last.len = r.off + r.len - last.off;
                continue;
            }
        }
        out->push_back(r);
    }
}

}  // namespace hdfs3crc
