// context.h — the context (sid_opts.context, --context N) on the host: the
// mark of the host path (sid_context_mark) and the stitch of the chunks' forced
// edge records (the engine's emit).  No HIP here: context.cpp builds into a
// stand-alone host program (tests/asan).
//
// A chunk is marked on the device before its neighbours' labels exist, so its
// first and last min(N, records) records are always formatted (forced) and a
// descriptor says what the chunk alone knows about them.  Once the descriptors
// are there in file order the stitch decides every forced record: kept when
// the in-chunk verdict says so, or when a selected record of a neighbouring
// chunk is within N records -- the distance carried through chunks without a
// selected record.  The records not kept are cut out of the chunk's bytes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sid.h"

// One chunk's descriptor, as the device writes it (textpath.hip) and the
// engine reads it back with the chunk's byte count.
struct sid_cx_desc {
    uint32_t records;     // the chunk's records (of U)
    uint32_t has_sel;     // it holds a selected record
    uint32_t lead;        // records before its first selected one, saturated at N + 1
    uint32_t trail;       // records after its last selected one, saturated at N + 1
    uint64_t head_keep;   // bit k: the in-chunk verdict keeps record k              (k < min(N, records))
    uint64_t tail_keep;   // bit k: ... record records - min(N, records) + k
    uint32_t head_len[SID_CONTEXT_MAX];   // the bytes of those records, newline included
    uint32_t tail_len[SID_CONTEXT_MAX];
};

struct sid_cx_range {
    uint64_t off, len;
};

// The final verdicts of one chunk's forced records (bits as head_keep /
// tail_keep; a record in both zones has the same bit in both).
struct sid_cx_verdict {
    uint64_t head_keep = 0, tail_keep = 0;
};

// The stitch, fed the descriptors in file order.  A chunk's verdict is final
// once no later chunk can reach its last records: resolved() chunks are.
class sid_cx_stitch {
  public:
    explicit sid_cx_stitch(int context) : n_((uint32_t)context), since_((uint32_t)context + 1) {}
    void push(const sid_cx_desc& d);
    void finish();   // the input's end: nothing follows
    size_t chunks() const { return v_.size(); }
    size_t resolved() const { return resolved_; }
    const sid_cx_verdict& verdict(size_t c) const { return v_[c]; }

  private:
    struct Pending {
        size_t chunk;
        uint32_t first;   // its records [first, records) wait for a selected record behind them
        uint32_t after;   // records seen behind the chunk so far
        uint32_t records;
    };
    void keep_bit(sid_cx_verdict& v, uint32_t records, uint32_t idx);
    void settle();
    uint32_t n_, since_;   // since_: records since the last selected one, saturated at N + 1
    std::vector<sid_cx_verdict> v_;
    std::vector<Pending> pend_;
    size_t resolved_ = 0;
};

// min(N, records): the records of each forced zone
inline uint32_t sid_cx_zone(const sid_cx_desc& d, int context)
{
    return d.records < (uint32_t)context ? d.records : (uint32_t)context;
}
// The byte ranges of a chunk's `total` bytes that stay, in order (at most
// 2 N + 1 of them; out needs 2 * SID_CONTEXT_MAX + 1 entries).  Returns their
// number; *kept = their bytes.
size_t sid_cx_ranges(const sid_cx_desc& d, int context, const sid_cx_verdict& v, uint64_t total, sid_cx_range* out,
                     uint64_t* kept);
// The bytes moved together in place; returns the new length.
uint64_t sid_cx_compact(char* bytes, const sid_cx_range* r, size_t nr);
// head_len / tail_len of d from the chunk's bytes (what the device's edge
// kernel computes): records end in '\n', the last one may lack it.
extern "C" void sid_cx_edge_lengths(const char* bytes, uint64_t total, int context, sid_cx_desc* d);
// The whole stitch over n chunks at once (tests; the engine feeds the class
// above as the chunks arrive): chunk c's bytes are bytes[off[c], off[c] +
// len[c]); they are cut down in place to what the stitch keeps, len[c]
// updated.  SID_EINVAL for a context outside 0 .. 64 or a NULL array.
extern "C" int sid_cx_stitch_chunks(const sid_cx_desc* d, size_t n, int context, char* bytes, const uint64_t* off,
                                    uint64_t* len);
