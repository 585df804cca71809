// callable.h — the callable runs (--callable FILE) on the host: the chunks'
// (site ranges') row lists, their stitch in file order, the rows of the
// host path (sid_callable_host), the join of two neighbouring row lists and the
// BED formatter.  No HIP here: callable.cpp builds into a stand-alone host
// program (tests/asan).
//
// A row is a maximal run of consecutive sites that are all callable (sid.h
// Conventions), with byte-equal chrom and each pos the previous pos + 1.  The
// device finds the runs of one chunk (textpath.hip, the run rows' CallRuns): a
// chunk's first site, if callable, always opens a row, so a run that crosses a
// chunk edge comes back as two rows, which the stitch joins -- through chunks
// without a site, and only when the earlier chunk's last site lies in its last
// row, the later chunk's first site in its first row, the chroms are equal and
// the later row starts where the earlier one ends.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "rowtable.h"

// One row as the device writes it and the host reads it back.
struct sid_call_row {
    uint64_t c8;        // the chrom's first min(clen, 8) bytes, byte k in bits 8k .. 8k + 7
    int32_t pos;        // the run's first pos (>= 1)
    uint32_t clen;      // the chrom's length
    uint32_t name;      // clen > 8: the offset of the chrom's bytes in the chunk's name blob
    uint32_t sites;     // a chunk holds fewer than 2^32
    uint32_t het;
    uint32_t pad;
};
static_assert(sizeof(sid_call_row) == 32, "the device's row layout");

// the three facts about a chunk (sid_call_chunk::edge; the device's word likewise)
enum { SID_CALL_HAS_SITE = 1, SID_CALL_OPEN_START = 2, SID_CALL_OPEN_END = 4 };

// One chunk's rows in file order, with the bytes of its chroms over 8 bytes and
// its edge bits: it has a site; its first site lies in its first row; its last
// site lies in its last row.
struct sid_call_chunk {
    std::vector<sid_call_row> rows;
    std::string names;
    uint32_t edge = 0;
    void clear()
    {
        rows.clear();
        names.clear();
        edge = 0;
    }
};

// The rows of a run: what sid_callable_host and sid_dtext_callable hand out (rowtable.h).
struct sid_call_table : sid_row_table<sid_callable_row> {
    bool open = false;   // the last site pushed lies in the last row
    void clear()
    {
        sid_row_table::clear();
        open = false;
    }
    // one more row in file order; join: its first site follows the table's last site with nothing between
    // (merged into the last row when that one is open, the chroms are equal and start == its end)
    void push(const char* chrom, uint32_t clen, int64_t start, int64_t end, uint64_t het, bool join);
    void finish();
};

// chunk c's rows appended to the table (chunks in file order)
void sid_call_stitch_push(sid_call_table* t, const sid_call_chunk& c);

// The whole stitch over nchunks row lists at once (tests, and callers that cut
// a run into ranges): chunk c's rows are rows[off[c], off[c + 1]), its name blob
// names[noff[c], noff[c + 1]), its edge bits edge[c].  The result is freed with
// sid_callable_free.  SID_EINVAL for a NULL array, a row whose name lies outside
// its chunk's blob, a row without a site or with pos < 1, or edge bits that
// contradict the rows (rows or an open edge without a site).
extern "C" int sid_callable_stitch_chunks(const sid_call_row* rows, const uint64_t* off, const char* names,
                                          const uint64_t* noff, const uint32_t* edge, size_t nchunks,
                                          sid_callable_row** out, size_t* n);
// a table's rows as one allocation (rows, then the names) for sid_callable_free
int sid_call_export(const sid_call_table& t, sid_callable_row** out, size_t* n);
