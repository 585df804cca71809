// windows.h — the windowed summary (sid_opts.window, --windows W) on the host:
// the chunks' row lists, their stitch in file order, the rows of the host path
// (sid_windows_host) and the CSV formatter.  No HIP here: windows.cpp builds
// into a stand-alone host program (tests/asan).
//
// A row is a maximal run of consecutive sites with byte-equal chrom and equal
// window index wi = floor((pos - 1) / W).  The device finds the runs of one
// chunk (textpath.hip, the run rows' WinRuns): a chunk's first site always opens
// a row, so a run that crosses a chunk edge comes back as two rows with equal
// keys, which the stitch adds up -- through chunks without a site, and only
// when the two rows are neighbours in file order.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "rowtable.h"

// One row as the device writes it and the engine reads it back.
struct sid_win_row {
    int64_t wi;         // the window's index
    uint64_t c8;        // the chrom's first min(clen, 8) bytes, byte k in bits 8k .. 8k + 7
    uint32_t clen;      // the chrom's length
    uint32_t name;      // clen > 8: the offset of the chrom's bytes in the chunk's name blob
    uint32_t sites;     // a chunk holds fewer than 2^32 of each
    uint32_t records;
    uint32_t het;
    uint32_t pad;
};
static_assert(sizeof(sid_win_row) == 40, "the device's row layout");

// One chunk's rows in file order, with the bytes of its chroms over 8 bytes.
struct sid_win_chunk {
    std::vector<sid_win_row> rows;
    std::string names;
    void clear()
    {
        rows.clear();
        names.clear();
    }
};

// The rows of a run: what sid_engine_windows hands out (rowtable.h).
struct sid_win_table : sid_row_table<sid_window> {
    int64_t window = 0;
    // one more site run in file order: merged into the last row when their keys are equal
    void push(const char* chrom, uint32_t clen, int64_t wi, uint64_t sites, uint64_t records, uint64_t het);
    void finish();
};

inline int64_t sid_win_index(int64_t pos, int64_t W)
{
    const int64_t p = pos - 1;
    return p >= 0 ? p / W : -((-p + W - 1) / W);
}

// chunk c's rows appended to the table (chunks in file order)
void sid_win_stitch_push(sid_win_table* t, const sid_win_chunk& c);

// The whole stitch over nchunks row lists at once (tests; the engine pushes the
// chunks itself): chunk c's rows are rows[off[c], off[c + 1]), its name blob
// names[noff[c], noff[c + 1]).  The result is freed with sid_windows_free.
// SID_EINVAL for a window outside 1 .. 2^31-1, a NULL array, or a row whose
// name lies outside its chunk's blob.
extern "C" int sid_win_stitch_chunks(const sid_win_row* rows, const uint64_t* off, const char* names,
                                     const uint64_t* noff, size_t nchunks, int window, sid_window** out, size_t* n);
// a table's rows as one allocation (rows, then the names) for sid_windows_free
int sid_win_export(const sid_win_table& t, sid_window** out, size_t* n);
