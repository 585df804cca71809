// depth_hist.h — the depth histogram (sid_engine_set_depth_hist, --depth-hist
// FILE) on the host: the chunks' row lists, their sum in file order, the rows
// of the host path (sid_depth_hist_host), the merge and the CSV formatter.  No
// HIP here: depth_hist.cpp builds into a stand-alone host program
// (tests/asan).
//
// A row is one depth that at least one site has.  The device bins the sites of
// one chunk (textpath.hip, sid_depth_hist_*_kernel) and hands back the chunk's
// non-zero bins in the order they were first touched; the engine sorts them,
// keeps them with the chunk's record and adds the chunks up at the emit -- a
// sorted merge, no dense array of 262141 bins.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sid.h"

// One row as the device writes it and the engine reads it back (a chunk has
// fewer than 2^32 sites).
struct sid_dh_row {
    uint32_t depth;
    uint32_t sites;
    uint32_t het;
    uint32_t hom;
};
static_assert(sizeof(sid_dh_row) == 16, "the device's row layout");

// One bin of the device's per-chunk table, a depth's (all zero between two stage runs).
struct sid_dh_bin {
    uint32_t sites;
    uint32_t het;
    uint32_t hom;
};
static_assert(sizeof(sid_dh_bin) == 12, "the device's bin layout");

constexpr uint32_t SID_DH_BINS = SID_DEPTH_MAX + 1;   // depths 0 .. 262140

// a chunk's rows as read back, sorted by depth in place; false: a depth twice or outside the range
bool sid_dh_sort(std::vector<sid_dh_row>* rows);
// the sorted rows of one chunk added into the run's table (sorted, stays sorted)
void sid_dh_add(std::vector<sid_depth_row>* table, const std::vector<sid_dh_row>& chunk);
// a table as one allocation for sid_depth_hist_free
int sid_dh_export(const std::vector<sid_depth_row>& t, sid_depth_row** out, size_t* n);
