// region_stats.h — the region rows (sid_engine_set_region_stats, --region-stats
// FILE) on the host: the chunks' row lists as the device hands them back, their
// sum in a dense table of one entry per interval, the rows of the host path
// (sid_region_stats_host), the merge and the CSV formatter.  No HIP here:
// region_stats.cpp builds into a stand-alone host program (tests/asan).
//
// A row is one interval of the region set after its merge.  The device bins
// the sites of one chunk by the interval's index in the flat table
// (textpath.hip, sid_region_stats_*_kernel) and hands back the chunk's touched
// bins in the order they were first touched; the engine checks them, keeps
// them with the chunk's record and adds the chunks up at the emit into a table
// of sid_regions_intervals entries, which sid_rs_export turns into rows in the
// set's source order (regions.h, sid_regions::row).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sid.h"
#include "regions.h"

// One row as the device writes it and the engine reads it back (a chunk has
// fewer than 2^32 sites): idx is the interval's index in the flat table.
struct sid_rs_row {
    uint64_t depth;
    uint32_t idx;
    uint32_t sites;
    uint32_t het;
    uint32_t hom;
};
static_assert(sizeof(sid_rs_row) == 24, "the device's row layout");

// One bin of the device's per-chunk table (all zero between two stage runs).
struct sid_rs_bin {
    unsigned long long depth;
    uint32_t sites;
    uint32_t het;
    uint32_t hom;
    uint32_t pad;
};
static_assert(sizeof(sid_rs_bin) == 24, "the device's bin layout");

// One interval's sums over a run.
struct sid_rs_sum {
    uint64_t sites = 0, depth = 0, het = 0, hom = 0;
};

// a chunk's rows as read back against a set of ni intervals; false: an index twice or outside the set, a row
// without a site, or more records than sites
bool sid_rs_check(const std::vector<sid_rs_row>& rows, size_t ni);
// the checked rows of one chunk added into the run's table (ni entries, by the flat table's index)
void sid_rs_add(std::vector<sid_rs_sum>* table, const std::vector<sid_rs_row>& chunk);
// a table as rows in the set's source order, one allocation for sid_region_stats_free; the chrom pointers are
// the set's (valid while r lives) unless own_names, which copies the names behind the rows
int sid_rs_export(const sid_regions* r, const std::vector<sid_rs_sum>& table, bool own_names, sid_region_row** out,
                  size_t* n);
