// regions.h — a region set (sid_regions, --regions): host object and the flat
// table the device kernels search.  No HIP here: regions.cpp builds into a
// stand-alone host program (tests/asan).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sid.h"

// The set after the merge.  Chroms are sorted by (first 8 bytes of the name as
// a little-endian u64, zero-padded; length; bytes) -- the order of the form the
// device formatters carry a site's chrom in (Head{clen, c8, cb}) -- and chrom k
// owns the sorted, disjoint, non-empty intervals [ibeg[k], ibeg[k + 1]):
// a position p is inside when start[j] < p <= end[j] (BED: 0-based, half-open).
struct sid_regions {
    std::vector<std::string> name;
    std::vector<uint64_t> c8;
    std::vector<uint32_t> ibeg;   // name.size() + 1 entries
    std::vector<int32_t> start, end;
    // The source order (the region rows, region_stats.h): rank[k] is chrom k's
    // place among the chroms by their first non-empty interval in the source,
    // and row[r] the interval of row r -- chroms by rank, a chrom's intervals
    // ascending.  Neither is part of the flat table.
    std::vector<uint32_t> rank;   // name.size() entries
    std::vector<uint32_t> row;    // start.size() entries
};

// first 8 bytes of a name, byte k in bits 8k.., zero beyond its length
uint64_t sid_regions_c8(const char* s, size_t n);

// The flat table: one buffer, every array at a 16-B aligned offset.
//   c8 (u64 x nc) | clen (u32 x nc) | noff (u32 x nc) | ibeg (u32 x (nc + 1)) |
//   start (i32 x ni) | end (i32 x ni) | names (the bytes of every name, at noff)
struct sid_regions_layout {
    uint32_t nc = 0, ni = 0;
    size_t c8 = 0, clen = 0, noff = 0, ibeg = 0, start = 0, end = 0, names = 0, bytes = 0;
};
void sid_regions_flatten(const sid_regions* r, std::vector<char>& buf, sid_regions_layout* L);
