// rowtable.h — what the row tables of windows.h and callable.h share on the
// host: rows in file order with each chrom's bytes stored once per run of its
// rows, their export as one allocation, a device row's chrom, the host paths'
// chromosome search and the decimal writers.  No HIP here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sid.h"

// The rows of a run, of the public type Row (chrom, chrom_len, ...).  The chrom
// pointers point into `names` and are set by finish().  (Hidden: libsid.so
// exports what sid_win_table and sid_call_table define themselves.)
template <class Row>
struct __attribute__((visibility("hidden"))) sid_row_table {
    std::vector<Row> rows;
    std::vector<uint64_t> name_off;
    std::string names;
    void clear()
    {
        rows.clear();
        name_off.clear();
        names.clear();
    }
    // whether the last row's chrom is this one (an empty table: no)
    bool same_chrom(const char* chrom, uint32_t clen) const
    {
        if (rows.empty()) return false;
        const char* ln = names.data() + name_off.back();
        return rows.back().chrom_len == clen && (clen == 0 || std::memcmp(ln, chrom, clen) == 0);
    }
    // one more row; same: same_chrom(chrom, r.chrom_len) (the chrom's bytes once per run of its rows)
    void append(const Row& r, const char* chrom, bool same)
    {
        name_off.push_back(same ? name_off.back() : names.size());
        if (!same) names.append(chrom, r.chrom_len);
        rows.push_back(r);
    }
    void finish()
    {
        for (size_t k = 0; k < rows.size(); ++k) rows[k].chrom = names.data() + name_off[k];
    }
    // the rows as one allocation (the rows, then the names): std::free of the rows' pointer frees both
    int export_rows(Row** out, size_t* n) const
    {
        const size_t nr = rows.size();
        char* mem = (char*)std::malloc(std::max<size_t>(nr * sizeof(Row) + names.size(), 1));
        if (!mem) return SID_ENOMEM;
        Row* r = (Row*)mem;
        char* nm = mem + nr * sizeof(Row);
        if (!names.empty()) std::memcpy(nm, names.data(), names.size());
        for (size_t k = 0; k < nr; ++k) {
            r[k] = rows[k];
            r[k].chrom = nm + name_off[k];
        }
        *out = r;
        *n = nr;
        return SID_OK;
    }
};

// the chrom of a device row (c8, clen, name): in the chunk's name blob, or its 8 bytes unpacked into tmp
template <class DevRow>
static inline const char* sid_row_chrom(const DevRow& r, const char* names, char (&tmp)[8])
{
    if (r.clen > 8) return names + r.name;
    for (int k = 0; k < 8; ++k) tmp[k] = (char)(r.c8 >> (8 * k));
    return tmp;
}

// the chromosome run holding site `begin` (seg_start: the runs' first sites, ascending)
static inline size_t sid_seg_of(const std::vector<uint64_t>& seg_start, size_t begin)
{
    size_t lo = 0, hi = seg_start.size();
    while (lo + 1 < hi) {
        const size_t mid = (lo + hi) / 2;
        if (seg_start[mid] <= begin) lo = mid; else hi = mid;
    }
    return lo;
}

// decimal digits of u (v) at p; they return their number
static inline size_t sid_put_u64(uint64_t u, char* p)
{
    char tmp[24];
    size_t k = 0, w = 0;
    do tmp[k++] = (char)('0' + u % 10); while (u /= 10);
    while (k) p[w++] = tmp[--k];
    return w;
}
static inline size_t sid_put_i64(int64_t v, char* p)
{
    if (v >= 0) return sid_put_u64((uint64_t)v, p);
    *p = '-';
    return 1 + sid_put_u64(0 - (uint64_t)v, p + 1);
}
