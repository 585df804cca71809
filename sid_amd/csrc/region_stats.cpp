// region_stats.cpp — the region rows on the host (region_stats.h): the check
// and the sum of the chunks' rows, the rows of the host path
// (sid_region_stats_host), the merge of two row lists and the CSV formatter.
// Pure host code, no HIP call.
#include "region_stats.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rowtable.h"
#include "sites.h"

bool sid_rs_check(const std::vector<sid_rs_row>& rows, size_t ni)
{
    if (rows.size() > ni) return false;
    std::vector<uint32_t> idx;
    idx.reserve(rows.size());
    for (const sid_rs_row& r : rows) {
        if (r.idx >= ni || r.sites == 0 || (uint64_t)r.het + r.hom > r.sites) return false;
        idx.push_back(r.idx);
    }
    std::sort(idx.begin(), idx.end());
    return std::adjacent_find(idx.begin(), idx.end()) == idx.end();
}

void sid_rs_add(std::vector<sid_rs_sum>* table, const std::vector<sid_rs_row>& chunk)
{
    for (const sid_rs_row& r : chunk) {
        if (r.idx >= table->size()) continue;   // (never: sid_rs_check)
        sid_rs_sum& t = (*table)[r.idx];
        t.sites += r.sites, t.depth += r.depth, t.het += r.het, t.hom += r.hom;
    }
}

// rows and, behind them, name bytes in one allocation
static sid_region_row* alloc_rows(size_t n, size_t name_bytes, char** names)
{
    const size_t rb = n * sizeof(sid_region_row);
    char* p = (char*)std::malloc(std::max<size_t>(rb + name_bytes, 1));
    if (!p) return nullptr;
    *names = p + rb;
    return (sid_region_row*)p;
}

int sid_rs_export(const sid_regions* r, const std::vector<sid_rs_sum>& table, bool own_names, sid_region_row** out,
                  size_t* n)
{
    if (!r || table.size() != r->start.size() || r->row.size() != r->start.size()) return SID_EINVAL;
    const size_t ni = table.size(), nc = r->name.size();
    size_t nb = 0;
    std::vector<size_t> noff(nc, 0);
    if (own_names)
        for (size_t k = 0; k < nc; ++k) noff[k] = nb, nb += r->name[k].size();
    char* names = nullptr;
    sid_region_row* rows = alloc_rows(ni, nb, &names);
    if (!rows) return SID_ENOMEM;
    if (own_names)
        for (size_t k = 0; k < nc; ++k)
            if (!r->name[k].empty()) std::memcpy(names + noff[k], r->name[k].data(), r->name[k].size());
    size_t k = 0;   // the chrom of the row: rows run chrom by chrom
    for (size_t j = 0; j < ni; ++j) {
        const uint32_t t = r->row[j];
        if (!(r->ibeg[k] <= t && t < r->ibeg[k + 1]))
            k = (size_t)(std::upper_bound(r->ibeg.begin(), r->ibeg.end(), t) - r->ibeg.begin()) - 1;
        const sid_rs_sum& s = table[t];
        sid_region_row& o = rows[j];
        o.chrom = own_names ? names + noff[k] : r->name[k].data();
        o.chrom_len = (uint32_t)r->name[k].size();
        o.start = r->start[t], o.end = r->end[t];
        o.sites = s.sites, o.depth = s.depth, o.records = s.het + s.hom, o.het = s.het, o.hom = s.hom;
    }
    *out = rows;
    *n = ni;
    return SID_OK;
}

extern "C" void sid_region_stats_free(sid_region_row* rows) { std::free(rows); }

extern "C" int sid_region_stats_valid(const sid_regions* r)
{
    if (!r) return SID_EINVAL;
    return r->start.size() <= (size_t)SID_REGION_STATS_MAX ? SID_OK : SID_EINVAL;
}

// the interval of chrom k (its range of the flat table) that holds pos, or -1
static long interval_of(const sid_regions* r, size_t k, int32_t pos)
{
    const int32_t* s0 = r->start.data() + r->ibeg[k];
    const int32_t* s1 = r->start.data() + r->ibeg[k + 1];
    const int32_t* p = std::lower_bound(s0, s1, pos);   // first start >= pos
    if (p == s0) return -1;
    const size_t j = (size_t)(p - 1 - r->start.data());   // the last start < pos
    return pos <= r->end[j] ? (long)j : -1;
}

extern "C" int sid_region_stats_host(const sid_regions* r, const sid_sites* s, size_t begin, size_t end,
                                     const uint8_t* code_all, sid_region_row** out, size_t* n)
{
    if (!out || !n) return SID_EINVAL;
    *out = nullptr, *n = 0;
    if (!r || !s || begin > end || end > s->pos.size() || s->counts.size() != 4 * s->pos.size()) return SID_EINVAL;
    if (end > begin && !code_all) return SID_EINVAL;
    std::vector<sid_rs_sum> table(r->start.size());
    size_t k = 0;   // the chromosome run holding i
    for (size_t i = begin; i < end;) {
        while (k + 1 < s->seg_start.size() && s->seg_start[k + 1] <= i) ++k;
        const size_t run_end = std::min<size_t>(end, k + 1 < s->seg_start.size() ? s->seg_start[k + 1] : end);
        const std::string& nm = s->seg_name[k];
        long c = -1;   // the set's chrom, byte-equal
        {
            const uint64_t c8 = sid_regions_c8(nm.data(), nm.size());
            for (size_t q = 0; q < r->name.size() && c < 0; ++q)
                if (r->c8[q] == c8 && r->name[q] == nm) c = (long)q;
        }
        for (; i < run_end; ++i) {
            if (c < 0) continue;
            const long j = interval_of(r, (size_t)c, s->pos[i]);
            if (j < 0) continue;
            const uint16_t* cn = s->counts.data() + 4 * i;
            const uint8_t code = code_all[i];
            const bool rec = !(code & SID_CODE_DROPPED), het = rec && (code & SID_CODE_HET);
            sid_rs_sum& t = table[(size_t)j];
            t.sites += 1, t.depth += (uint64_t)cn[0] + cn[1] + cn[2] + cn[3], t.het += het, t.hom += rec && !het;
        }
    }
    return sid_rs_export(r, table, true, out, n);
}

extern "C" int sid_region_stats_merge(const sid_region_row* a, const sid_region_row* b, size_t n, sid_region_row** out)
{
    if (!out) return SID_EINVAL;
    *out = nullptr;
    if (n && (!a || !b)) return SID_EINVAL;
    size_t nb = 0;
    for (size_t k = 0; k < n; ++k) {
        if (a[k].chrom_len != b[k].chrom_len || a[k].start != b[k].start || a[k].end != b[k].end) return SID_EINVAL;
        if (a[k].chrom_len && (!a[k].chrom || !b[k].chrom || std::memcmp(a[k].chrom, b[k].chrom, a[k].chrom_len) != 0))
            return SID_EINVAL;
        nb += a[k].chrom_len;
    }
    char* names = nullptr;
    sid_region_row* rows = alloc_rows(n, nb, &names);
    if (!rows) return SID_ENOMEM;
    size_t at = 0;
    for (size_t k = 0; k < n; ++k) {
        sid_region_row& o = rows[k];
        o = a[k];
        if (a[k].chrom_len) std::memcpy(names + at, a[k].chrom, a[k].chrom_len);
        o.chrom = names + at;
        at += a[k].chrom_len;
        o.sites += b[k].sites, o.depth += b[k].depth, o.records += b[k].records, o.het += b[k].het, o.hom += b[k].hom;
    }
    *out = rows;
    return SID_OK;
}

extern "C" int sid_region_stats_format(const sid_region_row* rows, size_t n, int with_header, char* buf, size_t cap,
                                       size_t* len)
{
    static const char header[] = "chrom,start,end,sites,depth,records,het,hom\n";
    if (!len || (n && !rows)) return SID_EINVAL;
    size_t at = 0;
    auto put = [&](const char* p, size_t m) {
        if (m && buf && at + m <= cap) std::memcpy(buf + at, p, m);
        at += m;
    };
    if (with_header) put(header, sizeof header - 1);
    char line[7 * 24 + 8];
    for (size_t k = 0; k < n; ++k) {
        const sid_region_row& r = rows[k];
        if (r.chrom_len && !r.chrom) return SID_EINVAL;
        put(r.chrom, r.chrom_len);
        size_t w = 0;
        line[w++] = ',';
        w += sid_put_i64(r.start, line + w);
        line[w++] = ',';
        w += sid_put_i64(r.end, line + w);
        for (uint64_t v : {r.sites, r.depth, r.records, r.het, r.hom}) {
            line[w++] = ',';
            w += sid_put_u64(v, line + w);
        }
        line[w++] = '\n';
        put(line, w);
    }
    *len = at;
    return (buf && at <= cap) ? SID_OK : SID_ENOMEM;
}
