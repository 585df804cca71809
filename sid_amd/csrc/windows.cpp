// windows.cpp — the windowed summary on the host (windows.h): the stitch of
// the chunks' row lists, the rows of the host path (sid_windows_host) and the
// CSV formatter (sid_windows_format).  Pure host code, no HIP call.
#include "windows.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "sites.h"

void sid_win_table::push(const char* chrom, uint32_t clen, int64_t wi, uint64_t sites, uint64_t records, uint64_t het)
{
    const int64_t start = wi * window;
    if (!rows.empty()) {
        sid_window& l = rows.back();
        const char* ln = names.data() + name_off.back();
        const bool same_chrom = l.chrom_len == clen && (clen == 0 || std::memcmp(ln, chrom, clen) == 0);
        if (same_chrom && l.start == start) {
            l.sites += sites, l.records += records, l.het += het, l.hom += records - het;
            return;
        }
        if (same_chrom) {   // (the chrom's bytes once per run of its rows)
            name_off.push_back(name_off.back());
            rows.push_back(sid_window{nullptr, clen, start, start + window, sites, records, het, records - het});
            return;
        }
    }
    name_off.push_back(names.size());
    names.append(chrom, clen);
    rows.push_back(sid_window{nullptr, clen, start, start + window, sites, records, het, records - het});
}

void sid_win_table::finish()
{
    for (size_t k = 0; k < rows.size(); ++k) rows[k].chrom = names.data() + name_off[k];
}

static const char* row_chrom(const sid_win_row& r, const char* names, char (&tmp)[8])
{
    if (r.clen > 8) return names + r.name;
    for (int k = 0; k < 8; ++k) tmp[k] = (char)(r.c8 >> (8 * k));
    return tmp;
}

void sid_win_stitch_push(sid_win_table* t, const sid_win_chunk& c)
{
    char tmp[8];
    for (const sid_win_row& r : c.rows)
        t->push(row_chrom(r, c.names.data(), tmp), r.clen, r.wi, r.sites, r.records, r.het);
}

int sid_win_export(const sid_win_table& t, sid_window** out, size_t* n)
{
    const size_t nr = t.rows.size();
    // one allocation: the rows, then the names (sid_windows_free frees the rows' pointer)
    char* mem = (char*)std::malloc(std::max<size_t>(nr * sizeof(sid_window) + t.names.size(), 1));
    if (!mem) return SID_ENOMEM;
    sid_window* rows = (sid_window*)mem;
    char* nm = mem + nr * sizeof(sid_window);
    if (!t.names.empty()) std::memcpy(nm, t.names.data(), t.names.size());
    for (size_t k = 0; k < nr; ++k) {
        rows[k] = t.rows[k];
        rows[k].chrom = nm + t.name_off[k];
    }
    *out = rows;
    *n = nr;
    return SID_OK;
}

extern "C" void sid_windows_free(sid_window* rows) { std::free(rows); }

extern "C" int sid_win_stitch_chunks(const sid_win_row* rows, const uint64_t* off, const char* names,
                                     const uint64_t* noff, size_t nchunks, int window, sid_window** out, size_t* n)
{
    if (!out || !n) return SID_EINVAL;
    *out = nullptr, *n = 0;
    if (window < 1) return SID_EINVAL;
    if (nchunks && (!off || !noff)) return SID_EINVAL;
    sid_win_table t;
    t.window = window;
    char tmp[8];
    for (size_t c = 0; c < nchunks; ++c) {
        if (off[c + 1] < off[c] || noff[c + 1] < noff[c]) return SID_EINVAL;
        if (off[c + 1] > off[c] && !rows) return SID_EINVAL;
        const uint64_t nb = noff[c + 1] - noff[c];
        for (uint64_t k = off[c]; k < off[c + 1]; ++k) {
            const sid_win_row& r = rows[k];
            if (r.clen > 8 && (!names || r.name > nb || r.clen > nb - r.name)) return SID_EINVAL;
            t.push(row_chrom(r, names ? names + noff[c] : nullptr, tmp), r.clen, r.wi, r.sites, r.records, r.het);
        }
    }
    return sid_win_export(t, out, n);
}

extern "C" int sid_windows_host(const sid_sites* s, size_t begin, size_t end, const uint8_t* code_all, int window,
                                sid_window** out, size_t* n)
{
    if (!out || !n) return SID_EINVAL;
    *out = nullptr, *n = 0;
    if (!s || begin > end || end > s->pos.size() || (end > begin && !code_all) || window < 1) return SID_EINVAL;
    sid_win_table t;
    t.window = window;
    size_t k = 0;   // the chromosome run holding `begin`
    {
        size_t lo = 0, hi = s->seg_start.size();
        while (lo + 1 < hi) {
            const size_t mid = (lo + hi) / 2;
            if (s->seg_start[mid] <= begin) lo = mid; else hi = mid;
        }
        k = lo;
    }
    for (size_t i = begin; i < end; ++i) {
        while (k + 1 < s->seg_start.size() && s->seg_start[k + 1] <= i) ++k;
        const std::string& nm = s->seg_name[k];
        const uint8_t c = code_all[i];
        const bool rec = !(c & SID_CODE_DROPPED);
        t.push(nm.data(), (uint32_t)nm.size(), sid_win_index(s->pos[i], window), 1, rec, rec && (c & SID_CODE_HET));
    }
    return sid_win_export(t, out, n);
}

// decimal digits of v at p; returns their number
static size_t put_i64(int64_t v, char* p)
{
    char tmp[24];
    size_t k = 0;
    uint64_t u = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    do tmp[k++] = (char)('0' + u % 10); while (u /= 10);
    size_t w = 0;
    if (v < 0) p[w++] = '-';
    while (k) p[w++] = tmp[--k];
    return w;
}
static size_t put_u64(uint64_t u, char* p)
{
    char tmp[24];
    size_t k = 0, w = 0;
    do tmp[k++] = (char)('0' + u % 10); while (u /= 10);
    while (k) p[w++] = tmp[--k];
    return w;
}

extern "C" int sid_windows_format(const sid_window* rows, size_t n, int with_header, char* buf, size_t cap, size_t* len)
{
    static const char header[] = "chrom,start,end,sites,records,het,hom\n";
    if (!len || (n && !rows)) return SID_EINVAL;
    size_t at = 0;
    auto put = [&](const char* p, size_t m) {
        if (m && buf && at + m <= cap) std::memcpy(buf + at, p, m);
        at += m;
    };
    if (with_header) put(header, sizeof header - 1);
    char line[6 * 24 + 8];
    for (size_t k = 0; k < n; ++k) {
        const sid_window& r = rows[k];
        if (r.chrom_len && !r.chrom) return SID_EINVAL;
        put(r.chrom, r.chrom_len);
        size_t w = 0;
        line[w++] = ',';
        w += put_i64(r.start, line + w);
        line[w++] = ',';
        w += put_i64(r.end, line + w);
        for (uint64_t v : {r.sites, r.records, r.het, r.hom}) {
            line[w++] = ',';
            w += put_u64(v, line + w);
        }
        line[w++] = '\n';
        put(line, w);
    }
    *len = at;
    return (buf && at <= cap) ? SID_OK : SID_ENOMEM;
}
