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
    const bool same = same_chrom(chrom, clen);
    if (same && rows.back().start == start) {
        sid_window& l = rows.back();
        l.sites += sites, l.records += records, l.het += het, l.hom += records - het;
        return;
    }
    append(sid_window{nullptr, clen, start, start + window, sites, records, het, records - het}, chrom, same);
}

void sid_win_table::finish() { sid_row_table::finish(); }   // (its own symbol, as push)

void sid_win_stitch_push(sid_win_table* t, const sid_win_chunk& c)
{
    char tmp[8];
    for (const sid_win_row& r : c.rows)
        t->push(sid_row_chrom(r, c.names.data(), tmp), r.clen, r.wi, r.sites, r.records, r.het);
}

int sid_win_export(const sid_win_table& t, sid_window** out, size_t* n) { return t.export_rows(out, n); }

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
            t.push(sid_row_chrom(r, names ? names + noff[c] : nullptr, tmp), r.clen, r.wi, r.sites, r.records, r.het);
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
    size_t k = sid_seg_of(s->seg_start, begin);
    for (size_t i = begin; i < end; ++i) {
        while (k + 1 < s->seg_start.size() && s->seg_start[k + 1] <= i) ++k;
        const std::string& nm = s->seg_name[k];
        const uint8_t c = code_all[i];
        const bool rec = !(c & SID_CODE_DROPPED);
        t.push(nm.data(), (uint32_t)nm.size(), sid_win_index(s->pos[i], window), 1, rec, rec && (c & SID_CODE_HET));
    }
    return sid_win_export(t, out, n);
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
        w += sid_put_i64(r.start, line + w);
        line[w++] = ',';
        w += sid_put_i64(r.end, line + w);
        for (uint64_t v : {r.sites, r.records, r.het, r.hom}) {
            line[w++] = ',';
            w += sid_put_u64(v, line + w);
        }
        line[w++] = '\n';
        put(line, w);
    }
    *len = at;
    return (buf && at <= cap) ? SID_OK : SID_ENOMEM;
}
