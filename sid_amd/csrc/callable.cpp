// callable.cpp — the callable runs on the host (callable.h): the stitch of the
// chunks' row lists, the rows of the host path (sid_callable_host), the join of
// two neighbouring row lists (sid_callable_join) and the BED formatter
// (sid_callable_format).  Pure host code, no HIP call.
#include "callable.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "sites.h"

void sid_call_table::push(const char* chrom, uint32_t clen, int64_t start, int64_t end, uint64_t het, bool join)
{
    const bool same = same_chrom(chrom, clen);
    if (join && open && same && rows.back().end == start) {
        rows.back().end = end, rows.back().het += het;
        return;
    }
    append(sid_callable_row{nullptr, clen, 0, start, end, het}, chrom, same);
}

void sid_call_table::finish() { sid_row_table::finish(); }   // (its own symbol, as push)

// one chunk's rows and edge bits into the table
static void push_chunk(sid_call_table* t, const sid_call_row* rows, size_t n, const char* names, uint32_t edge)
{
    if (!(edge & SID_CALL_HAS_SITE)) return;   // (transparent: the table's last site stays the last)
    char tmp[8];
    for (size_t k = 0; k < n; ++k) {
        const sid_call_row& r = rows[k];
        const int64_t start = (int64_t)r.pos - 1;
        t->push(sid_row_chrom(r, names, tmp), r.clen, start, start + (int64_t)r.sites, r.het,
                k == 0 && (edge & SID_CALL_OPEN_START));
        t->open = false;   // (a chunk's rows never join one another)
    }
    t->open = n && (edge & SID_CALL_OPEN_END);
}

void sid_call_stitch_push(sid_call_table* t, const sid_call_chunk& c)
{
    push_chunk(t, c.rows.data(), c.rows.size(), c.names.data(), c.edge);
}

int sid_call_export(const sid_call_table& t, sid_callable_row** out, size_t* n) { return t.export_rows(out, n); }

extern "C" void sid_callable_free(sid_callable_row* rows) { std::free(rows); }

extern "C" int sid_callable_stitch_chunks(const sid_call_row* rows, const uint64_t* off, const char* names,
                                          const uint64_t* noff, const uint32_t* edge, size_t nchunks,
                                          sid_callable_row** out, size_t* n)
{
    if (!out || !n) return SID_EINVAL;
    *out = nullptr, *n = 0;
    if (nchunks && (!off || !noff || !edge)) return SID_EINVAL;
    sid_call_table t;
    for (size_t c = 0; c < nchunks; ++c) {
        if (off[c + 1] < off[c] || noff[c + 1] < noff[c]) return SID_EINVAL;
        const uint64_t nr = off[c + 1] - off[c], nb = noff[c + 1] - noff[c];
        if (nr && !rows) return SID_EINVAL;
        if (edge[c] & ~7u) return SID_EINVAL;
        if (!(edge[c] & SID_CALL_HAS_SITE) && (nr || edge[c])) return SID_EINVAL;
        if (!nr && (edge[c] & (SID_CALL_OPEN_START | SID_CALL_OPEN_END))) return SID_EINVAL;
        for (uint64_t k = off[c]; k < off[c + 1]; ++k) {
            const sid_call_row& r = rows[k];
            if (r.clen > 8 && (!names || r.name > nb || r.clen > nb - r.name)) return SID_EINVAL;
            if (r.pos < 1 || r.sites == 0 || r.het > r.sites) return SID_EINVAL;
        }
        push_chunk(&t, rows ? rows + off[c] : nullptr, nr, names ? names + noff[c] : nullptr, edge[c]);
    }
    return sid_call_export(t, out, n);
}

extern "C" int sid_callable_host(const sid_sites* s, size_t begin, size_t end, const uint8_t* code_all, int min,
                                 int max, sid_callable_row** out, size_t* n)
{
    if (!out || !n) return SID_EINVAL;
    *out = nullptr, *n = 0;
    if (min < 0 || min > SID_DEPTH_MAX || (max != 0 && (max < min || max > SID_DEPTH_MAX))) return SID_EINVAL;
    if (!s || begin > end || end > s->pos.size() || s->counts.size() != 4 * s->pos.size()) return SID_EINVAL;
    if (end > begin && !code_all) return SID_EINVAL;
    sid_call_table t;
    size_t k = sid_seg_of(s->seg_start, begin);
    for (size_t i = begin; i < end; ++i) {
        while (k + 1 < s->seg_start.size() && s->seg_start[k + 1] <= i) ++k;
        const std::string& nm = s->seg_name[k];
        const uint16_t* c = s->counts.data() + 4 * i;
        const uint32_t d = (uint32_t)c[0] + c[1] + c[2] + c[3];
        const uint8_t code = code_all[i];
        const int64_t pos = s->pos[i];
        const bool callable = !(code & SID_CODE_DROPPED) && d >= 1 && d >= (uint32_t)min &&
                              (max == 0 || d <= (uint32_t)max) && pos >= 1;
        // (push joins on chrom and start == the last row's end: pos == the previous pos + 1, in 64 bits)
        if (callable) t.push(nm.data(), (uint32_t)nm.size(), pos - 1, pos, (code & SID_CODE_HET) != 0, true);
        t.open = callable;
    }
    return sid_call_export(t, out, n);
}

extern "C" int sid_callable_join(const sid_callable_row* a, size_t na, int a_open_end, const sid_callable_row* b,
                                 size_t nb, int b_open_start, sid_callable_row** out, size_t* n)
{
    if (!out || !n) return SID_EINVAL;
    *out = nullptr, *n = 0;
    if ((na && !a) || (nb && !b)) return SID_EINVAL;
    for (size_t k = 0; k < na; ++k)
        if (a[k].chrom_len && !a[k].chrom) return SID_EINVAL;
    for (size_t k = 0; k < nb; ++k)
        if (b[k].chrom_len && !b[k].chrom) return SID_EINVAL;
    sid_call_table t;
    for (size_t k = 0; k < na; ++k) t.push(a[k].chrom, a[k].chrom_len, a[k].start, a[k].end, a[k].het, false);
    t.open = na && a_open_end;
    for (size_t k = 0; k < nb; ++k) {
        t.push(b[k].chrom, b[k].chrom_len, b[k].start, b[k].end, b[k].het, k == 0 && b_open_start);
        t.open = false;
    }
    return sid_call_export(t, out, n);
}

extern "C" int sid_callable_format(const sid_callable_row* rows, size_t n, char* buf, size_t cap, size_t* len)
{
    if (!len || (n && !rows)) return SID_EINVAL;
    size_t at = 0;
    auto put = [&](const char* p, size_t m) {
        if (m && buf && at + m <= cap) std::memcpy(buf + at, p, m);
        at += m;
    };
    char line[3 * 24 + 8];
    for (size_t k = 0; k < n; ++k) {
        const sid_callable_row& r = rows[k];
        if (r.chrom_len && !r.chrom) return SID_EINVAL;
        put(r.chrom, r.chrom_len);
        size_t w = 0;
        line[w++] = '\t';
        w += sid_put_i64(r.start, line + w);
        line[w++] = '\t';
        w += sid_put_i64(r.end, line + w);
        line[w++] = '\t';
        w += sid_put_u64(r.het, line + w);
        line[w++] = '\n';
        put(line, w);
    }
    *len = at;
    return (buf && at <= cap) ? SID_OK : SID_ENOMEM;
}
