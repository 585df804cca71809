// depth_hist.cpp — the depth histogram on the host (depth_hist.h): the sum of
// the chunks' rows, the rows of the host path (sid_depth_hist_host), the merge
// of two row sets and the CSV formatter.  Pure host code, no HIP call.
#include "depth_hist.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

#include "rowtable.h"
#include "sites.h"

bool sid_dh_sort(std::vector<sid_dh_row>* rows)
{
    std::sort(rows->begin(), rows->end(), [](const sid_dh_row& a, const sid_dh_row& b) { return a.depth < b.depth; });
    for (size_t k = 0; k < rows->size(); ++k) {
        if ((*rows)[k].depth >= SID_DH_BINS) return false;
        if (k && (*rows)[k - 1].depth == (*rows)[k].depth) return false;
    }
    return true;
}

static sid_depth_row make_row(uint32_t depth, uint64_t sites, uint64_t het, uint64_t hom)
{
    return sid_depth_row{sites, het + hom, het, hom, depth, 0};
}

static void add_row(sid_depth_row& d, const sid_depth_row& s)
{
    d.sites += s.sites, d.records += s.records, d.het += s.het, d.hom += s.hom;
}

// a, b sorted by depth: their sum, sorted
static std::vector<sid_depth_row> merge_rows(const sid_depth_row* a, size_t na, const sid_depth_row* b, size_t nb)
{
    std::vector<sid_depth_row> out;
    out.reserve(na + nb);
    size_t i = 0, j = 0;
    while (i < na || j < nb) {
        if (j == nb || (i < na && a[i].depth < b[j].depth)) {
            out.push_back(a[i++]);
        } else if (i == na || b[j].depth < a[i].depth) {
            out.push_back(b[j++]);
        } else {
            out.push_back(a[i++]);
            add_row(out.back(), b[j++]);
        }
        out.back().pad = 0;
    }
    return out;
}

void sid_dh_add(std::vector<sid_depth_row>* table, const std::vector<sid_dh_row>& chunk)
{
    if (chunk.empty()) return;
    std::vector<sid_depth_row> c;
    c.reserve(chunk.size());
    for (const sid_dh_row& r : chunk) c.push_back(make_row(r.depth, r.sites, r.het, r.hom));
    *table = merge_rows(table->data(), table->size(), c.data(), c.size());
}

int sid_dh_export(const std::vector<sid_depth_row>& t, sid_depth_row** out, size_t* n)
{
    sid_depth_row* rows = (sid_depth_row*)std::malloc(std::max<size_t>(t.size() * sizeof(sid_depth_row), 1));
    if (!rows) return SID_ENOMEM;
    if (!t.empty()) std::memcpy(rows, t.data(), t.size() * sizeof(sid_depth_row));
    *out = rows;
    *n = t.size();
    return SID_OK;
}

extern "C" void sid_depth_hist_free(sid_depth_row* rows) { std::free(rows); }

extern "C" int sid_depth_hist_host(const sid_sites* s, size_t begin, size_t end, const uint8_t* code_all,
                                   sid_depth_row** out, size_t* n)
{
    if (!out || !n) return SID_EINVAL;
    *out = nullptr, *n = 0;
    if (!s || begin > end || end > s->pos.size() || s->counts.size() != 4 * s->pos.size()) return SID_EINVAL;
    if (end > begin && !code_all) return SID_EINVAL;
    std::map<uint32_t, sid_depth_row> bins;   // (the host path: a few hundred depths)
    for (size_t i = begin; i < end; ++i) {
        const uint16_t* c = s->counts.data() + 4 * i;
        const uint32_t d = (uint32_t)c[0] + c[1] + c[2] + c[3];
        const uint8_t code = code_all[i];
        const bool rec = !(code & SID_CODE_DROPPED), het = rec && (code & SID_CODE_HET);
        sid_depth_row& r = bins.emplace(d, make_row(d, 0, 0, 0)).first->second;
        r.sites += 1, r.records += rec, r.het += het, r.hom += rec && !het;
    }
    std::vector<sid_depth_row> t;
    t.reserve(bins.size());
    for (const auto& kv : bins) t.push_back(kv.second);
    return sid_dh_export(t, out, n);
}

extern "C" int sid_depth_hist_merge(const sid_depth_row* a, size_t na, const sid_depth_row* b, size_t nb,
                                    sid_depth_row** out, size_t* n)
{
    if (!out || !n) return SID_EINVAL;
    *out = nullptr, *n = 0;
    if ((na && !a) || (nb && !b)) return SID_EINVAL;
    for (size_t k = 1; k < na; ++k)
        if (a[k - 1].depth >= a[k].depth) return SID_EINVAL;
    for (size_t k = 1; k < nb; ++k)
        if (b[k - 1].depth >= b[k].depth) return SID_EINVAL;
    return sid_dh_export(merge_rows(a, na, b, nb), out, n);
}

extern "C" int sid_depth_hist_format(const sid_depth_row* rows, size_t n, int with_header, char* buf, size_t cap,
                                     size_t* len)
{
    static const char header[] = "depth,sites,records,het,hom\n";
    if (!len || (n && !rows)) return SID_EINVAL;
    size_t at = 0;
    auto put = [&](const char* p, size_t m) {
        if (m && buf && at + m <= cap) std::memcpy(buf + at, p, m);
        at += m;
    };
    if (with_header) put(header, sizeof header - 1);
    char line[5 * 24 + 8];
    for (size_t k = 0; k < n; ++k) {
        const sid_depth_row& r = rows[k];
        size_t w = sid_put_u64(r.depth, line);
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
