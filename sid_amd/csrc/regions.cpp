// regions.cpp — region sets (sid_regions_*, --regions): the BED parser, the
// per-chrom merge, the host membership test and sid_regions_mark (the host
// formatter's selection, as sid_select_mark is the label selection's).
//
// The reference pipeline filters its CSV by interval after the run
// (filter-exon-sites.sh, one chromosome per process in parallel-run-sid.sh);
// here the set selects the records before they are formatted.  A site is
// inside when its chrom equals a set chrom byte for byte and start < pos <=
// end, pos being the integer the record prints (call.hpp:25).
//
// No HIP in this file: it builds into a stand-alone sanitized program
// (tests/asan).  The device table is uploaded by capi.cpp.
#include <algorithm>
#include <cstring>
#include <map>
#include <new>

#include "regions.h"
#include "sites.h"

namespace {
constexpr int64_t POS_MAX = 2147483647;   // 2^31 - 1

struct Raw {
    int32_t start, end;
};
struct RawChrom {
    std::vector<Raw> iv;
    uint64_t first = UINT64_MAX;   // the source index of its first non-empty interval
};
using RawSet = std::map<std::string, RawChrom>;

void raw_add(RawSet& raw, std::string chrom, Raw x, uint64_t at)
{
    RawChrom& c = raw[std::move(chrom)];
    c.iv.push_back(x);
    if (x.start < x.end && c.first == UINT64_MAX) c.first = at;
}

bool is_sep(char c) { return c == ' ' || c == '\t'; }

// decimal digits only (no sign, no blank); saturates far above POS_MAX
bool parse_dec(const char* b, const char* e, uint64_t* out)
{
    if (b == e) return false;
    uint64_t v = 0;
    for (const char* p = b; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        v = v > (UINT64_MAX - 9) / 10 ? UINT64_MAX : v * 10 + (uint64_t)(*p - '0');
    }
    *out = v;
    return true;
}

bool key_less(uint64_t a8, size_t alen, const char* a, uint64_t b8, size_t blen, const char* b)
{
    if (a8 != b8) return a8 < b8;
    if (alen != blen) return alen < blen;
    return std::memcmp(a, b, alen) < 0;
}

sid_regions* build(RawSet& raw)
{
    sid_regions* r = new sid_regions();
    struct Ent {
        uint64_t c8;
        const std::string* name;
        std::vector<Raw>* iv;
        uint64_t first;
    };
    std::vector<Ent> ents;
    for (auto& kv : raw)
        ents.push_back(Ent{sid_regions_c8(kv.first.data(), kv.first.size()), &kv.first, &kv.second.iv, kv.second.first});
    std::sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) {
        return key_less(a.c8, a.name->size(), a.name->data(), b.c8, b.name->size(), b.name->data());
    });
    std::vector<std::pair<uint64_t, uint32_t>> by;   // (first source index, chrom)
    for (const Ent& en : ents) {
        std::vector<Raw>& v = *en.iv;
        std::sort(v.begin(), v.end(), [](const Raw& a, const Raw& b) { return a.start < b.start; });
        const size_t first = r->start.size();
        for (const Raw& x : v) {
            if (x.start >= x.end) continue;   // an empty interval holds nothing
            if (r->start.size() > first && x.start <= r->end.back())   // overlapping, nested or adjacent
                r->end.back() = std::max(r->end.back(), x.end);
            else
                r->start.push_back(x.start), r->end.push_back(x.end);
        }
        if (r->start.size() == first) continue;   // a chrom without a position
        r->name.push_back(*en.name);
        r->c8.push_back(en.c8);
        r->ibeg.push_back((uint32_t)first);
        by.push_back({en.first, (uint32_t)r->name.size() - 1});
    }
    r->ibeg.push_back((uint32_t)r->start.size());
    std::sort(by.begin(), by.end());   // the source order: the kept chroms by their first non-empty interval
    r->rank.assign(r->name.size(), 0);
    r->row.reserve(r->start.size());
    for (size_t q = 0; q < by.size(); ++q) {
        const uint32_t k = by[q].second;
        r->rank[k] = (uint32_t)q;
        for (uint32_t j = r->ibeg[k]; j < r->ibeg[k + 1]; ++j) r->row.push_back(j);
    }
    return r;
}

// index of the chrom, or -1
long find_chrom(const sid_regions* r, const char* chrom, size_t n)
{
    const uint64_t c8 = sid_regions_c8(chrom, n);
    size_t lo = 0, hi = r->name.size();
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (key_less(r->c8[mid], r->name[mid].size(), r->name[mid].data(), c8, n, chrom)) lo = mid + 1;
        else hi = mid;
    }
    if (lo < r->name.size() && r->name[lo].size() == n && std::memcmp(r->name[lo].data(), chrom, n) == 0)
        return (long)lo;
    return -1;
}

bool chrom_has(const sid_regions* r, long k, int32_t pos)
{
    const int32_t* s0 = r->start.data() + r->ibeg[k];
    const int32_t* s1 = r->start.data() + r->ibeg[k + 1];
    const int32_t* p = std::lower_bound(s0, s1, pos);   // first start >= pos
    if (p == s0) return false;
    return pos <= r->end[(size_t)(p - 1 - r->start.data())];   // the last start < pos
}
}  // namespace

uint64_t sid_regions_c8(const char* s, size_t n)
{
    uint64_t v = 0;
    for (size_t k = 0; k < n && k < 8; ++k) v |= (uint64_t)(unsigned char)s[k] << (8 * k);
    return v;
}

extern "C" int sid_regions_from_bed(const char* text, size_t len, sid_regions** out, uint64_t* err_line)
{
    if (!out || (len && !text)) return SID_EINVAL;
    *out = nullptr;
    if (err_line) *err_line = 0;
    RawSet raw;
    uint64_t line = 0;
    const char* p = text;
    const char* const te = text + len;
    while (p < te) {
        const char* le = (const char*)std::memchr(p, '\n', (size_t)(te - p));
        if (!le) le = te;
        ++line;
        const char* b = p;
        p = le < te ? le + 1 : te;
        const size_t ll = (size_t)(le - b);
        if (ll == 0 || b[0] == '#' || (ll >= 5 && std::memcmp(b, "track", 5) == 0) ||
            (ll >= 7 && std::memcmp(b, "browser", 7) == 0))
            continue;
        const char *fb[3], *fe[3];
        int nf = 0;
        for (const char* q = b; q < le;) {
            while (q < le && is_sep(*q)) ++q;
            if (q == le) break;
            const char* t = q;
            while (q < le && !is_sep(*q)) ++q;
            if (nf < 3) fb[nf] = t, fe[nf] = q;
            ++nf;
        }
        uint64_t s = 0, e = (uint64_t)POS_MAX;
        bool ok = nf == 1 || nf >= 3;
        if (ok && nf >= 3) ok = parse_dec(fb[1], fe[1], &s) && parse_dec(fb[2], fe[2], &e) && s <= e;
        if (!ok) {
            if (err_line) *err_line = line;
            return SID_EINVAL;
        }
        s = std::min<uint64_t>(s, (uint64_t)POS_MAX);
        e = std::min<uint64_t>(e, (uint64_t)POS_MAX);
        raw_add(raw, std::string(fb[0], fe[0]), Raw{(int32_t)s, (int32_t)e}, line);
    }
    *out = build(raw);
    return SID_OK;
}

extern "C" int sid_regions_from_intervals(const char* const* chrom, const int32_t* start, const int32_t* end, size_t n,
                                          sid_regions** out)
{
    if (!out || (n && (!chrom || !start || !end))) return SID_EINVAL;
    *out = nullptr;
    RawSet raw;
    for (size_t i = 0; i < n; ++i) {
        if (!chrom[i] || !chrom[i][0] || start[i] < 0 || start[i] > end[i]) return SID_EINVAL;
        for (const char* q = chrom[i]; *q; ++q)
            if (is_sep(*q) || *q == '\n') return SID_EINVAL;   // the pileup's separators: no chrom holds one
        raw_add(raw, chrom[i], Raw{start[i], end[i]}, i);
    }
    *out = build(raw);
    return SID_OK;
}

extern "C" size_t sid_regions_intervals(const sid_regions* r) { return r ? r->start.size() : 0; }
extern "C" size_t sid_regions_chroms(const sid_regions* r) { return r ? r->name.size() : 0; }

extern "C" int sid_regions_contains(const sid_regions* r, const char* chrom, size_t chrom_len, int32_t pos)
{
    if (!r || (chrom_len && !chrom)) return 0;
    const long k = find_chrom(r, chrom, chrom_len);
    return k >= 0 && chrom_has(r, k, pos) ? 1 : 0;
}

extern "C" int sid_regions_interval(const sid_regions* r, size_t j, const char** chrom, uint32_t* chrom_len,
                                    int64_t* start, int64_t* end)
{
    if (!r || j >= r->row.size()) return SID_EINVAL;
    const uint32_t t = r->row[j];
    const size_t k = (size_t)(std::upper_bound(r->ibeg.begin(), r->ibeg.end(), t) - r->ibeg.begin()) - 1;
    if (chrom) *chrom = r->name[k].data();
    if (chrom_len) *chrom_len = (uint32_t)r->name[k].size();
    if (start) *start = r->start[t];
    if (end) *end = r->end[t];
    return SID_OK;
}

extern "C" void sid_regions_free(sid_regions* r) { delete r; }

// --regions on the host path: the sites outside get the "no record" bit, which
// sid_format_csv skips (r == NULL: every site is inside, nothing changes)
extern "C" int sid_regions_mark(const sid_regions* r, const sid_sites* s, size_t begin, size_t end, uint8_t* code)
{
    if (!s || begin > end || end > s->pos.size() || (end > begin && !code)) return SID_EINVAL;
    if (!r || begin == end) return SID_OK;
    size_t k = 0;   // the chromosome run holding `begin`
    {
        size_t lo = 0, hi = s->seg_start.size();
        while (lo + 1 < hi) {
            const size_t mid = (lo + hi) / 2;
            if (s->seg_start[mid] <= begin) lo = mid; else hi = mid;
        }
        k = lo;
    }
    for (size_t i = begin; i < end;) {
        while (k + 1 < s->seg_start.size() && s->seg_start[k + 1] <= i) ++k;
        const size_t run_end = std::min<size_t>(end, k + 1 < s->seg_start.size() ? s->seg_start[k + 1] : end);
        const std::string& nm = s->seg_name[k];
        const long c = find_chrom(r, nm.data(), nm.size());
        for (; i < run_end; ++i)
            if (c < 0 || !chrom_has(r, c, s->pos[i])) code[i] |= SID_CODE_DROPPED;
    }
    return SID_OK;
}

void sid_regions_flatten(const sid_regions* r, std::vector<char>& buf, sid_regions_layout* L)
{
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t nc = r->name.size(), ni = r->start.size();
    size_t nb = 0;
    for (const auto& n : r->name) nb += n.size();
    L->nc = (uint32_t)nc;
    L->ni = (uint32_t)ni;
    L->c8 = 0;
    L->clen = up(L->c8 + 8 * nc);
    L->noff = up(L->clen + 4 * nc);
    L->ibeg = up(L->noff + 4 * nc);
    L->start = up(L->ibeg + 4 * (nc + 1));
    L->end = up(L->start + 4 * ni);
    L->names = up(L->end + 4 * ni);
    L->bytes = up(L->names + nb + 16);
    buf.assign(L->bytes, 0);
    uint32_t off = 0;
    for (size_t k = 0; k < nc; ++k) {
        const uint32_t cl = (uint32_t)r->name[k].size();
        std::memcpy(&buf[L->c8 + 8 * k], &r->c8[k], 8);
        std::memcpy(&buf[L->clen + 4 * k], &cl, 4);
        std::memcpy(&buf[L->noff + 4 * k], &off, 4);
        std::memcpy(&buf[L->names + off], r->name[k].data(), cl);
        off += cl;
    }
    std::memcpy(&buf[L->ibeg], r->ibeg.data(), 4 * (nc + 1));
    if (ni) {
        std::memcpy(&buf[L->start], r->start.data(), 4 * ni);
        std::memcpy(&buf[L->end], r->end.data(), 4 * ni);
    }
}
