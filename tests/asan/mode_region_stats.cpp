// sid_asan region_stats CORPUS — region_stats.cpp, regions.cpp and parse.cpp
// under ASan + UBSan (tests/test_region_stats_asan.py; TEST INFRASTRUCTURE, CPU
// only).
//
// CORPUS is a sequence of cases, each opened by its region set:
//   "B <bytes>", then <bytes> bytes of BED text and a newline:
//   sid_regions_from_bed (a BED that does not parse: "<rc> 0" for the case that
//   follows).  Then one of
//   "I": the set's intervals through sid_regions_interval, "<rc> <n>" and a
//   line "<chrom> <start> <end>" each, then sid_region_stats_valid's status;
//   "T <bytes> <sites> <begin> <end>", then <bytes> bytes of pileup text, a
//   newline and a line of <sites> codes: sid_parse_text, then
//   sid_region_stats_host over sites [begin, end);
//   "M <bytes> <sites> <cut> <spoil>": likewise, the rows of [0, cut) and
//   [cut, sites) through sid_region_stats_merge; spoil 1 changes a key of the
//   second list first (SID_EINVAL);
//   "C <chunks>", then per chunk a line "R <rows>" and per row a line "<idx>
//   <sites> <het> <hom> <depth>": the chunks' rows as the device hands them
//   back, through sid_rs_check, sid_rs_add and sid_rs_export (a chunk that
//   fails the check: "7 0").
// Each prints "<rc> <rows>", then the rows through sid_region_stats_format
// (sized, then into a block of exactly that size).  Every array is an
// exact-size heap block: a read or write past it is a report.  Exit status 3: a
// corpus format error; 4: the sizing protocol.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "harness.h"
#include "region_stats.h"
#include "sites.h"

static void print_rows(int rc, sid_region_row* rows, size_t n)
{
    std::printf("%d %zu\n", rc, rc == SID_OK ? n : (size_t)0);
    if (rc == SID_OK) {
        size_t need = 0;
        const int s = sid_region_stats_format(rows, n, 0, nullptr, 0, &need);
        if (s != SID_ENOMEM) std::exit(4);
        char* out = (char*)std::malloc(need ? need : 1);
        size_t len = 0;
        if (need && sid_region_stats_format(rows, n, 0, out, need - 1, &len) != SID_ENOMEM) std::exit(4);
        if (need && (sid_region_stats_format(rows, n, 0, out, need, &len) != SID_OK || len != need)) std::exit(4);
        std::fwrite(out, 1, need, stdout);
        std::free(out);
    }
    sid_region_stats_free(rows);
}

int mode_region_stats(const std::string& all)
{
    size_t p = 0;
    auto next_line = [&]() {
        size_t nl = all.find('\n', p);
        if (nl == std::string::npos) nl = all.size();
        std::string s = all.substr(p, nl - p);
        p = nl + 1;
        return s;
    };
    // <bytes> bytes at p as an exact-size block, and the newline behind them
    auto block = [&](unsigned long long len, char** out) {
        if (p + len > all.size()) return false;
        *out = (char*)std::malloc(len ? len : 1);
        if (len) std::memcpy(*out, all.data() + p, len);
        p += len + 1;
        return true;
    };
    auto codes = [&](unsigned long long n, uint8_t** out) {
        const std::string cl = next_line();
        *out = (uint8_t*)std::malloc(n ? n : 1);
        const char* q = cl.c_str();
        for (unsigned long long i = 0; i < n; ++i) {
            char* end = nullptr;
            (*out)[i] = (uint8_t)std::strtoul(q, &end, 10);
            if (end == q) return false;
            q = end;
        }
        return true;
    };
    while (p < all.size()) {
        const std::string bh = next_line();
        if (bh.empty()) continue;
        unsigned long long blen = 0;
        if (std::sscanf(bh.c_str(), "B %llu", &blen) != 1) return 3;
        char* bed = nullptr;
        if (!block(blen, &bed)) return 3;
        sid_regions* rg = nullptr;
        uint64_t bad = 0;
        const int brc = sid_regions_from_bed(bed, blen, &rg, &bad);
        std::free(bed);
        const std::string head = next_line();
        if (head.empty()) return 3;
        if (head[0] == 'I') {
            const size_t n = sid_regions_intervals(rg);
            std::printf("%d %zu\n", brc, n);
            for (size_t j = 0; j <= n && brc == SID_OK; ++j) {
                const char* c = nullptr;
                uint32_t cl = 0;
                int64_t s = 0, e = 0;
                const int rc = sid_regions_interval(rg, j, &c, &cl, &s, &e);
                if ((rc == SID_OK) != (j < n)) return 4;
                if (rc == SID_OK) std::printf("%.*s %lld %lld\n", (int)cl, c, (long long)s, (long long)e);
            }
            std::printf("%d\n", sid_region_stats_valid(rg));
        } else if (head[0] == 'T' || head[0] == 'M') {
            unsigned long long len = 0, n = 0, a = 0, b = 0;
            if (std::sscanf(head.c_str() + 1, " %llu %llu %llu %llu", &len, &n, &a, &b) != 4) return 3;
            char* text = nullptr;
            if (!block(len, &text)) return 3;
            uint8_t* code = nullptr;
            if (!codes(n, &code)) return 3;
            sid_sites* s = nullptr;
            uint64_t badl = 0;
            int rc = brc != SID_OK ? brc : sid_parse_text(text, len, 2, &s, &badl);
            sid_region_row* rows = nullptr;
            size_t nr = 0;
            if (rc == SID_OK && sid_sites_count(s) != n) return 3;
            if (rc == SID_OK && head[0] == 'T') {
                rc = sid_region_stats_host(rg, s, a, b, n ? code : nullptr, &rows, &nr);
            } else if (rc == SID_OK) {
                sid_region_row *ra = nullptr, *rb = nullptr;
                size_t na = 0, nb = 0;
                rc = sid_region_stats_host(rg, s, 0, a, n ? code : nullptr, &ra, &na);
                if (rc == SID_OK) rc = sid_region_stats_host(rg, s, a, n, n ? code : nullptr, &rb, &nb);
                if (rc == SID_OK && na != nb) return 4;
                if (rc == SID_OK && b && nb) rb[nb - 1].end += 1;   // (spoil: a key differs)
                if (rc == SID_OK) rc = sid_region_stats_merge(ra, rb, na, &rows);
                nr = na;
                sid_region_stats_free(ra);
                sid_region_stats_free(rb);
            }
            print_rows(rc, rows, nr);
            sid_sites_free(s);
            std::free(code);
            std::free(text);
        } else if (head[0] == 'C') {
            unsigned long long nc = 0;
            if (std::sscanf(head.c_str(), "C %llu", &nc) != 1) return 3;
            const size_t ni = sid_regions_intervals(rg);
            std::vector<sid_rs_sum> tab(ni);
            int rc = brc;
            for (unsigned long long c = 0; c < nc; ++c) {
                unsigned long long nr = 0;
                if (std::sscanf(next_line().c_str(), "R %llu", &nr) != 1) return 3;
                std::vector<sid_rs_row> ch;
                for (unsigned long long k = 0; k < nr; ++k) {
                    unsigned idx = 0, ns = 0, nh = 0, nm = 0;
                    unsigned long long d = 0;
                    if (std::sscanf(next_line().c_str(), "%u %u %u %u %llu", &idx, &ns, &nh, &nm, &d) != 5) return 3;
                    ch.push_back(sid_rs_row{d, idx, ns, nh, nm});
                }
                ch.shrink_to_fit();
                if (rc == SID_OK && !sid_rs_check(ch, ni)) rc = SID_ESTATE;
                if (rc == SID_OK) sid_rs_add(&tab, ch);
            }
            sid_region_row* rows = nullptr;
            size_t nr = 0;
            // (the names the set's own, or -- an odd number of chunks -- copied behind the rows)
            if (rc == SID_OK) rc = sid_rs_export(rg, tab, (nc & 1) != 0, &rows, &nr);
            print_rows(rc, rows, nr);
        } else {
            return 3;
        }
        sid_regions_free(rg);
    }
    return 0;
}
