// sid_asan callable CORPUS — callable.cpp (and rowtable.h, parse.cpp) under
// ASan + UBSan (tests/test_callable_asan.py; TEST INFRASTRUCTURE, CPU only).
//
// CORPUS is a sequence of cases.
//   "H <min> <max> <sites> <begin> <end>", then per site a line "<chrom> <pos>
//   <code> <depth>": sid_callable_host over sites [begin, end) of hand-made
//   sites, the depth spread over the four counts.
//   "T <min> <max> <bytes> <sites>", then <bytes> bytes of pileup text, a
//   newline and a line of <sites> codes: sid_parse_text, then sid_callable_host
//   over the parser's sites (a text that does not parse: "<rc> 0").
//   "S <chunks>", then per chunk a line "C <rows> <edge>" and per row a line
//   "<chrom> <pos> <sites> <het>": the rows in the device's layout (chroms over
//   8 bytes in the chunk's name blob), sid_callable_stitch_chunks.
//   "J <na> <a_open_end> <nb> <b_open_start>", then na + nb lines "<chrom>
//   <start> <end> <het>": sid_callable_join.
// Each prints "<rc> <rows>", then the rows through sid_callable_format (sized,
// then into a block of exactly that size).  Every array is an exact-size heap
// block: a read or write past it is a report.  Exit status 3: a corpus format
// error; 4: the sizing protocol.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "callable.h"
#include "harness.h"
#include "sites.h"

static void print_rows(int rc, sid_callable_row* rows, size_t n)
{
    std::printf("%d %zu\n", rc, n);
    if (rc == SID_OK) {
        size_t need = 0;
        const int s = sid_callable_format(rows, n, nullptr, 0, &need);
        if (s != SID_ENOMEM) std::exit(4);
        char* out = (char*)std::malloc(need ? need : 1);
        size_t len = 0;
        if (need && sid_callable_format(rows, n, out, need - 1, &len) != SID_ENOMEM) std::exit(4);
        if (sid_callable_format(rows, n, out, need, &len) != SID_OK || len != need) std::exit(4);
        std::fwrite(out, 1, len, stdout);
        std::free(out);
    }
    sid_callable_free(rows);
}

// rows "<chrom> <start> <end> <het>" as an exact-size block of sid_callable_row, the chroms exact-size blocks too
struct RowList {
    sid_callable_row* rows = nullptr;
    std::vector<char*> names;
    size_t n = 0;
    ~RowList()
    {
        for (char* p : names) std::free(p);
        std::free(rows);
    }
};

int mode_callable(const std::string& all)
{
    size_t p = 0;
    auto next_line = [&]() {
        size_t nl = all.find('\n', p);
        if (nl == std::string::npos) nl = all.size();
        std::string s = all.substr(p, nl - p);
        p = nl + 1;
        return s;
    };
    char name[4096];
    while (p < all.size()) {
        const std::string head = next_line();
        if (head.empty()) continue;
        if (head[0] == 'H') {
            int lo = 0, hi = 0;
            unsigned long long n = 0, b = 0, e = 0;
            if (std::sscanf(head.c_str(), "H %d %d %llu %llu %llu", &lo, &hi, &n, &b, &e) != 5) return 3;
            sid_sites s;
            uint8_t* code = (uint8_t*)std::malloc(n ? n : 1);
            for (unsigned long long i = 0; i < n; ++i) {
                long long pos = 0;
                unsigned c = 0, d = 0;
                if (std::sscanf(next_line().c_str(), "%4095s %lld %u %u", name, &pos, &c, &d) != 4) return 3;
                if (s.seg_name.empty() || s.seg_name.back() != name) {
                    s.seg_start.push_back(i);
                    s.seg_name.push_back(name);
                }
                s.pos.push_back((int32_t)pos);
                for (int k = 0; k < 4; ++k) {
                    const unsigned x = d < 65535u ? d : 65535u;
                    s.counts.push_back((uint16_t)x);
                    d -= x;
                }
                code[i] = (uint8_t)c;
            }
            s.pos.shrink_to_fit();
            s.counts.shrink_to_fit();
            sid_callable_row* rows = nullptr;
            size_t nr = 0;
            const int rc = sid_callable_host(&s, b, e, n ? code : nullptr, lo, hi, &rows, &nr);
            print_rows(rc, rows, nr);
            std::free(code);
        } else if (head[0] == 'T') {
            int lo = 0, hi = 0;
            unsigned long long len = 0, n = 0;
            if (std::sscanf(head.c_str(), "T %d %d %llu %llu", &lo, &hi, &len, &n) != 4) return 3;
            if (p + len > all.size()) return 3;
            char* text = (char*)std::malloc(len ? len : 1);
            if (len) std::memcpy(text, all.data() + p, len);
            p += len + 1;
            const std::string cl = next_line();
            uint8_t* code = (uint8_t*)std::malloc(n ? n : 1);
            const char* q = cl.c_str();
            for (unsigned long long i = 0; i < n; ++i) {
                char* end = nullptr;
                code[i] = (uint8_t)std::strtoul(q, &end, 10);
                if (end == q) return 3;
                q = end;
            }
            sid_sites* s = nullptr;
            uint64_t bad = 0;
            int rc = sid_parse_text(text, len, 2, &s, &bad);
            sid_callable_row* rows = nullptr;
            size_t nr = 0;
            if (rc == SID_OK) {
                if (sid_sites_count(s) != n) return 3;
                rc = sid_callable_host(s, 0, n, n ? code : nullptr, lo, hi, &rows, &nr);
            }
            print_rows(rc, rows, nr);
            sid_sites_free(s);
            std::free(code);
            std::free(text);
        } else if (head[0] == 'S') {
            unsigned long long nc = 0;
            if (std::sscanf(head.c_str(), "S %llu", &nc) != 1) return 3;
            std::vector<sid_call_row> rv;
            std::string names;
            uint64_t* off = (uint64_t*)std::malloc((nc + 1) * 8);
            uint64_t* noff = (uint64_t*)std::malloc((nc + 1) * 8);
            uint32_t* edge = (uint32_t*)std::malloc(nc ? nc * 4 : 1);
            off[0] = noff[0] = 0;
            for (unsigned long long c = 0; c < nc; ++c) {
                unsigned long long nr = 0;
                unsigned eg = 0;
                if (std::sscanf(next_line().c_str(), "C %llu %u", &nr, &eg) != 2) return 3;
                edge[c] = eg;
                const size_t blob0 = names.size();
                for (unsigned long long k = 0; k < nr; ++k) {
                    long long pos = 0;
                    unsigned ns = 0, nh = 0;
                    if (std::sscanf(next_line().c_str(), "%4095s %lld %u %u", name, &pos, &ns, &nh) != 4) return 3;
                    sid_call_row r{};
                    r.pos = (int32_t)pos;
                    r.clen = (uint32_t)std::strlen(name);
                    for (uint32_t j = 0; j < r.clen && j < 8; ++j) r.c8 |= (uint64_t)(uint8_t)name[j] << (8 * j);
                    if (r.clen > 8) {
                        r.name = (uint32_t)(names.size() - blob0);
                        names.append(name, r.clen);
                    }
                    r.sites = ns, r.het = nh;
                    rv.push_back(r);
                }
                off[c + 1] = rv.size();
                noff[c + 1] = names.size();
            }
            sid_call_row* rows_in = (sid_call_row*)std::malloc(rv.size() ? rv.size() * sizeof(sid_call_row) : 1);
            if (!rv.empty()) std::memcpy(rows_in, rv.data(), rv.size() * sizeof(sid_call_row));
            char* blob = (char*)std::malloc(names.size() ? names.size() : 1);
            if (!names.empty()) std::memcpy(blob, names.data(), names.size());
            sid_callable_row* rows = nullptr;
            size_t nr = 0;
            const int rc = sid_callable_stitch_chunks(rows_in, off, blob, noff, edge, nc, &rows, &nr);
            print_rows(rc, rows, nr);
            std::free(rows_in);
            std::free(blob);
            std::free(off);
            std::free(noff);
            std::free(edge);
        } else if (head[0] == 'J') {
            unsigned long long na = 0, nb = 0;
            int fa = 0, fb = 0;
            if (std::sscanf(head.c_str(), "J %llu %d %llu %d", &na, &fa, &nb, &fb) != 4) return 3;
            RowList L[2];
            for (int side = 0; side < 2; ++side) {
                const unsigned long long m = side ? nb : na;
                L[side].n = m;
                L[side].rows = (sid_callable_row*)std::malloc(m ? m * sizeof(sid_callable_row) : 1);
                for (unsigned long long k = 0; k < m; ++k) {
                    long long st = 0, en = 0;
                    unsigned long long h = 0;
                    if (std::sscanf(next_line().c_str(), "%4095s %lld %lld %llu", name, &st, &en, &h) != 4) return 3;
                    const size_t cl = std::strlen(name);
                    char* nm = (char*)std::malloc(cl ? cl : 1);
                    std::memcpy(nm, name, cl);
                    L[side].names.push_back(nm);
                    L[side].rows[k] = sid_callable_row{nm, (uint32_t)cl, 0, st, en, h};
                }
            }
            sid_callable_row* rows = nullptr;
            size_t nr = 0;
            const int rc = sid_callable_join(L[0].rows, L[0].n, fa, L[1].rows, L[1].n, fb, &rows, &nr);
            print_rows(rc, rows, nr);
        } else {
            return 3;
        }
    }
    return 0;
}
