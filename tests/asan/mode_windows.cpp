// sid_asan windows CORPUS — windows.cpp (tests/test_windows_asan.py).
//
// CORPUS is a sequence of cases.
//   "H <W> <sites> <begin> <end>", then per site a line "<chrom> <pos>
//   <code>": sid_windows_host over sites [begin, end).
//   "S <W> <chunks>", then per chunk a line "C <rows>" and per row a line
//   "<chrom> <wi> <sites> <records> <het>": the rows in the device's layout
//   (chroms over 8 bytes in the chunk's name blob), sid_win_stitch_chunks.
// Either prints "<rc> <rows>", then the rows through sid_windows_format
// (sized, then into a block of exactly that size) without the header.
// Every array is an exact-size heap block: a read or write past it is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness.h"
#include "sites.h"
#include "windows.h"

static void print_rows(int rc, sid_window* rows, size_t n)
{
    std::printf("%d %zu\n", rc, n);
    if (rc == SID_OK) {
        size_t need = 0;
        const int s = sid_windows_format(rows, n, 0, nullptr, 0, &need);
        if (s != SID_ENOMEM) std::exit(4);
        char* out = (char*)std::malloc(need ? need : 1);
        size_t len = 0;
        if (need && sid_windows_format(rows, n, 0, out, need - 1, &len) != SID_ENOMEM) std::exit(4);
        if (sid_windows_format(rows, n, 0, out, need, &len) != SID_OK || len != need) std::exit(4);
        std::fwrite(out, 1, len, stdout);
        std::free(out);
    }
    sid_windows_free(rows);
}

int mode_windows(const std::string& all)
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
            int W = 0;
            unsigned long long n = 0, b = 0, e = 0;
            if (std::sscanf(head.c_str(), "H %d %llu %llu %llu", &W, &n, &b, &e) != 4) return 3;
            sid_sites s;
            uint8_t* code = (uint8_t*)std::malloc(n ? n : 1);
            for (unsigned long long i = 0; i < n; ++i) {
                long long pos = 0;
                unsigned c = 0;
                if (std::sscanf(next_line().c_str(), "%4095s %lld %u", name, &pos, &c) != 3) return 3;
                if (s.seg_name.empty() || s.seg_name.back() != name) {
                    s.seg_start.push_back(i);
                    s.seg_name.push_back(name);
                }
                s.pos.push_back((int32_t)pos);
                code[i] = (uint8_t)c;
            }
            s.pos.shrink_to_fit();
            sid_window* rows = nullptr;
            size_t nr = 0;
            const int rc = sid_windows_host(&s, b, e, n ? code : nullptr, W, &rows, &nr);
            print_rows(rc, rows, nr);
            std::free(code);
        } else if (head[0] == 'S') {
            int W = 0;
            unsigned long long nc = 0;
            if (std::sscanf(head.c_str(), "S %d %llu", &W, &nc) != 2) return 3;
            std::vector<sid_win_row> rv;
            std::string names;
            uint64_t* off = (uint64_t*)std::malloc((nc + 1) * 8);
            uint64_t* noff = (uint64_t*)std::malloc((nc + 1) * 8);
            off[0] = noff[0] = 0;
            for (unsigned long long c = 0; c < nc; ++c) {
                unsigned long long nr = 0;
                if (std::sscanf(next_line().c_str(), "C %llu", &nr) != 1) return 3;
                const size_t blob0 = names.size();
                for (unsigned long long k = 0; k < nr; ++k) {
                    long long wi = 0;
                    unsigned ns = 0, nrec = 0, nh = 0;
                    if (std::sscanf(next_line().c_str(), "%4095s %lld %u %u %u", name, &wi, &ns, &nrec, &nh) != 5) return 3;
                    sid_win_row r{};
                    r.wi = wi;
                    r.clen = (uint32_t)std::strlen(name);
                    for (uint32_t j = 0; j < r.clen && j < 8; ++j) r.c8 |= (uint64_t)(uint8_t)name[j] << (8 * j);
                    if (r.clen > 8) {
                        r.name = (uint32_t)(names.size() - blob0);
                        names.append(name, r.clen);
                    }
                    r.sites = ns, r.records = nrec, r.het = nh;
                    rv.push_back(r);
                }
                off[c + 1] = rv.size();
                noff[c + 1] = names.size();
            }
            sid_win_row* rows_in = (sid_win_row*)std::malloc(rv.size() ? rv.size() * sizeof(sid_win_row) : 1);
            if (!rv.empty()) std::memcpy(rows_in, rv.data(), rv.size() * sizeof(sid_win_row));
            char* blob = (char*)std::malloc(names.size() ? names.size() : 1);
            if (!names.empty()) std::memcpy(blob, names.data(), names.size());
            sid_window* rows = nullptr;
            size_t nr = 0;
            const int rc = sid_win_stitch_chunks(rows_in, off, blob, noff, nc, W, &rows, &nr);
            print_rows(rc, rows, nr);
            std::free(rows_in);
            std::free(blob);
            std::free(off);
            std::free(noff);
        } else {
            return 3;
        }
    }
    return 0;
}
