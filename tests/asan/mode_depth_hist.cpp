// sid_asan depth_hist CORPUS — depth_hist.cpp (sid_depth_hist_host / _merge /
// _format) over parse.cpp's sites (tests/test_depth_hist_asan.py).
//
// CORPUS: text cases (harness.h) "T <bytes> <threads>".  Per text that parsed:
// "H <bytes>" and the formatted rows of all sites (with the header) over codes
// that are a fixed function of the site's index; "M <bytes>" and the formatted
// merge of the rows of the two halves of the range (without the header); then
// "E" + the statuses of the calls the ABI rejects.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "harness.h"

// the rows formatted through the sizing protocol into an exact-size block
static int put_rows(const char* tag, const sid_depth_row* rows, size_t n, int header)
{
    size_t need = 0, len = 0;
    if (sid_depth_hist_format(rows, n, header, nullptr, 0, &need) != SID_ENOMEM) return 5;
    char* out = (char*)std::malloc(need ? need : 1);
    if (need > 1 && sid_depth_hist_format(rows, n, header, out, need - 1, &len) != SID_ENOMEM) return 5;
    if (sid_depth_hist_format(rows, n, header, out, need, &len) != SID_OK || len != need) return 5;
    std::printf("%s %zu\n", tag, len);
    std::fwrite(out, 1, len, stdout);
    std::free(out);
    return 0;
}

int mode_depth_hist(const std::string& corpus)
{
    return text_cases(corpus, 0, [](sid_sites* s, size_t n, const int*) -> int {
        // exact-size codes: bits 0-3 the genotype, bit 7 het, now and then bit 6
        uint8_t* code = (uint8_t*)std::malloc(n ? n : 1);
        for (size_t i = 0; i < n; ++i) code[i] = (uint8_t)((i * 37u + (i >> 3)) & 0x8Fu) | (i % 5 == 0 ? 0x40u : 0u);
        sid_depth_row *all_rows = nullptr, *a = nullptr, *b = nullptr, *m = nullptr;
        size_t na = 0, nb = 0, nm = 0, nall = 0;
        const size_t half = n / 2;
        if (sid_depth_hist_host(s, 0, n, code, &all_rows, &nall) != SID_OK) return 4;
        if (sid_depth_hist_host(s, 0, half, code, &a, &na) != SID_OK) return 4;
        if (sid_depth_hist_host(s, half, n, code, &b, &nb) != SID_OK) return 4;
        if (sid_depth_hist_merge(a, na, b, nb, &m, &nm) != SID_OK) return 4;
        if (int e = put_rows("H", all_rows, nall, 1)) return e;
        if (int e = put_rows("M", m, nm, 0)) return e;
        sid_depth_row* x = nullptr;
        size_t nx = 0;
        // (a set twice over: not strictly ascending once it has two rows or more, fed back to back)
        std::vector<sid_depth_row> twice(all_rows, all_rows + nall);
        twice.insert(twice.end(), all_rows, all_rows + nall);
        std::printf("E %d %d %d %d %d %d\n", sid_depth_hist_host(s, 0, n + 1, code, &x, &nx),
                    sid_depth_hist_host(s, n + 1, n + 1, code, &x, &nx), sid_depth_hist_host(nullptr, 0, 0, code, &x, &nx),
                    n ? sid_depth_hist_host(s, 0, n, nullptr, &x, &nx) : SID_EINVAL,
                    sid_depth_hist_host(s, 0, n, code, nullptr, &nx),
                    nall ? sid_depth_hist_merge(twice.data(), twice.size(), a, na, &x, &nx) : SID_EINVAL);
        if (x) return 4;
        sid_depth_hist_free(all_rows);
        sid_depth_hist_free(a);
        sid_depth_hist_free(b);
        sid_depth_hist_free(m);
        std::free(code);
        return 0;
    });
}
