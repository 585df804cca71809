// sid_asan depth CORPUS — parse.cpp's sid_parse_text and sid_depth_mark
// (tests/test_depth_asan.py).
//
// CORPUS: text cases (harness.h) "T <bytes> <threads> <min> <max>".  Per text
// that parsed, "M" + the dropped bit per site after sid_depth_mark with the
// case's bounds (in two calls that split the range) over codes that are a
// fixed function of the site's index, then "E" + the statuses of the calls the
// ABI rejects.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "harness.h"

int mode_depth(const std::string& corpus)
{
    return text_cases(corpus, 2, [](sid_sites* s, size_t n, const int* bounds) -> int {
        const int lo = bounds[0], hi = bounds[1];
        // exact-size codes: bits 0-3 the genotype, bit 7 het, now and then bit 6
        uint8_t* code = (uint8_t*)std::malloc(n ? n : 1);
        for (size_t i = 0; i < n; ++i) code[i] = (uint8_t)((i * 37u + (i >> 3)) & 0x8Fu) | (i % 11 == 0 ? 0x40u : 0u);
        const size_t half = n / 2;
        if (sid_depth_mark(s, 0, half, lo, hi, code) != SID_OK) return 4;
        if (sid_depth_mark(s, half, n, lo, hi, code) != SID_OK) return 4;
        std::string m = "M";
        for (size_t i = 0; i < n; ++i) m.push_back(code[i] & SID_CODE_DROPPED ? '1' : '0');
        std::printf("%s\n", m.c_str());
        std::printf("E %d %d %d %d %d %d %d\n", sid_depth_mark(s, 0, n + 1, lo, hi, code),
                    sid_depth_mark(s, n + 1, n + 1, lo, hi, code), sid_depth_mark(nullptr, 0, 0, lo, hi, code),
                    sid_depth_mark(s, 0, n, lo, hi, nullptr), sid_depth_mark(s, 0, n, -1, 0, code),
                    sid_depth_mark(s, 0, n, 9, 8, code), sid_depth_mark(s, 0, n, 0, SID_DEPTH_MAX + 1, code));
        std::free(code);
        return 0;
    });
}
