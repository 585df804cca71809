// sid_asan variants CORPUS — parse.cpp's reference bytes and sid_variants_mark
// (tests/test_variants_asan.py).
//
// CORPUS: text cases (harness.h) "T <bytes> <threads>".  Per text that parsed,
// a line of the sites' reference bytes in hex, then "M" + the dropped bit per
// site after sid_variants_mark (in two calls that split the range) over codes
// that are a fixed function of the site's index, then "E" + the statuses of
// the calls the ABI rejects.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "harness.h"

int mode_variants(const std::string& corpus)
{
    return text_cases(corpus, 0, [](sid_sites* s, size_t n, const int*) -> int {
        const uint8_t* refs = sid_sites_refs(s);
        std::string hex;
        for (size_t i = 0; i < n; ++i) {
            char h[3];
            std::snprintf(h, sizeof h, "%02x", refs[i]);
            hex += h;
        }
        std::printf("%s\n", hex.c_str());
        // exact-size codes: bits 0-3 the genotype, bit 7 het, now and then bit 6
        uint8_t* code = (uint8_t*)std::malloc(n ? n : 1);
        for (size_t i = 0; i < n; ++i) code[i] = (uint8_t)((i * 37u + (i >> 3)) & 0x8Fu) | (i % 11 == 0 ? 0x40u : 0u);
        const size_t half = n / 2;
        if (sid_variants_mark(s, 0, half, code) != SID_OK) return 4;
        if (sid_variants_mark(s, half, n, code) != SID_OK) return 4;
        std::string m = "M";
        for (size_t i = 0; i < n; ++i) m.push_back(code[i] & SID_CODE_DROPPED ? '1' : '0');
        std::printf("%s\n", m.c_str());
        std::printf("E %d %d %d %d\n", sid_variants_mark(s, 0, n + 1, code), sid_variants_mark(s, n + 1, n + 1, code),
                    sid_variants_mark(nullptr, 0, 0, code), sid_variants_mark(s, 0, n, nullptr));
        std::free(code);
        return 0;
    });
}
