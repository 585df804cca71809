// driver.cpp — parse.cpp's sid_parse_text and sid_depth_mark under ASan + UBSan
// (tests/test_depth_asan.py).
//
//   depth_asan CORPUS
//
// CORPUS is a sequence of cases: a line "T <bytes> <threads> <min> <max>", then
// <bytes> bytes of pileup text and a newline.  Per case one line "rc err_line
// sites" (sid_parse_text; sites 0 after an error) and, when it parsed, "M" +
// the dropped bit per site after sid_depth_mark with the case's bounds (in two
// calls that split the range) over codes that are a fixed function of the
// site's index, then "E" + the statuses of the calls the ABI rejects.  The
// text and the codes are exact-size heap blocks: an access past their ends is
// a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sid.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::string all;
    char buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) all.append(buf, k);
    std::fclose(f);
    size_t p = 0;
    while (p < all.size()) {
        const size_t nl = all.find('\n', p);
        if (nl == std::string::npos) return 3;
        unsigned long long nbytes = 0;
        int threads = 0, lo = 0, hi = 0;
        if (std::sscanf(all.c_str() + p, "T %llu %d %d %d", &nbytes, &threads, &lo, &hi) != 4) return 3;
        p = nl + 1;
        if (p + nbytes + 1 > all.size()) return 3;
        char* text = (char*)std::malloc(nbytes ? nbytes : 1);
        std::memcpy(text, all.data() + p, nbytes);
        p += nbytes + 1;
        sid_sites* s = nullptr;
        uint64_t bad = 0;
        const int rc = sid_parse_text(text, nbytes, threads, &s, &bad);
        std::free(text);
        const size_t n = sid_sites_count(s);
        std::printf("%d %llu %zu\n", rc, (unsigned long long)(rc ? bad : 0), n);
        if (rc != SID_OK) {
            if (s) return 4;
            continue;
        }
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
        sid_sites_free(s);
    }
    return 0;
}
