// text_cases.cpp — the "T" corpus of the parse-based modes (harness.h).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "harness.h"

int text_cases(const std::string& all, int nextra, text_case_fn fn)
{
    size_t p = 0;
    while (p < all.size()) {
        const size_t nl = all.find('\n', p);
        if (nl == std::string::npos) return 3;
        unsigned long long nbytes = 0;
        int threads = 0, extra[2] = {0, 0};
        if (std::sscanf(all.c_str() + p, "T %llu %d %d %d", &nbytes, &threads, &extra[0], &extra[1]) < 2 + nextra) return 3;
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
        if (const int e = fn(s, n, extra)) return e;
        sid_sites_free(s);
    }
    return 0;
}
