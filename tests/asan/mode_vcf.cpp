// sid_asan vcf CORPUS — emit.cpp's sid_format_vcf over parse.cpp's sites
// (tests/test_vcf_asan.py).
//
// CORPUS: text cases (harness.h) "T <bytes> <threads>".  Per text that parsed,
// "V <bytes>", the VCF lines of the sites (two calls that split the range, each
// sized by the protocol and written into a heap block of exactly the size it
// asked for) and a newline, then "E" + the statuses of the calls the ABI
// rejects.  The codes and confidences are fixed functions of the site's index.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "harness.h"

static double conf(size_t k)
{
    static const double T[9] = {1.0, 0.0, 1e-300, -4.94066e-324, std::numeric_limits<double>::quiet_NaN(),
                                std::numeric_limits<double>::infinity(), 0.05, 123456.0, 1e22};
    return T[k % 9];
}

int mode_vcf(const std::string& corpus)
{
    return text_cases(corpus, 0, [](sid_sites* s, size_t n, const int*) -> int {
        // exact-size arrays: bits 0-3 the genotype, bit 7 het, now and then bit 6
        uint8_t* code = (uint8_t*)std::malloc(n ? n : 1);
        double* hom = (double*)std::malloc((n ? n : 1) * sizeof(double));
        double* het = (double*)std::malloc((n ? n : 1) * sizeof(double));
        for (size_t i = 0; i < n; ++i) {
            code[i] = (uint8_t)((i * 37u + (i >> 3)) & 0x8Fu) | (i % 11 == 0 ? 0x40u : 0u);
            hom[i] = conf(i);
            het[i] = conf(i * 7 + 3);
        }
        std::string out;
        const size_t half = n / 2;
        for (int part = 0; part < 2; ++part) {
            const size_t b = part ? half : 0, e = part ? n : half;
            size_t need = 0, len = 0;
            const int r0 = sid_format_vcf(s, b, e, code, hom, het, nullptr, 0, &need);
            if (r0 != SID_ENOMEM && !(r0 == SID_OK && need == 0)) return 4;
            char* o = (char*)std::malloc(need ? need : 1);
            if (need && sid_format_vcf(s, b, e, code, hom, het, o, need - 1, &len) != SID_ENOMEM) return 4;
            if (sid_format_vcf(s, b, e, code, hom, het, o, need, &len) != SID_OK || len > need) return 4;
            out.append(o, len);
            std::free(o);
        }
        std::printf("V %zu\n", out.size());
        std::fwrite(out.data(), 1, out.size(), stdout);
        std::printf("\n");
        size_t len = 0;
        char tiny[8];
        std::printf("E %d %d %d %d %d %d\n", sid_format_vcf(s, 0, n + 1, code, hom, het, tiny, sizeof tiny, &len),
                    sid_format_vcf(s, n + 1, n + 1, code, hom, het, tiny, sizeof tiny, &len),
                    sid_format_vcf(nullptr, 0, 0, code, hom, het, tiny, sizeof tiny, &len),
                    sid_format_vcf(s, 0, n, nullptr, hom, het, tiny, sizeof tiny, &len),
                    sid_format_vcf(s, 0, n, code, hom, het, tiny, sizeof tiny, nullptr),
                    n ? sid_format_vcf(s, 0, n, code, hom, het, tiny, sizeof tiny, &len) : SID_ENOMEM);
        std::free(code);
        std::free(hom);
        std::free(het);
        return 0;
    });
}
