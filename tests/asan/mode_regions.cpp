// sid_asan regions CORPUS — regions.cpp (tests/test_regions_asan.py).
//
// CORPUS is a sequence of cases: a line "B <bytes> <queries>", then <bytes>
// bytes of BED text and a newline, then <queries> lines "chrom pos".  Per
// case one line "rc err_line intervals chroms" (sid_regions_from_bed; the
// counts 0 after an error), then one line of '0' / '1' per query
// (sid_regions_contains; empty after an error).  The set is also flattened
// (the device table's host form), rebuilt through sid_regions_from_intervals
// from its own intervals ("R intervals chroms"), and marked over a sid_sites
// made of the queries ("M" + the dropped bit per query, in runs by chrom).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness.h"
#include "regions.h"
#include "sites.h"

int mode_regions(const std::string& all)
{
    size_t p = 0;
    while (p < all.size()) {
        size_t nl = all.find('\n', p);
        if (nl == std::string::npos) return 3;
        unsigned long long nbytes = 0, nq = 0;
        if (std::sscanf(all.c_str() + p, "B %llu %llu", &nbytes, &nq) != 2) return 3;
        p = nl + 1;
        if (p + nbytes + 1 > all.size()) return 3;
        // an exact-size heap copy: a read past the text's end is a report
        char* bed = (char*)std::malloc(nbytes ? nbytes : 1);
        std::memcpy(bed, all.data() + p, nbytes);
        p += nbytes + 1;
        sid_regions* r = nullptr;
        uint64_t bad = 0;
        const int rc = sid_regions_from_bed(bed, nbytes, &r, &bad);
        std::free(bed);
        std::printf("%d %llu %zu %zu\n", rc, (unsigned long long)bad, sid_regions_intervals(r), sid_regions_chroms(r));
        std::string ans;
        sid_sites sites;
        std::vector<uint8_t> code;
        for (unsigned long long q = 0; q < nq; ++q) {
            nl = all.find('\n', p);
            if (nl == std::string::npos) return 3;
            const size_t sp = all.rfind(' ', nl);
            if (sp == std::string::npos || sp < p) return 3;
            const std::string chrom = all.substr(p, sp - p);
            const int32_t pos = (int32_t)std::strtol(all.c_str() + sp + 1, nullptr, 10);
            p = nl + 1;
            if (!r) continue;
            char* c = (char*)std::malloc(chrom.size() ? chrom.size() : 1);   // (not NUL-terminated)
            std::memcpy(c, chrom.data(), chrom.size());
            ans.push_back(sid_regions_contains(r, c, chrom.size(), pos) ? '1' : '0');
            std::free(c);
            if (sites.seg_name.empty() || sites.seg_name.back() != chrom) {
                sites.seg_start.push_back(sites.pos.size());
                sites.seg_name.push_back(chrom);
            }
            sites.pos.push_back(pos);
            code.push_back((uint8_t)(q & 0x8F));
        }
        std::printf("%s\n", ans.c_str());
        if (!r) continue;
        std::vector<char> flat;
        sid_regions_layout L;
        sid_regions_flatten(r, flat, &L);
        if (L.bytes != flat.size() || L.nc != r->name.size() || L.ni != r->start.size()) return 4;
        std::vector<const char*> names;
        std::vector<int32_t> st, en;
        for (size_t k = 0; k < r->name.size(); ++k)
            for (uint32_t j = r->ibeg[k]; j < r->ibeg[k + 1]; ++j) {
                names.push_back(r->name[k].c_str());
                st.push_back(r->start[j]);
                en.push_back(r->end[j]);
            }
        sid_regions* r2 = nullptr;
        if (sid_regions_from_intervals(names.data(), st.data(), en.data(), names.size(), &r2) != SID_OK) return 4;
        std::printf("R %zu %zu\n", sid_regions_intervals(r2), sid_regions_chroms(r2));
        sid_regions_free(r2);
        const size_t half = code.size() / 2;   // in two calls: the run holding `begin` is searched for
        if (sid_regions_mark(r, &sites, 0, half, code.data()) != SID_OK) return 4;
        if (sid_regions_mark(r, &sites, half, code.size(), code.data()) != SID_OK) return 4;
        std::string m = "M";
        for (uint8_t c : code) m.push_back(c & SID_CODE_DROPPED ? '1' : '0');
        std::printf("%s\n", m.c_str());
        sid_regions_free(r);
    }
    return 0;
}
