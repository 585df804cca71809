// sid_asan context CORPUS — context.cpp: sid_context_mark and the stitch of
// the chunks' forced edge records (tests/test_context_asan.py).
//
// CORPUS is a sequence of cases.
//   "M <n> <context>", then a line of n characters ('.' a site with a record
//   in U, 'x' one without) and a line of n characters ('1' selected, '0'
//   not): sid_context_mark; one line "<rc> " + per site '1' (it keeps its
//   record) or '0'.
//   "S <context> <chunks>", then per chunk a line "C <bytes> <records>
//   <has_sel> <lead> <trail> <head_keep> <tail_keep>", <bytes> bytes (what the
//   chunk's writer emitted: its kept and its forced records) and a newline:
//   the forced records' lengths from the bytes (sid_cx_edge_lengths), the
//   stitch fed chunk by chunk as the engine's writer feeds it, every chunk cut
//   down in place once it is resolved; one line "S <bytes>", then the bytes
//   that stay and a newline.
// Every array is an exact-size heap block: a read or write past it is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "context.h"
#include "harness.h"

int mode_context(const std::string& all)
{
    size_t p = 0;
    auto line_end = [&]() {
        const size_t nl = all.find('\n', p);
        return nl == std::string::npos ? all.size() : nl;
    };
    while (p < all.size()) {
        size_t nl = line_end();
        if (all[p] == 'M') {
            unsigned long long n = 0;
            int cx = 0;
            if (std::sscanf(all.c_str() + p, "M %llu %d", &n, &cx) != 2) return 3;
            p = nl + 1;
            if (p + 2 * (n + 1) > all.size()) return 3;
            uint8_t* code_all = (uint8_t*)std::malloc(n ? n : 1);
            uint8_t* code = (uint8_t*)std::malloc(n ? n : 1);
            for (size_t i = 0; i < n; ++i) {
                code_all[i] = (uint8_t)((all[p + i] == 'x' ? SID_CODE_DROPPED : 0) | (i % 3 ? SID_CODE_HET : 0) | (i & 15));
                code[i] = (uint8_t)(code_all[i] | (all[p + n + 1 + i] == '1' ? 0 : SID_CODE_DROPPED));
            }
            p += 2 * (n + 1);
            const int rc = sid_context_mark(n ? code_all : nullptr, n ? code : nullptr, n, cx);
            std::printf("%d ", rc);
            for (size_t i = 0; i < n; ++i) std::putchar(code[i] & SID_CODE_DROPPED ? '0' : '1');
            std::putchar('\n');
            std::free(code_all);
            std::free(code);
            continue;
        }
        int cx = 0;
        unsigned long long nch = 0;
        if (std::sscanf(all.c_str() + p, "S %d %llu", &cx, &nch) != 2) return 3;
        p = nl + 1;
        std::vector<char*> bytes(nch, nullptr);
        std::vector<uint64_t> len(nch, 0);
        sid_cx_desc* d = (sid_cx_desc*)std::malloc(sizeof(sid_cx_desc) * (nch ? nch : 1));
        sid_cx_stitch S(cx);
        size_t cut = 0;   // the chunks cut down so far (resolved ones only)
        sid_cx_range g[2 * SID_CONTEXT_MAX + 1];
        auto settle = [&]() {
            for (; cut < S.resolved(); ++cut) {
                const size_t nr = sid_cx_ranges(d[cut], cx, S.verdict(cut), len[cut], g, nullptr);
                len[cut] = sid_cx_compact(bytes[cut], g, nr);
            }
        };
        for (size_t c = 0; c < nch; ++c) {
            nl = line_end();
            unsigned long long nb = 0, hk = 0, tk = 0;
            unsigned rec = 0, has = 0, lead = 0, trail = 0;
            if (std::sscanf(all.c_str() + p, "C %llu %u %u %u %u %llu %llu", &nb, &rec, &has, &lead, &trail, &hk, &tk) != 7)
                return 3;
            p = nl + 1;
            if (p + nb + 1 > all.size()) return 3;
            bytes[c] = (char*)std::malloc(nb ? nb : 1);
            std::memcpy(bytes[c], all.data() + p, nb);
            len[c] = nb;
            p += nb + 1;
            std::memset(&d[c], 0, sizeof d[c]);
            d[c].records = rec, d[c].has_sel = has, d[c].lead = lead, d[c].trail = trail;
            d[c].head_keep = hk, d[c].tail_keep = tk;
            sid_cx_edge_lengths(bytes[c], nb, cx, &d[c]);
            const size_t before = S.resolved();
            S.push(d[c]);
            if (S.resolved() < before || S.resolved() > c + 1) return 4;
            settle();
        }
        S.finish();
        if (S.resolved() != nch) return 4;
        settle();
        uint64_t tot = 0;
        for (size_t c = 0; c < nch; ++c) tot += len[c];
        std::printf("S %llu\n", (unsigned long long)tot);
        for (size_t c = 0; c < nch; ++c) {
            std::fwrite(bytes[c], 1, len[c], stdout);
            std::free(bytes[c]);
        }
        std::putchar('\n');
        std::free(d);
    }
    return 0;
}
