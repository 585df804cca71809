// strip_san — the line stripper driven over a case file, built with
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_strip_san.py).
//
//   strip_san CASES
//
// CASES holds cases of "<n> <align>\n" + n bytes + "\n".  Every case's text is
// copied into a heap block that ends with its last byte, its first byte
// `align` bytes past a 64-B boundary, and stripped into a block of exactly n
// bytes by every variant this CPU runs (all must agree), then by the engine's
// streaming form with a small step, then mapped back line by line
// (sid_strip_map).  Prints "<m> <lines>\n" + the m stripped bytes + "\n" per
// case; exit status 1 on a disagreement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "strip.h"

static int fail(const char* what, size_t c)
{
    std::fprintf(stderr, "strip_san: case %zu: %s\n", c, what);
    return 1;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    size_t n, align;
    for (size_t c = 0; std::fscanf(f, "%zu %zu", &n, &align) == 2; ++c) {
        if (std::fgetc(f) != '\n') return fail("header", c);
        void* blk = nullptr;
        if (posix_memalign(&blk, 64, align + n + (align + n == 0))) return 2;
        char* in = (char*)blk + align;
        if (n && std::fread(in, 1, n, f) != n) return fail("short text", c);
        if (std::fgetc(f) != '\n') return fail("trailer", c);
        std::string want;
        uint64_t want_lines = 0;
        for (int impl = SID_STRIP_AUTO; impl <= SID_STRIP_AVX512; ++impl) {
            char* out = (char*)std::malloc(n ? n : 1);
            uint64_t lines = 0;
            const size_t m = sid_strip_lines_impl(impl, in, n, out, n, &lines);
            if (m == (size_t)-1) {
                std::free(out);
                if (impl <= SID_STRIP_SCALAR) return fail("variant missing", c);
                continue;
            }
            if (m > n) return fail("longer than the input", c);
            if (impl == SID_STRIP_AUTO) want.assign(out, m), want_lines = lines;
            else if (want != std::string(out, m) || lines != want_lines) return fail("variants disagree", c);
            std::free(out);
        }
        // the streaming form: whole lines only (the engine's regions), 64-B aligned output
        const char* last = n ? (const char*)memrchr(in, '\n', n) : nullptr;
        const size_t whole = last ? (size_t)(last + 1 - in) : 0;
        void* so = nullptr;
        if (posix_memalign(&so, 64, whole + 64)) return 2;
        struct Seen {
            uint64_t in_done = 0, out_done = 0, lines = 0, ticks = 0;
        } seen;
        const uint64_t used = sid_strip_stream(in, whole, (char*)so, 256,
                                               [](void* u, uint64_t a, uint64_t b, uint64_t l) {
                                                   Seen& s = *(Seen*)u;
                                                   if (a < s.in_done || b < s.out_done) return false;
                                                   s.in_done = a, s.out_done = b, s.lines = l, ++s.ticks;
                                                   return true;
                                               },
                                               &seen);
        if (used != whole || seen.in_done != whole) return fail("stream: input not consumed", c);
        {
            std::vector<char> ref(whole ? whole : 1);
            uint64_t l = 0;
            const size_t m = sid_strip_lines(in, whole, ref.data(), whole, &l);
            if (m != seen.out_done || l != seen.lines || std::memcmp(ref.data(), so, m)) return fail("stream differs", c);
            // the map back: every stripped line's start is its input line's start
            size_t i = 0, o = 0;
            while (i < whole) {
                if (sid_strip_map(in, whole, o) != i) return fail("map", c);
                const char* a = (const char*)std::memchr(in + i, '\n', whole - i);
                const char* b = (const char*)std::memchr(ref.data() + o, '\n', m - o);
                if (!a || !b) return fail("map: lines", c);
                i = (size_t)(a + 1 - in);
                o = (size_t)(b + 1 - ref.data());
            }
            if (o != m || sid_strip_map(in, whole, m) != whole) return fail("map: end", c);
        }
        std::free(so);
        std::printf("%zu %llu\n", want.size(), (unsigned long long)want_lines);
        std::fwrite(want.data(), 1, want.size(), stdout);
        std::fputc('\n', stdout);
        std::free(blk);
    }
    std::fclose(f);
    return 0;
}
