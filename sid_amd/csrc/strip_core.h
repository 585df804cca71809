// strip_core.h — the vector stripper's body, included by strip.cpp once per
// instruction set (no include guard).  The including file defines
//   STRIP_FN      the function's name
//   STRIP_TARGET  its target attribute
//   STRIP_MASKS   (p, nl, sep, ctl): the 64 bytes at p as three bit masks --
//                 '\n'; ' ' or '\t'; a byte below 0x20 that is neither '\t'
//                 nor '\n'
//   STRIP_COPY64  (dst, src): 64 bytes, unaligned
//
// 64 bytes a step: the newline mask cuts the block into line segments; in a
// segment the token starts are the non-separator bits whose lower neighbour is
// a separator (or the line's start), the 5th of them opens the read bases, and
// the first separator bit at or above it -- or the newline -- is the cut.  The
// state of a line that runs over a block's end (tokens seen, inside a token,
// the cut, a control byte in front of it) is carried.  Semantics: strip.h.

STRIP_TARGET static size_t STRIP_FN(const char* in, size_t n, char* out, size_t cap, uint64_t* lines_out)
{
    constexpr unsigned NONE = 65;
    const char* p = in;
    const char* const end = in + n;
    char* o = out;
    char* const oend = out + cap;
    const char* ls = in;         // the current line's start
    const char* cut = nullptr;   // ... its cut, once found
    unsigned ntok = 0;           // ... the tokens begun so far (5: the read bases, or behind them)
    bool prev_ns = false;        // ... the block before ended inside a token
    bool bad = false;            // ... a control byte in front of the cut
    uint64_t lines = 0;
    // [s, s + len) to o: 64 bytes a step where both sides have the room (what a step writes past len is
    // overwritten by the next line), else memcpy
#define STRIP_PUT(s_, len_)                                                             \
    do {                                                                                \
        const char* s = (s_);                                                           \
        const size_t len = (len_), r = (len + 63) & ~(size_t)63;                        \
        if (len <= 512 && (size_t)(end - s) >= r && (size_t)(oend - o) >= r) {          \
            for (size_t k = 0; k < len; k += 64) STRIP_COPY64(o + k, s + k);            \
        } else {                                                                        \
            std::memcpy(o, s, len);                                                     \
        }                                                                               \
        o += len;                                                                       \
    } while (0)
    while (p < end) {
        const size_t m = (size_t)(end - p);
        const unsigned W = m >= 64 ? 64u : (unsigned)m;
        uint64_t nl, sep, ctl;
        if (W == 64) {
            STRIP_MASKS(p, nl, sep, ctl);
        } else {
            alignas(64) char t[64];
            std::memset(t, 'x', sizeof t);
            std::memcpy(t, p, m);
            STRIP_MASKS(t, nl, sep, ctl);
            nl &= below(W), sep &= below(W), ctl &= below(W);
        }
        unsigned lo = 0;
        for (;;) {
            const uint64_t nlr = nl & ~below(lo);
            const unsigned se = nlr ? (unsigned)__builtin_ctzll(nlr) : W;   // the segment's end: its newline, or the block's
            if (!cut) {
                const uint64_t seg = below(se) & ~below(lo);
                const uint64_t S = sep & seg, N = ~sep & seg;
                unsigned cp = NONE;
                if (ntok < 5) {
                    uint64_t st = N & ~((N << 1) | ((uint64_t)prev_ns << lo));
                    const unsigned c = (unsigned)__builtin_popcountll(st);
                    if (ntok + c >= 5) {
                        for (unsigned k = ntok + 1; k < 5; ++k) st &= st - 1;
                        const unsigned p5 = (unsigned)__builtin_ctzll(st);
                        ntok = 5;
                        const uint64_t af = S & ~below(p5);
                        cp = af ? (unsigned)__builtin_ctzll(af) : se < W ? se : NONE;
                    } else {
                        ntok += c;
                    }
                } else {
                    cp = S ? (unsigned)__builtin_ctzll(S) : se < W ? se : NONE;
                }
                if (ctl & seg & below(cp != NONE ? cp : se)) bad = true;
                if (cp != NONE) cut = p + cp;
                prev_ns = se == W && ((N >> (W - 1)) & 1);
            }
            if (se == W) break;
            const char* nlp = p + se;
            ++lines;
            if (cut && !bad) {
                STRIP_PUT(ls, (size_t)(cut - ls));
                *o++ = '\n';
            } else {
                STRIP_PUT(ls, (size_t)(nlp + 1 - ls));
            }
            ls = nlp + 1;
            cut = nullptr;
            ntok = 0;
            prev_ns = bad = false;
            lo = se + 1;
            if (lo >= W) break;
        }
        p += W;
    }
    if (ls < end) {   // no final newline: the line whole
        std::memcpy(o, ls, (size_t)(end - ls));
        o += end - ls;
        ++lines;
    }
    *lines_out = lines;
    return (size_t)(o - out);
}
#undef STRIP_PUT
