// strip.cpp — the line stripper (strip.h): scalar, AVX2 and AVX-512 builds of
// one function, byte-identical on every input, picked at run time; the
// engine's streaming form; and the map from a stripped text's offsets back to
// the input's.  Pure host C++.
#include "strip.h"

#include <string.h>

#include <algorithm>
#include <cstring>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace {

inline bool is_sep(unsigned char c) { return c == ' ' || c == '\t'; }
inline uint64_t below(unsigned k) { return k >= 64 ? ~0ull : (1ull << k) - 1; }

// One line [p, nl) (nl: its newline): the cut -- the end of its 5th token --
// or null when the line is to be copied whole (strip.h)
const char* line_cut(const char* p, const char* nl)
{
    const char* q = p;
    bool bad = false;
    int ntok = 0;
    while (ntok < 5) {
        while (q < nl && is_sep((unsigned char)*q)) ++q;
        if (q == nl) break;
        ++ntok;
        for (; q < nl && !is_sep((unsigned char)*q); ++q) bad |= (unsigned char)*q < 0x20;
    }
    return ntok == 5 && !bad ? q : nullptr;
}

size_t strip_scalar(const char* in, size_t n, char* out, size_t, uint64_t* lines_out)
{
    const char* p = in;
    const char* const end = in + n;
    char* o = out;
    uint64_t lines = 0;
    while (p < end) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        ++lines;
        if (!nl) {   // no final newline: the line whole
            std::memcpy(o, p, (size_t)(end - p));
            o += end - p;
            break;
        }
        const char* cut = line_cut(p, nl);
        if (cut) {
            std::memcpy(o, p, (size_t)(cut - p));
            o += cut - p;
            *o++ = '\n';
        } else {
            std::memcpy(o, p, (size_t)(nl + 1 - p));
            o += nl + 1 - p;
        }
        p = nl + 1;
    }
    *lines_out = lines;
    return (size_t)(o - out);
}

#if defined(__x86_64__)
#define STRIP_FN strip_avx2
#define STRIP_TARGET __attribute__((target("avx2,bmi,popcnt")))
#define STRIP_MASKS(p_, nl_, sep_, ctl_)                                                                         \
    do {                                                                                                         \
        const __m256i a = _mm256_loadu_si256((const __m256i*)(p_));                                              \
        const __m256i b = _mm256_loadu_si256((const __m256i*)((p_) + 32));                                       \
        const __m256i vn = _mm256_set1_epi8('\n'), vt = _mm256_set1_epi8('\t'), vs = _mm256_set1_epi8(' ');      \
        const uint64_t n0 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(a, vn));                            \
        const uint64_t n1 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(b, vn));                            \
        const uint64_t t0 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(a, vt));                            \
        const uint64_t t1 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(b, vt));                            \
        const uint64_t s0 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(a, vs));                            \
        const uint64_t s1 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(b, vs));                            \
        /* c >= 0x20  <=>  max(c, 0x20) == c (unsigned) */                                                       \
        const uint64_t g0 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_max_epu8(a, vs), a));        \
        const uint64_t g1 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_max_epu8(b, vs), b));        \
        const uint64_t tab = t0 | (t1 << 32);                                                                    \
        nl_ = n0 | (n1 << 32);                                                                                   \
        sep_ = tab | s0 | (s1 << 32);                                                                            \
        ctl_ = ~(g0 | (g1 << 32)) & ~tab & ~nl_;                                                                 \
    } while (0)
#define STRIP_COPY64(d_, s_)                                                                       \
    do {                                                                                           \
        const __m256i x0 = _mm256_loadu_si256((const __m256i*)(s_));                               \
        const __m256i x1 = _mm256_loadu_si256((const __m256i*)((s_) + 32));                        \
        _mm256_storeu_si256((__m256i*)(d_), x0);                                                   \
        _mm256_storeu_si256((__m256i*)((d_) + 32), x1);                                            \
    } while (0)
#include "strip_core.h"
#undef STRIP_FN
#undef STRIP_TARGET
#undef STRIP_MASKS
#undef STRIP_COPY64

#define STRIP_FN strip_avx512
#define STRIP_TARGET __attribute__((target("avx512f,avx512bw,bmi,popcnt")))
#define STRIP_MASKS(p_, nl_, sep_, ctl_)                                                           \
    do {                                                                                           \
        const __m512i v = _mm512_loadu_si512((const void*)(p_));                                   \
        const uint64_t tab = _mm512_cmpeq_epi8_mask(v, _mm512_set1_epi8('\t'));                    \
        nl_ = _mm512_cmpeq_epi8_mask(v, _mm512_set1_epi8('\n'));                                   \
        sep_ = tab | _mm512_cmpeq_epi8_mask(v, _mm512_set1_epi8(' '));                             \
        ctl_ = _mm512_cmplt_epu8_mask(v, _mm512_set1_epi8(0x20)) & ~tab & ~nl_;                    \
    } while (0)
#define STRIP_COPY64(d_, s_) _mm512_storeu_si512((void*)(d_), _mm512_loadu_si512((const void*)(s_)))
#include "strip_core.h"
#undef STRIP_FN
#undef STRIP_TARGET
#undef STRIP_MASKS
#undef STRIP_COPY64
#endif

typedef size_t (*strip_fn)(const char*, size_t, char*, size_t, uint64_t*);

bool impl_ok(int impl)
{
    if (impl == SID_STRIP_SCALAR) return true;
#if defined(__x86_64__)
    if (impl == SID_STRIP_AVX2)
        return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("bmi") && __builtin_cpu_supports("popcnt");
    if (impl == SID_STRIP_AVX512)
        return impl_ok(SID_STRIP_AVX2) && __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw");
#endif
    return false;
}

int impl_auto()
{
    static const int best = impl_ok(SID_STRIP_AVX512) ? SID_STRIP_AVX512 : impl_ok(SID_STRIP_AVX2) ? SID_STRIP_AVX2
                                                                                                    : SID_STRIP_SCALAR;
    return best;
}

strip_fn impl_fn(int impl)
{
#if defined(__x86_64__)
    if (impl == SID_STRIP_AVX2) return strip_avx2;
    if (impl == SID_STRIP_AVX512) return strip_avx512;
#endif
    return strip_scalar;
}

#if defined(__x86_64__)
// n bytes (a multiple of 64) to dst (64-B aligned) past the caches
void stream64(char* dst, const char* src, size_t n)
{
    for (size_t k = 0; k < n; k += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i*)(src + k));
        const __m128i b = _mm_loadu_si128((const __m128i*)(src + k + 16));
        const __m128i c = _mm_loadu_si128((const __m128i*)(src + k + 32));
        const __m128i d = _mm_loadu_si128((const __m128i*)(src + k + 48));
        _mm_stream_si128((__m128i*)(dst + k), a);
        _mm_stream_si128((__m128i*)(dst + k + 16), b);
        _mm_stream_si128((__m128i*)(dst + k + 32), c);
        _mm_stream_si128((__m128i*)(dst + k + 48), d);
    }
}
void store_fence() { _mm_sfence(); }
#else
void stream64(char* dst, const char* src, size_t n) { std::memcpy(dst, src, n); }
void store_fence() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }
#endif

}  // namespace

extern "C" int sid_strip_impl(void) { return impl_auto(); }

extern "C" size_t sid_strip_lines_impl(int impl, const char* in, size_t n, char* out, size_t cap, uint64_t* lines)
{
    uint64_t l = 0;
    if (lines) *lines = 0;
    if (impl == SID_STRIP_AUTO) impl = impl_auto();
    if (!impl_ok(impl) || cap < n || (n && (!in || !out))) return (size_t)-1;
    const size_t m = n ? impl_fn(impl)(in, n, out, cap, &l) : 0;
    if (lines) *lines = l;
    return m;
}

extern "C" size_t sid_strip_lines(const char* in, size_t n, char* out, size_t cap, uint64_t* lines)
{
    return sid_strip_lines_impl(SID_STRIP_AUTO, in, n, out, cap, lines);
}

extern "C" size_t sid_strip_map(const char* in, size_t n, size_t out_off)
{
    const char* p = in;
    const char* const end = in + n;
    size_t o = 0;
    while (p < end) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        if (!nl) break;   // (the last line whole: offsets map one to one)
        const char* cut = line_cut(p, nl);
        const size_t len = cut ? (size_t)(cut - p) + 1 : (size_t)(nl + 1 - p);
        if (out_off < o + len) {
            // (the stripped line's newline stands for the input line's)
            const size_t k = out_off - o;
            return (size_t)(p - in) + (cut && k == len - 1 ? (size_t)(nl - p) : k);
        }
        o += len;
        p = nl + 1;
    }
    return std::min(n, (size_t)(p - in) + (out_off - o));
}

uint64_t sid_strip_stream(const char* in, uint64_t n, char* out, uint64_t step, sid_strip_tick tick, void* user)
{
    constexpr uint64_t BLK = 32u << 10;   // input bytes a block: it and its output stay in the L1 / L2
    const strip_fn fn = impl_fn(impl_auto());
    std::vector<char> tmp(BLK + 128);
    const char* p = in;
    const char* const end = in + n;
    char* o = out;          // 64-B aligned: the bytes before it are streamed
    uint64_t carry = 0;     // tmp[0, carry): stripped, not yet a whole 64-B line
    uint64_t lines = 0, since = 0;
    while (p < end) {
        // the block: whole lines of up to BLK bytes (a longer line: that line)
        const char* e = end;
        if ((uint64_t)(end - p) > BLK) {
            e = (const char*)memrchr(p, '\n', BLK);
            if (!e) e = (const char*)std::memchr(p + BLK, '\n', (size_t)(end - p) - BLK);
            e = e ? e + 1 : end;
        }
        const uint64_t m = (uint64_t)(e - p);
        if (tmp.size() < carry + m + 64) tmp.resize(carry + m + 64);
        uint64_t l = 0;
        const uint64_t got = fn(p, m, tmp.data() + carry, m, &l);
        lines += l;
        const uint64_t total = carry + got, full = total & ~(uint64_t)63;
        stream64(o, tmp.data(), full);
        o += full;
        carry = total - full;
        std::memmove(tmp.data(), tmp.data() + full, carry);
        p = e;
        since += m;
        if (since >= step || p == end) {
            since = 0;
            std::memcpy(o, tmp.data(), carry);   // (overwritten by the line's stream later)
            store_fence();
            if (!tick(user, (uint64_t)(p - in), (uint64_t)(o - out) + carry, lines)) break;
        }
    }
    return (uint64_t)(p - in);
}
