// bgzf.h — the BGZF decoder core: member header (RFC 1952 + SAM spec §4.1),
// inflate (RFC 1951, complete) and CRC32, as __host__ __device__ code without
// a HIP call.  One source for the host build (bgzf.cpp: the index, the host
// inflate, the engine's chunk cuts; tests/asan runs it under ASan +
// UBSan) and for the kernel (inflate.hip).
//
// Bounds.  The decoder reads only in[0, n) and hands its output policy only
// writes inside [0, cap) and copies whose source lies inside [0, pos): every
// read past the compressed extent (the bit reader feeds zeros there and the
// overrun is an error), every write past cap, every distance past the first
// byte and every invalid code set is a status, never an access.
//
// The symbol loop keeps the bit buffer, the positions and the table entries
// uniform over a wave (BGZF_UNI: readfirstlane on the device, nothing on the
// host), so a wave that decodes one member together holds them in scalar
// registers; what is parallel -- literal runs, match copies, stored bytes --
// is the output policy's business.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define BGZF_HD __host__ __device__
#else
#define BGZF_HD
#endif
// The CRC routines are inlined into their caller: the lanes of a wave walk
// spans of different lengths there (some of them empty), and a call in that
// divergent code made the compiler save a register across it while the empty
// lanes were masked off (the kernel then lost its lane number in those lanes).
#define BGZF_FLAT __attribute__((always_inline))
#if defined(__HIP_DEVICE_COMPILE__)
#define BGZF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define BGZF_UNI(x) ((uint32_t)(x))
#endif

enum {
    BGZF_OK = 0,
    BGZF_EHEADER = 1,   // not a BGZF member header
    BGZF_ETRUNC = 2,    // the member does not fit the bytes given / reads past its extent
    BGZF_EBTYPE = 3,    // block type 3
    BGZF_ESTORED = 4,   // LEN / NLEN disagree
    BGZF_ECODES = 5,    // invalid, over-subscribed or incomplete code set
    BGZF_ESYMBOL = 6,   // a bit pattern that is no code, length symbol 286/287, distance symbol 30/31
    BGZF_EDIST = 7,     // distance reaches back past the first byte
    BGZF_EFULL = 8,     // output past ISIZE
    BGZF_ESHORT = 9,    // final block ended with the output short of ISIZE
    BGZF_ECRC = 10,     // CRC32 mismatch
};

constexpr uint32_t BGZF_MAX_ISIZE = 65536;
constexpr uint32_t BGZF_LIT_BITS = 10, BGZF_DIST_BITS = 9, BGZF_CL_BITS = 7;

// Huffman tables of one deflate block (4 KiB: the device keeps them in LDS).
// Primary lookup by the next BITS input bits: (symbol << 4) | length, 0 for a
// longer (or no) code, which the canonical walk over cnt / sym then decodes.
struct bgzf_tables {
    uint16_t lit[1u << BGZF_LIT_BITS];
    uint16_t dist[1u << BGZF_DIST_BITS];   // (the code-length code's 7-bit table while a header is read)
    uint16_t lsym[288], dsym[32];          // symbols sorted by (length, symbol)
    uint16_t lcnt[16], dcnt[16];           // codes per length
    uint8_t len[320];                      // the code lengths read from a dynamic header
};

// ------------------------------------------------------------- container --
struct bgzf_member {
    uint32_t hdr;     // header bytes: the deflate data starts there
    uint32_t bsize;   // the whole member's bytes (BSIZE + 1)
    uint32_t isize;   // inflated bytes (trailer)
    uint32_t crc;     // CRC32 of the inflated bytes (trailer)
};

BGZF_HD inline uint32_t bgzf_le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
BGZF_HD inline uint32_t bgzf_le32(const uint8_t* p) { return bgzf_le16(p) | (bgzf_le16(p + 2) << 16); }

// One member at p, of which n bytes are readable.  BGZF_EHEADER: no BGZF
// header there (plain gzip included); BGZF_ETRUNC: a header whose member does
// not fit n (or n too short to tell).
BGZF_HD inline int bgzf_member_parse(const uint8_t* p, uint64_t n, bgzf_member* m)
{
    if (n >= 1 && p[0] != 0x1f) return BGZF_EHEADER;
    if (n >= 2 && p[1] != 0x8b) return BGZF_EHEADER;
    if (n >= 3 && p[2] != 8) return BGZF_EHEADER;
    if (n >= 4 && !(p[3] & 4)) return BGZF_EHEADER;
    if (n < 12) return n == 0 ? BGZF_EHEADER : BGZF_ETRUNC;
    const uint32_t xlen = bgzf_le16(p + 10);
    if (n < 12ull + xlen) return BGZF_ETRUNC;
    uint32_t q = 12, end = 12 + xlen, bsize = 0;
    bool found = false;
    while (q + 4 <= end) {   // the subfields; others may precede BC
        const uint32_t slen = bgzf_le16(p + q + 2);
        if (q + 4 + slen > end) break;
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2) {
            bsize = bgzf_le16(p + q + 4) + 1;
            found = true;
            break;
        }
        q += 4 + slen;
    }
    if (!found) return BGZF_EHEADER;
    if (bsize < end + 8) return BGZF_EHEADER;
    if (n < bsize) return BGZF_ETRUNC;
    m->hdr = end;
    m->bsize = bsize;
    m->crc = bgzf_le32(p + bsize - 8);
    m->isize = bgzf_le32(p + bsize - 4);
    if (m->isize > BGZF_MAX_ISIZE) return BGZF_EHEADER;
    return BGZF_OK;
}

// ------------------------------------------------------------------ CRC32 --
// IEEE, reflected (zlib's).  A span's raw remainder (register 0 at its start,
// no final xor) is linear in its bytes, so spans are combined by shifting each
// over the bytes behind it: crc(M) = ~(shift(~crc0, |M|) ^ xor over the spans
// of shift(raw(span), bytes after the span)).
constexpr uint32_t BGZF_CRC_POLY = 0xedb88320u;

BGZF_HD BGZF_FLAT inline uint32_t bgzf_crc_entry(uint32_t k)
{
    for (int j = 0; j < 8; ++j) k = (k >> 1) ^ (BGZF_CRC_POLY & (0u - (k & 1)));
    return k;
}
// a(x) * b(x) mod P, reflected bit order (zlib crc32.c multmodp)
BGZF_HD BGZF_FLAT inline uint32_t bgzf_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (BGZF_CRC_POLY & (0u - (b & 1)));
    }
    return p;
}
// c(x) * x^(8 * bytes) mod P by square-and-multiply: the register after
// `bytes` zero bytes
BGZF_HD BGZF_FLAT inline uint32_t bgzf_crc_shift(uint32_t c, uint64_t bytes)
{
    uint32_t p = 1u << 31, sq = 1u << 23;   // x^0, x^8
    for (; bytes; bytes >>= 1) {
        if (bytes & 1) p = bgzf_crc_mul(p, sq);
        sq = bgzf_crc_mul(sq, sq);
    }
    return bgzf_crc_mul(c, p);
}
BGZF_HD BGZF_FLAT inline uint32_t bgzf_crc_raw(const uint32_t* tab, const uint8_t* p, uint64_t n)
{
    uint32_t c = 0;
    for (uint64_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c;
}
// lane `lane` of `lanes` takes bytes [n * lane / lanes, n * (lane + 1) / lanes)
BGZF_HD BGZF_FLAT inline uint32_t bgzf_crc_lane(const uint32_t* tab, const uint8_t* p, uint64_t n, uint32_t lane,
                                      uint32_t lanes)
{
    const uint64_t a = n * lane / lanes, b = n * (lane + 1) / lanes;
    return bgzf_crc_shift(bgzf_crc_raw(tab, p + a, b - a), n - b);
}
BGZF_HD BGZF_FLAT inline uint32_t bgzf_crc_finish(uint32_t crc0, uint32_t xored, uint64_t n)
{
    return ~(bgzf_crc_shift(~crc0, n) ^ xored);
}

// ---------------------------------------------------------------- inflate --
struct bgzf_bits {
    const uint8_t* in;
    uint32_t ip, iend;   // next byte, extent
    uint64_t buf;
    uint32_t nbits;
};

BGZF_HD inline void bgzf_refill(bgzf_bits& b)
{
    if (b.ip + 8 <= b.iend) {
        uint64_t w;
        memcpy(&w, b.in + b.ip, 8);
        b.buf |= w << b.nbits;
        b.ip += (63 - b.nbits) >> 3;
        b.nbits |= 56;
    } else {
        while (b.nbits < 56) {   // past the extent: zeros, and the overrun is found by bgzf_over
            const uint64_t c = b.ip < b.iend ? b.in[b.ip] : 0;
            b.buf |= c << b.nbits;
            ++b.ip;
            b.nbits += 8;
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
    b.buf = (uint64_t)BGZF_UNI((uint32_t)b.buf) | ((uint64_t)BGZF_UNI((uint32_t)(b.buf >> 32)) << 32);
#endif
}
BGZF_HD inline bool bgzf_over(const bgzf_bits& b) { return (uint64_t)b.ip * 8 - b.nbits > (uint64_t)b.iend * 8; }
BGZF_HD inline uint32_t bgzf_take(bgzf_bits& b, uint32_t k)   // k <= 16, after a refill
{
    const uint32_t v = (uint32_t)b.buf & ((1u << k) - 1);
    b.buf >>= k;
    b.nbits -= k;
    return v;
}

// Canonical code from `n` lengths: cnt, sym and the primary table of `bits`
// bits.  An over-subscribed set is an error; an incomplete one too, unless
// every code has length 1 (zlib accepts the single-code case; not for the
// code-length code) or, for the distance code only, there is no code at all.
enum { BGZF_CODES = 0, BGZF_LENS = 1, BGZF_DISTS = 2 };
BGZF_HD inline int bgzf_build(const uint8_t* len, uint32_t n, uint16_t* cnt, uint16_t* sym, uint16_t* tab,
                              uint32_t bits, int kind)
{
    uint16_t offs[16];
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++cnt[len[s] & 15];
    for (uint32_t e = 0; e < (1u << bits); ++e) tab[e] = 0;
    int left = 1;
    uint32_t maxl = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return BGZF_ECODES;
        if (cnt[l]) maxl = l;
    }
    if (maxl == 0) return kind == BGZF_DISTS ? BGZF_OK : BGZF_ECODES;
    if (left > 0 && (kind == BGZF_CODES || maxl != 1)) return BGZF_ECODES;
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (uint32_t s = 0; s < n; ++s)
        if (len[s] & 15) sym[offs[len[s] & 15]++] = (uint16_t)s;
    uint32_t code = 0, k = 0;
    for (uint32_t l = 1; l <= bits && l <= maxl; ++l) {
        for (uint32_t j = 0; j < cnt[l]; ++j, ++k, ++code) {
            uint32_t r = 0;   // the code's bits reversed: deflate packs codes from their first bit
            for (uint32_t t = 0; t < l; ++t) r |= ((code >> t) & 1) << (l - 1 - t);
            const uint16_t e = (uint16_t)((sym[k] << 4) | l);
            for (; r < (1u << bits); r += 1u << l) tab[r] = e;
        }
        code <<= 1;
    }
    return BGZF_OK;
}

// One symbol: the primary table, else the canonical walk bit by bit.  -1: the
// bits are no code of this set.  (15 bits available: callers refill first.)
BGZF_HD inline int bgzf_symbol(bgzf_bits& b, const uint16_t* tab, uint32_t bits, const uint16_t* cnt,
                               const uint16_t* sym)
{
    const uint32_t e = BGZF_UNI(tab[(uint32_t)b.buf & ((1u << bits) - 1)]);
    if (e) {
        b.buf >>= (e & 15);
        b.nbits -= (e & 15);
        return (int)(e >> 4);
    }
    uint32_t code = 0, first = 0, index = 0;
    uint64_t v = b.buf;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= (uint32_t)v & 1;
        v >>= 1;
        const uint32_t c = BGZF_UNI(cnt[l]);
        if (code < first + c) {
            b.buf >>= l;
            b.nbits -= l;
            return (int)BGZF_UNI(sym[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// The output policy `Out`:
//   uint32_t pos, cap;                   bytes written so far, ISIZE
//   void lit(uint8_t c);                 pos < cap
//   void copy(uint32_t dist, uint32_t len);   1 <= dist <= pos, pos + len <= cap; may overlap
//   void raw(const uint8_t* src, uint32_t len);  stored bytes, pos + len <= cap
//   void finish();                       everything written
struct bgzf_host_out {
    uint8_t* o;
    uint32_t pos, cap;
    BGZF_HD void lit(uint8_t c) { o[pos++] = c; }
    BGZF_HD void copy(uint32_t dist, uint32_t len)
    {
        for (uint32_t i = 0; i < len; ++i, ++pos) o[pos] = o[pos - dist];
    }
    BGZF_HD void raw(const uint8_t* src, uint32_t len)
    {
        for (uint32_t i = 0; i < len; ++i) o[pos++] = src[i];
    }
    BGZF_HD void finish() {}
};

// Inflates the deflate stream in[0, n) into out (exactly out.cap bytes).
template <class Out>
BGZF_HD inline int bgzf_inflate(const uint8_t* in, uint32_t n, Out& out, bgzf_tables& T)
{
    bgzf_bits b{in, 0, n, 0, 0};
    for (uint32_t last = 0; !last;) {
        bgzf_refill(b);
        last = bgzf_take(b, 1);
        const uint32_t type = bgzf_take(b, 2);
        if (type == 3) return BGZF_EBTYPE;
        if (type == 0) {
            bgzf_take(b, b.nbits & 7);
            bgzf_refill(b);
            const uint32_t len = bgzf_take(b, 16), nlen = bgzf_take(b, 16);
            if (bgzf_over(b)) return BGZF_ETRUNC;
            if ((len ^ nlen) != 0xffff) return BGZF_ESTORED;
            b.ip -= b.nbits >> 3;   // whole bytes left in the buffer go back
            b.nbits = 0;
            b.buf = 0;
            if (b.ip > b.iend || len > b.iend - b.ip) return BGZF_ETRUNC;
            if (len > out.cap - out.pos) return BGZF_EFULL;
            out.raw(in + b.ip, len);
            b.ip += len;
            continue;
        }
        if (type == 1) {
            for (uint32_t s = 0; s < 288; ++s) T.len[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            for (uint32_t s = 0; s < 30; ++s) T.len[288 + s] = 5;
            // (30 five-bit distance codes: an incomplete set by construction, so built as 32)
            T.len[318] = T.len[319] = 5;
            bgzf_build(T.len, 288, T.lcnt, T.lsym, T.lit, BGZF_LIT_BITS, BGZF_LENS);
            bgzf_build(T.len + 288, 32, T.dcnt, T.dsym, T.dist, BGZF_DIST_BITS, BGZF_DISTS);
        } else {
            const uint32_t hlit = bgzf_take(b, 5) + 257, hdist = bgzf_take(b, 5) + 1, hclen = bgzf_take(b, 4) + 4;
            if (hlit > 286 || hdist > 30) return BGZF_ECODES;
            const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint8_t cl[19];
            for (uint32_t i = 0; i < 19; ++i) cl[i] = 0;
            for (uint32_t i = 0; i < hclen; ++i) {
                bgzf_refill(b);
                cl[ord[i]] = (uint8_t)bgzf_take(b, 3);
            }
            // (the code-length code: its symbols in dsym, its table in dist, both rebuilt below)
            if (bgzf_build(cl, 19, T.dcnt, T.dsym, T.dist, BGZF_CL_BITS, BGZF_CODES)) return BGZF_ECODES;
            for (uint32_t i = 0; i < hlit + hdist;) {
                bgzf_refill(b);
                if (bgzf_over(b)) return BGZF_ETRUNC;
                const int s = bgzf_symbol(b, T.dist, BGZF_CL_BITS, T.dcnt, T.dsym);
                if (s < 0) return BGZF_ESYMBOL;
                if (s < 16) {
                    T.len[i++] = (uint8_t)s;
                    continue;
                }
                uint32_t rep, v = 0;
                if (s == 16) {
                    if (i == 0) return BGZF_ECODES;
                    v = T.len[i - 1];
                    rep = 3 + bgzf_take(b, 2);
                } else if (s == 17)
                    rep = 3 + bgzf_take(b, 3);
                else
                    rep = 11 + bgzf_take(b, 7);
                if (i + rep > hlit + hdist) return BGZF_ECODES;
                for (; rep; --rep) T.len[i++] = (uint8_t)v;
            }
            if (T.len[256] == 0) return BGZF_ECODES;   // no end-of-block code
            if (bgzf_build(T.len, hlit, T.lcnt, T.lsym, T.lit, BGZF_LIT_BITS, BGZF_LENS)) return BGZF_ECODES;
            if (bgzf_build(T.len + hlit, hdist, T.dcnt, T.dsym, T.dist, BGZF_DIST_BITS, BGZF_DISTS)) return BGZF_ECODES;
        }
        for (;;) {
            bgzf_refill(b);   // 56 bits: a length code, its extra bits, a distance code and its extra bits are 48
            if (bgzf_over(b)) return BGZF_ETRUNC;
            int s = bgzf_symbol(b, T.lit, BGZF_LIT_BITS, T.lcnt, T.lsym);
            if (s < 0) return BGZF_ESYMBOL;
            if (s < 256) {
                if (out.pos >= out.cap) return BGZF_EFULL;
                out.lit((uint8_t)s);
                continue;
            }
            if (s == 256) break;
            s -= 257;
            if (s >= 29) return BGZF_ESYMBOL;
            uint32_t len;
            if (s < 8)
                len = 3 + s;
            else if (s == 28)
                len = 258;
            else {
                const uint32_t x = (uint32_t)(s - 4) >> 2;
                len = 3 + ((4 + (s & 3)) << x) + bgzf_take(b, x);
            }
            const int d = bgzf_symbol(b, T.dist, BGZF_DIST_BITS, T.dcnt, T.dsym);
            if (d < 0 || d >= 30) return BGZF_ESYMBOL;
            uint32_t dist;
            if (d < 4)
                dist = 1 + d;
            else {
                const uint32_t x = (uint32_t)(d - 2) >> 1;
                dist = 1 + ((2 + (d & 1)) << x) + bgzf_take(b, x);
            }
            if (dist > out.pos) return BGZF_EDIST;
            if (len > out.cap - out.pos) return BGZF_EFULL;
            out.copy(dist, len);
        }
        if (bgzf_over(b)) return BGZF_ETRUNC;
    }
    out.finish();
    if (out.pos != out.cap) return BGZF_ESHORT;
    return BGZF_OK;
}
