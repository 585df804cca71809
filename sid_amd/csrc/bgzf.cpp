// bgzf.cpp — the host side of BGZF input: the block index (hops over headers
// and trailers only), the host inflate (every block, every CRC) and
// sid_crc32, all through the decoder core of bgzf.h.  Plain C++: no HIP call,
// no libz.
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "bgzf_host.h"

static const uint32_t* crc_table()
{
    static uint32_t tab[256];
    static bool ready = [] {
        for (uint32_t k = 0; k < 256; ++k) tab[k] = bgzf_crc_entry(k);
        return true;
    }();
    (void)ready;
    return tab;
}

// the device routine, its 64 lanes one after another
extern "C" uint32_t sid_crc32(uint32_t crc, const void* p, size_t n)
{
    if (!p || !n) return crc;
    const uint32_t* tab = crc_table();
    uint32_t x = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) x ^= bgzf_crc_lane(tab, (const uint8_t*)p, n, lane, 64);
    return bgzf_crc_finish(crc, x, n);
}

extern "C" int sid_bgzf_index(const void* bytes, size_t len, sid_bgzf** out, uint64_t* err_offset)
{
    if (out) *out = nullptr;
    if (err_offset) *err_offset = 0;
    if (!out || (!bytes && len)) return SID_EINVAL;
    sid_bgzf* z = new (std::nothrow) sid_bgzf;
    if (!z) return SID_ENOMEM;
    const uint8_t* p = (const uint8_t*)bytes;
    uint64_t off = 0, text = 0;
    try {
        while (off < len) {
            bgzf_member m;
            if (bgzf_member_parse(p + off, len - off, &m) != BGZF_OK) {
                if (err_offset) *err_offset = off;
                delete z;
                return SID_EBGZF;
            }
            z->blk.push_back(sid_bgzf_blk{off, text, m.bsize, m.isize});
            off += m.bsize;
            text += m.isize;
        }
    } catch (const std::bad_alloc&) {
        delete z;
        return SID_ENOMEM;
    }
    z->clen = len;
    z->tlen = text;
    *out = z;
    return SID_OK;
}

extern "C" size_t sid_bgzf_blocks(const sid_bgzf* z) { return z ? z->blk.size() : 0; }
extern "C" uint64_t sid_bgzf_text_len(const sid_bgzf* z) { return z ? z->tlen : 0; }
extern "C" int sid_bgzf_block(const sid_bgzf* z, size_t k, uint64_t* coff, uint32_t* csize, uint64_t* toff,
                              uint32_t* isize)
{
    if (!z || k >= z->blk.size()) return SID_EINVAL;
    const sid_bgzf_blk& b = z->blk[k];
    if (coff) *coff = b.coff;
    if (csize) *csize = b.csize;
    if (toff) *toff = b.toff;
    if (isize) *isize = b.isize;
    return SID_OK;
}
extern "C" void sid_bgzf_free(sid_bgzf* z) { delete z; }

int sid_bgzf_inflate_block(const uint8_t* p, uint32_t csize, uint32_t isize, uint8_t* out)
{
    bgzf_member m;
    if (bgzf_member_parse(p, csize, &m) != BGZF_OK || m.bsize != csize || m.isize != isize) return BGZF_EHEADER;
    bgzf_tables T;
    bgzf_host_out o{out, 0, isize};
    const int rc = bgzf_inflate(p + m.hdr, csize - m.hdr - 8, o, T);
    if (rc != BGZF_OK) return rc;
    return sid_crc32(0, out, isize) == m.crc ? BGZF_OK : BGZF_ECRC;
}

extern "C" int sid_bgzf_inflate_host(const void* bytes, size_t len, char* out, size_t cap, size_t* out_len,
                                     uint64_t* err_offset)
{
    if (out_len) *out_len = 0;
    sid_bgzf* z = nullptr;
    const int rc = sid_bgzf_index(bytes, len, &z, err_offset);
    if (rc != SID_OK) return rc;
    if (out_len) *out_len = z->tlen;
    int st = SID_OK;
    if (out && cap < z->tlen) st = SID_ENOMEM;
    if (out && st == SID_OK) {
        uint8_t none;
        for (const sid_bgzf_blk& b : z->blk) {
            uint8_t* dst = b.isize ? (uint8_t*)out + b.toff : &none;
            if (sid_bgzf_inflate_block((const uint8_t*)bytes + b.coff, b.csize, b.isize, dst) != BGZF_OK) {
                if (err_offset) *err_offset = b.coff;
                st = SID_EBGZF;
                break;
            }
        }
    }
    sid_bgzf_free(z);
    return st;
}
