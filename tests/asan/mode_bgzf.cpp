// sid_asan bgzf CORPUS — bgzf.cpp and the decoder core bgzf.h (the code the
// inflate kernel runs, host build: header parse, inflate, CRC32, the index)
// (tests/test_bgzf_asan.py).
//
// CORPUS is a sequence of cases: a line "Z <bytes>", then <bytes> bytes of a
// (possibly damaged) BGZF range and a newline.  Per case one line
// "rc err_offset blocks text_len crc32" -- sid_bgzf_inflate_host's status and
// offset, the index's counts (0 when it fails) and sid_crc32 of the text --
// then the text itself and a newline (nothing but the newline after an error).
// Input and output live in exact-size heap blocks: an access one byte outside
// either extent is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "harness.h"

int mode_bgzf(const std::string& all)
{
    size_t p = 0;
    while (p < all.size()) {
        const size_t nl = all.find('\n', p);
        if (nl == std::string::npos) return 3;
        unsigned long long nbytes = 0;
        if (std::sscanf(all.c_str() + p, "Z %llu", &nbytes) != 1) return 3;
        p = nl + 1;
        if (p + nbytes + 1 > all.size()) return 3;
        unsigned char* z = (unsigned char*)std::malloc(nbytes ? nbytes : 1);
        std::memcpy(z, all.data() + p, nbytes);
        p += nbytes + 1;
        sid_bgzf* idx = nullptr;
        uint64_t off = 0;
        size_t blocks = 0, need = 0;
        uint64_t text_len = 0;
        if (sid_bgzf_index(z, nbytes, &idx, &off) == SID_OK) {
            blocks = sid_bgzf_blocks(idx);
            text_len = sid_bgzf_text_len(idx);
            for (size_t k = 0; k < blocks; ++k) {
                uint64_t coff, toff;
                uint32_t csize, isize;
                if (sid_bgzf_block(idx, k, &coff, &csize, &toff, &isize) != SID_OK) return 4;
                if (coff + csize > nbytes || toff + isize > text_len) return 4;
            }
            sid_bgzf_free(idx);
        }
        int rc = sid_bgzf_inflate_host(z, nbytes, nullptr, 0, &need, &off);
        char* out = nullptr;
        size_t got = 0;
        if (rc == SID_OK) {
            if (need != text_len) return 4;
            out = (char*)std::malloc(need ? need : 1);
            if (need && sid_bgzf_inflate_host(z, nbytes, out, need - 1, &got, &off) != SID_ENOMEM) return 4;
            rc = sid_bgzf_inflate_host(z, nbytes, out, need, &got, &off);
        }
        std::free(z);
        if (rc != SID_OK) got = 0;
        std::printf("%d %llu %zu %llu %u\n", rc, (unsigned long long)off, blocks, (unsigned long long)text_len,
                    (unsigned)sid_crc32(0, out, got));
        if (got) std::fwrite(out, 1, got, stdout);
        std::fputc('\n', stdout);
        std::free(out);
    }
    return 0;
}
