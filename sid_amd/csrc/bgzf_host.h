// bgzf_host.h — the block index of a BGZF byte range as libsid's translation
// units share it (bgzf.cpp builds it; inflate.hip and run.cpp read it).
#pragma once

#include <vector>

#include "../../include/sid.h"
#include "bgzf.h"

struct sid_bgzf_blk {
    uint64_t coff;    // the member's offset in the compressed bytes
    uint64_t toff;    // its text's offset in the inflated text
    uint32_t csize;   // the member's bytes
    uint32_t isize;   // its text's bytes
};
struct sid_bgzf {
    std::vector<sid_bgzf_blk> blk;
    uint64_t clen = 0, tlen = 0;
};

// One member (its csize bytes at p) inflated into out (isize bytes), CRC
// checked: BGZF_OK or the decoder's status.
int sid_bgzf_inflate_block(const uint8_t* p, uint32_t csize, uint32_t isize, uint8_t* out);
