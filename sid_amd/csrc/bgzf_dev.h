// bgzf_dev.h — the device inflate's launcher (inflate.hip), as the engine
// (run.cpp) uses it underneath sid_bgzf_inflate_device.
#pragma once

#include <hip/hip_runtime.h>

#include "bgzf_host.h"

// one member of a launch: its bytes at d_in + coff, its text to d_out + ooff
// (ooff may be negative: the engine writes a chunk's first block in front of
// the chunk's first line)
struct sid_bgzf_dblk {
    uint64_t coff;
    int64_t ooff;
    uint32_t csize, isize;
};

// Stream-ordered, no sync: member k of the table inflated and CRC-checked by
// one wave, d_status[k] = its BGZF_* status, *d_bad = the lowest k whose status
// is not BGZF_OK, or 0xffffffff.
hipError_t sid_launch_bgzf_inflate(const uint8_t* d_in, const sid_bgzf_dblk* d_tab, uint32_t nblocks, uint8_t* d_out,
                                   uint32_t* d_status, uint32_t* d_bad, hipStream_t st);
