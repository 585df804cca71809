// strip.h — the host-side line stripper (strip.cpp): a pileup line's bytes
// behind its 5th token (the quality columns) are dropped before the text is
// uploaded, for the option sets that never read them.  Pure host C++, no HIP.
//
// A line is `chrom pos ref cov bases [quals [mapq]]`; tokens are separated by
// runs of ' ' / '\t', leading separators skipped (the reference's strtok_r,
// pileup.cpp:11-48).  The cut is the end of the 5th token: the byte after it
// is a separator or the newline, and the device parser ends the token at
// either, so no separator byte is kept.  A line is copied whole when it has
// fewer than five tokens, no final newline, or a byte below 0x20 other than
// '\t' in front of the cut (NUL and CR among them): the stripper is sound,
// not complete.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sid.h"

// the variants sid_strip_lines_impl takes (sid.h); SID_STRIP_AUTO picks the
// widest one the CPU runs
enum { SID_STRIP_AUTO = 0, SID_STRIP_SCALAR = 1, SID_STRIP_AVX2 = 2, SID_STRIP_AVX512 = 3 };

// The engine's form: whole lines in[0, n) stripped into out (64-B aligned, at
// least n + 64 bytes) through a cache-resident block, the bulk written with
// non-temporal stores.  After every `step` input bytes or so, at a line end,
// and at the end, the bytes so far are made visible (the partial 64-B line
// stored, a store fence) and tick(user, in_done, out_done, lines) is called:
// false stops the walk.  Returns the input bytes consumed.
typedef bool (*sid_strip_tick)(void* user, uint64_t in_done, uint64_t out_done, uint64_t lines);
uint64_t sid_strip_stream(const char* in, uint64_t n, char* out, uint64_t step, sid_strip_tick tick, void* user);
