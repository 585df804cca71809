// harness.h — what sid_asan's modes share (TEST INFRASTRUCTURE, CPU only).
//
// A mode is one function over the corpus bytes (driver.cpp read them) that
// returns the program's exit status: 0, 3 for a corpus format error, 4 for ABI
// misbehaviour, 5 for the sizing protocol.  Every block a mode hands to the
// product is an exact-size heap block: an access one byte outside it is a
// report.
#pragma once
#include <cstddef>
#include <string>

#include "sid.h"

int mode_bgzf(const std::string& corpus);
int mode_callable(const std::string& corpus);
int mode_context(const std::string& corpus);
int mode_depth(const std::string& corpus);
int mode_depth_hist(const std::string& corpus);
int mode_region_stats(const std::string& corpus);
int mode_regions(const std::string& corpus);
int mode_variants(const std::string& corpus);
int mode_vcf(const std::string& corpus);
int mode_windows(const std::string& corpus);

// The corpus of the parse-based modes: per case a line "T <bytes> <threads>"
// with `nextra` (at most 2) further integers, then <bytes> bytes of pileup
// text and a newline.  Per case: the text copied into an exact-size heap block,
// sid_parse_text, one line "rc err_line sites" (sites 0 after an error, when
// the handle must be null), and for a text that parsed fn(sites, count, the
// further integers).  The sites are freed after fn; a non-zero return of fn
// ends the run with that status.
typedef int (*text_case_fn)(sid_sites* s, size_t n, const int* extra);
int text_cases(const std::string& corpus, int nextra, text_case_fn fn);
