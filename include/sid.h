/*
 * sid.h — C ABI of libsid.so, the MI355X-native per-site genotype caller.
 *
 * Drop-in boundary.  EvolBioInf/sid has no plugin/FFI API; its internal seam
 * is the four method functions declared at call.hpp:40-43,
 *     std::vector<OutputRecord> callX(std::istream&, ...)
 * called only from sid.cpp:92-100.  This header replaces that seam with plain
 * pointers and sizes (no C++ or torch types), split where the data crosses the
 * host/device boundary:
 *
 *   host text --(sid_parse_*: pileup.cpp:13-153)--> SoA counts (u16 x 4 per site)
 *   counts --(sid_call_local / sid_profile_* + sid_lynch_* + sid_lookup_sites:
 *             call.cpp:62-289, lynch.hpp/.cpp, stats.cpp)--> code + 2 x f64 per site
 *   code + confs --(sid_format_csv: call.hpp:29-38, sid.cpp:102-105)--> CSV text
 *
 * Conventions
 *   - Caller owns every buffer.  "device" pointers are HIP device memory
 *     (hipMalloc / torch); "host" pointers are ordinary or pinned host memory.
 *   - No exception crosses the ABI: every function returns SID_OK (0) or a
 *     SID_E* status; sid_strerror() names it.
 *   - Device work is asynchronous on the caller's stream (hipStream_t passed as
 *     void*, NULL = default stream) unless the function says it synchronises.
 *   - One sid_ctx per device and host thread (thread-compatible, not
 *     thread-safe).
 *   - Per-site result code: bits 0-1 = gt[0] base (0..3 = A,C,G,T), bits 2-3 =
 *     gt[1] base, bit 7 = het label, bit 6 = site dropped (its profile was
 *     filtered, coverage < 4, and the reference prints no record for it:
 *     call.cpp:131-140).
 *   - Selection by label (sid_opts.select: SID_SELECT_ALL, _HET, _HOM): every
 *     formatter bound to a context -- the engine, sid_dtext_format and the
 *     chunk formatters behind them -- emits only the records whose label is
 *     the context's selection, byte for byte and in the order of the
 *     unselected output.  The calls and the Lynch estimate see every site;
 *     the per-site arrays (code / confs) are not changed by it.  Host
 *     formatting (sid_format_csv) takes no context: sid_select_mark marks the
 *     codes first.
 *   - Selection by region (sid_opts.regions, a sid_regions; NULL = every
 *     site): the same formatters emit only the records whose site lies inside
 *     the set -- its chrom field equals a set chrom byte for byte and start <
 *     pos <= end (BED: 0-based, half-open), pos being the integer the record
 *     prints -- byte for byte and in the order of the unselected output.  With
 *     a selection by label as well, a record is emitted when both hold.  The
 *     calls, the -R prior, the Lynch estimate and Benjamini-Hochberg see every
 *     site; the caller's per-site arrays are not changed.  sid_create and
 *     sid_engine_create copy what they need: the object may be freed right
 *     after.  Host formatting: sid_regions_mark marks the codes first.
 *   - Context (sid_opts.context = N, 0 .. 64; --context N): grep -C N over the
 *     unselected output.  Let U be the records u_0 .. u_(R-1) of the run
 *     without a selection, in file order (a site that prints no record has no
 *     index in U), and S the indices the selections by label and region keep.
 *     The same formatters then emit exactly the records u_i with
 *     min over s in S of |i - s| <= N, byte for byte and in U's order: every
 *     selected record with the N records before and after it.  The distance
 *     is in records, not sites or positions.  S empty: the header alone.
 *     Without a selection, or with N = 0, the output is what it is without
 *     the option.  Header, stderr, exit status, the calls, the -R prior, the
 *     Lynch estimate and Benjamini-Hochberg are unchanged, and the result does
 *     not depend on chunk size, device count, lanes, budgets or source kind.
 *     Any other N: SID_EINVAL from sid_create and sid_engine_create.  Host
 *     formatting: sid_context_mark, after the two marks above.
 *   - Windows (sid_opts.window = W, 0 = off, 1 .. 2^31-1; --windows W): a
 *     summary of the run along the input, beside the records.  The sites are the
 *     non-empty lines in file order; a site's chrom is its first token, its pos
 *     the integer its record prints (atoi: possibly 0 or negative) and its
 *     window index wi = floor((pos - 1) / W) in 64-bit signed arithmetic.  A row
 *     is a maximal run of consecutive sites with byte-equal chrom and equal wi:
 *     chrom; start = wi W and end = start + W (BED, as the region sets: the row
 *     holds the positions with start < pos <= end); sites, the lines of the
 *     run; records, those of them that print a record in the unselected output
 *     (the Lynch methods print none below coverage 4); het and hom, those
 *     records by label (records = het + hom).  Sorted input gives one row per
 *     window that has a site; a position that goes back or a chrom that
 *     returns opens a further row, as uniq -c would (no sorting, no hashing).
 *     Like the calls and the estimate the rows see every site: the selections
 *     by label and region and the context do not change them, and the option
 *     changes neither the records, stderr nor the exit status.  The rows do
 *     not depend on chunk size, device count, lanes, budgets, source kind or
 *     sink mode; a chunk counts once however often it is parsed.  A run that
 *     fails has no rows.  Any other W: SID_EINVAL from sid_create and
 *     sid_engine_create.  Host path: sid_windows_host, on the codes before any
 *     mark.
 *   - Variants (sid_opts.variants = 1; --variants): the records whose genotype
 *     is not the reference's.  For the site of a record, R is the single byte
 *     of its line's third token (the reference base, pileup.cpp:26-30),
 *     upper-cased as pileup.cpp:79 does (toupper, ASCII).  The record is a
 *     variant when (1) R is one of A, C, G, T, (2) the site has at least one
 *     counted base (a non-zero count in its profile_t) and (3) its gt field is
 *     not RR.  (2) is not decoration: -m local prints "hom,TT,1,1,p_value" for
 *     a site without a counted base -- depth 0, only '*', only '.' / ',' on an
 *     N reference -- whatever its reference.  The same formatters then emit only
 *     the variants, byte for byte and in U's order.  With a selection by label
 *     and / or region a record is emitted when all of them hold; with
 *     --context N, S is the set all of them keep; the window rows never change.
 *     Header, stderr, exit status, the calls, the -R prior, the Lynch estimate
 *     and Benjamini-Hochberg see every site and are unchanged; bytes_out stays
 *     exact in every sink mode, and the result does not depend on chunk size,
 *     device count, lanes, budgets, source kind or tile shape.  Any other
 *     value: SID_EINVAL from sid_create and sid_engine_create.  Host
 *     formatting: sid_variants_mark, before sid_context_mark.
 *   - Depth bounds (sid_set_depth / sid_engine_set_depth; --min-depth N,
 *     --max-depth N): the records of the sites whose coverage lies in a range.
 *     A site's depth is A + C + G + T of its profile_t as the parser stores it
 *     -- what sid_sites_counts / sid_dtext_counts report, the coverage
 *     call.cpp:66-70 compares with 4 -- not the pileup's fourth column: '*',
 *     'N', and '.' / ',' on a reference that is no base do not count.  The
 *     bounds are min (default 0) and max (default 0 = no upper bound); a record
 *     is emitted when min <= depth and (max == 0 or depth <= max).  Valid:
 *     0 <= min <= 262140 (4 x 65535), and max == 0 or min <= max <= 262140;
 *     anything else is SID_EINVAL.  min == 0 and max == 0 is the option switched
 *     off: every byte and every kernel as without it.  The same formatters
 *     then emit only those records, byte for byte and in U's order.  With a
 *     selection by label, region and / or variant a record is emitted when all
 *     of them hold; with --context N, S is the set all of them keep; the
 *     window rows never change.  Header, stderr, exit status, the calls, the -R
 *     prior, the Lynch estimate and Benjamini-Hochberg see every site and are
 *     unchanged; bytes_out stays exact in every sink mode, and the result does
 *     not depend on chunk size, device count, lanes, budgets, source kind or
 *     tile shape.  The Lynch methods print no record below coverage 4, so
 *     min <= 4 changes nothing there.  The bounds are no field of sid_opts
 *     (whose layout stands): they are set on a context or an engine.  Host
 *     formatting: sid_depth_mark, after the marks by label, region and variant
 *     and before sid_context_mark.
 *   - VCF (sid_set_format / sid_engine_set_format with SID_FORMAT_VCF; --vcf):
 *     what a record is, not which records exist.  The same formatters print a
 *     VCF line for exactly the sites that print a CSV record under the same
 *     options, in the same order -- the selections by label, region, variant
 *     and depth and the context decide which records exist, the format then
 *     applies to those -- and a line is a pure function of that CSV record, the
 *     site's reference byte and its depth.  Ten columns, tab-separated, '\n':
 *         CHROM POS . REF ALT . . DP=<d>;HOM=<hom_conf>;HET=<het_conf> GT <g>
 *     CHROM, POS: the bytes the CSV record prints; the position is the atoi
 *     integer, so it may be 0 or negative -- parity with the CSV wins over VCF
 *     validity.  REF: the single byte of the line's third token, upper-cased as
 *     pileup.cpp:79 does, when that is one of A, C, G, T; else N.  DP: the depth
 *     of the paragraph above (A + C + G + T of the profile_t), in decimal.  With
 *     DP = 0 (no counted base: the "hom,TT" placeholder of -m local) ALT is "."
 *     and <g> is "./.".  Otherwise, X and Y being the two bytes of the CSV's gt
 *     field: ALT is the distinct bytes among X, Y that differ from REF, X's
 *     first, joined by ','; none: ".".  Allele 0 is REF, the ALT alleles are 1
 *     and 2, and <g> is the allele numbers of X and Y, the smaller first, joined
 *     by '/': 0/0, 0/1, 1/1 or 1/2.  With REF N every counted base is an ALT.
 *     HOM, HET: the %g bytes of the CSV's hom_conf and het_conf fields, byte for
 *     byte (nan, -nan, inf as printed there).  The header (sid_vcf_header)
 *     replaces the CSV's header line; it has no ##contig lines, a pileup does
 *     not hold the chrom lengths.  stderr, the exit status, "nothing is written
 *     before the whole input has parsed", a failing run's empty output, the
 *     calls, the estimate, Benjamini-Hochberg and the window rows are
 *     unchanged; bytes_out stays exact in every sink mode, and the result does
 *     not depend on chunk size, device count, lanes, budgets, source kind or
 *     tile shape.  The format is no field of sid_opts (whose layout stands).
 *     Host formatting: sid_format_vcf in place of sid_format_csv, after the
 *     same marks.
 *   - Depth histogram (sid_engine_set_depth_hist; --depth-hist FILE): a summary
 *     of the run along the depth axis, beside the records.  The sites are the
 *     non-empty lines; a site's depth is the one the depth bounds use, A + C +
 *     G + T of its profile_t as the parser stores it (u16 counts that wrap),
 *     0 .. 262140.  There is one row for every depth that at least one site
 *     has, in ascending depth order: depth; sites; records, the sites that
 *     print a record in the unselected output; het and hom, those records by
 *     label (records = het + hom) -- the definitions of the window rows'
 *     columns, so for any W each of the four columns summed over the depth
 *     rows equals the same column summed over the window rows, and sites sums
 *     to sid_run_stats.sites.  Like the window rows, the calls and the
 *     estimate the rows see every site: the selections by label, region,
 *     variant and depth, the context and the record format never change them,
 *     and the option changes neither the records, bytes_out, stderr nor the
 *     exit status.  The rows do not depend on chunk size, device count, lanes,
 *     budgets, source kind, sink mode or tile shape; a chunk counts once
 *     however often it is parsed.  A run that fails has no rows; an engine
 *     that is reused starts every run from zero.  The switch is no field of
 *     sid_opts (whose layout stands).  Host path: sid_depth_hist_host, on the
 *     codes before any mark.
 *   - Region rows (sid_engine_set_region_stats; --region-stats FILE with
 *     --regions): a summary of the run along the region set, beside the
 *     records: one row for every interval of the set after its merge, exactly
 *     the intervals sid_regions_intervals counts, an interval without a site
 *     included.  The sites are the non-empty lines; a site's chrom, pos, depth,
 *     record and label are as in the paragraphs on windows and depth bounds:
 *     the atoi position, A + C + G + T of the stored profile_t, and the
 *     unselected code.  A site belongs to interval j when sid_regions_contains
 *     holds for it and j is the interval that holds it: chrom byte-equal, start
 *     < pos <= end.  The intervals are disjoint, so a site belongs to at most
 *     one; sites outside every interval count nowhere.  The columns: chrom,
 *     start, end (the interval, BED); sites; depth, the sum of the sites'
 *     depths in 64 bits (what samtools bedcov prints); records, the sites that
 *     print a record in the unselected output; het and hom, those records by
 *     label (records = het + hom).  Row order: the chroms in the order of their
 *     first non-empty interval in the source (BED line order; array order for
 *     sid_regions_from_intervals), a chrom's intervals ascending by start --
 *     sid_regions_interval enumerates them; the device's flat table keeps its
 *     own order, (first 8 bytes, length, bytes), byte for byte what it was.
 *     Like the other summaries the rows see every site: the selections by
 *     label, variant and depth, the context and the record format never change
 *     them; the region set is where the intervals come from, and its selection
 *     of the records does not change what the rows count; the option changes
 *     neither the records, bytes_out, stderr nor the exit status.  The rows do
 *     not depend on chunk size, device count, lanes, budgets, source kind, sink
 *     mode or tile shape; a chunk counts once however often it is parsed.  A
 *     run that fails has no rows; an engine that is reused starts every run
 *     from zero.  A set of more than SID_REGION_STATS_MAX = 2^20 merged
 *     intervals is refused when the option is switched on
 *     (sid_region_stats_valid): a memory budget -- the device's per-chunk table
 *     and its two row sets take 24 bytes an interval each, 72 MiB a workspace
 *     at the cap -- not a measured figure; a finer tiling is what the windows
 *     are for.  By construction sites sums to the number of sites for which
 *     sid_regions_contains is true, records to the records of a run whose only
 *     selection is the set, het to its het records.  The switch is no field of
 *     sid_opts (whose layout stands).  Host path: sid_region_stats_host, on
 *     the codes before any mark; over a resident shard:
 *     sid_dtext_region_stats.
 *   - Callable runs (sid_callable_host, sid_dtext_callable; --callable FILE
 *     with --host-parse): the positions where a call could be made, as BED
 *     rows beside the records.  The sites
 *     are the non-empty lines in file order; a site's chrom, pos, depth and
 *     record are as in the paragraphs on windows and depth bounds.  A site is
 *     callable when (1) it prints a record in the unselected output -- its
 *     unselected code has no SID_CODE_DROPPED; the Lynch methods print none
 *     below coverage 4 -- (2) its depth d satisfies d >= 1 and min <= d and
 *     (max == 0 or d <= max), with the depth bounds in force for the run
 *     (sid_set_depth, or the host path's arguments; the default (0, 0)
 *     leaves d >= 1, which keeps out -m local's "hom,TT" placeholder for a site without a
 *     counted base), and (3) pos >= 1: the atoi position may be 0 or negative,
 *     a BED start cannot.  A row is a maximal run of consecutive sites, with no
 *     site of any kind between them in file order, that are all callable, whose
 *     chroms are byte-equal and where each pos is the previous pos + 1,
 *     compared in 64 bits (2^31-1 has no successor).  Its fields: chrom; start
 *     = first pos - 1 and end = last pos (BED, as the region sets use it; end -
 *     start is the run's sites); het, the run's het records.  No sorting and
 *     no hashing: a repeated position, a position that goes back, a chrom that
 *     returns or a non-callable site in between each opens a further row, as
 *     uniq would, and two rows may abut or overlap.  The file has one line
 *     "chrom\tstart\tend\thet\n" per row, integers in decimal, and no header
 *     line.  The depth bounds are part of the definition (the ones that also
 *     choose the records); otherwise, like the window rows, the rows see every site: the
 *     selections by label, region and variant, the context and the record
 *     format never change them, and the option changes neither the records,
 *     bytes_out, stderr nor the exit status.  The rows do not depend on how
 *     the sites are cut into ranges: sid_callable_join and the stitch of
 *     per-range lists (callable.h) give the rows of the whole.  A run that
 *     fails has no rows.  Host path: sid_callable_host, on the codes before
 *     any mark; on the device: sid_dtext_callable over a resident shard.  The
 *     streaming engine does not produce the rows yet.
 *   - Counts layout: profile_t (pileup.hpp:7) = 4 x uint16 {A,C,G,T} per site,
 *     array of structures, 8 bytes per site.
 */
#ifndef SID_H
#define SID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status -- */
enum {
    SID_OK = 0,
    SID_EINVAL = 1,      /* bad argument (null pointer, misuse)                     */
    SID_EHIP = 2,        /* HIP runtime error (sid_last_hip_error() has the code)   */
    SID_ENOMEM = 3,      /* host or device allocation failed                        */
    SID_EMALFORMED = 4,  /* "Malformed pileup line"                pileup.cpp:9       */
    SID_EMISSING_MQ = 5, /* "Malformed pileup line or missing mapping qualities" :10 */
    SID_ENULLCHROM = 6,  /* no first token: the reference assigns a NULL char* to a
                            std::string (pileup.cpp:18) and dies with SIGSEGV       */
    SID_ESTATE = 7,      /* call order violated (e.g. lookup before lynch_prepare)  */
    SID_EBADFUNC = 8,    /* non-finite objective at the simplex start: GSL would
                            abort (nmsimplex2 set; optimization.hpp:55)            */
    SID_EEMPTY = 9,      /* no profile with coverage >= 4: the reference indexes an
                            empty vector in adjustBenjaminiHochberg (stats.cpp:73) */
    SID_EIO = 10,        /* the output callback reported a write failure            */
    SID_ERANGE = 11,     /* a confidence outside the device formatter's range
                            (|v| >= 2^63; p-values and posteriors never are)        */
    SID_ENOBQ = 12,      /* -m quality, no base-quality field: parseQualities(NULL)
                            dereferences NULL (pileup.cpp:54,158): SIGSEGV          */
    SID_ELINE = 13,      /* a line that makes a chunk span 4 GiB or more (line
                            offsets on the device are 32-bit)                      */
    SID_EBGZF = 14,      /* not a BGZF file, or a truncated or corrupt BGZF block   */
};
const char* sid_strerror(int status);
int sid_last_hip_error(void);
/* Library version string, e.g. "sid-mi355x 0.1.0 (gfx950)". */
const char* sid_version(void);

/* --------------------------------------------------------------- options -- */
/* per-site result code bits (see Conventions) */
#define SID_CODE_HET 0x80
#define SID_CODE_DROPPED 0x40

enum { SID_METHOD_LOCAL = 0, SID_METHOD_LIKELIHOOD_RATIO = 1, SID_METHOD_BAYES = 2, SID_METHOD_QUALITY = 3 };
/* which records a formatter emits, by their label field (--only) */
enum { SID_SELECT_ALL = 0, SID_SELECT_HET = 1, SID_SELECT_HOM = 2 };

/* GlobalOptions, sid.cpp:11-17 */
typedef struct {
    int method;                  /* -m   (default SID_METHOD_LOCAL)                */
    int estimate_prior;          /* -R   (default 0)                               */
    double snp_prior;            /* -r   (default -1 = no prior)                   */
    double significance_level;   /* -p   (default 0.05)                            */
    double site_error_threshold; /* -E   (default 0.1)                             */
    int select;                  /* --only (default SID_SELECT_ALL): the records
                                    emitted, by label; sid_create and
                                    sid_engine_create return SID_EINVAL for any
                                    other value                                    */
    int variants;                /* --variants (default 0): 1 = only the records
                                    whose genotype is not homozygous reference are
                                    emitted (Conventions); any other value:
                                    SID_EINVAL.  It takes the four bytes that were
                                    padding in front of the pointer below: the
                                    structure's size and every other field's
                                    offset are as before, `window` stays last      */
    const struct sid_regions* regions; /* --regions (default NULL = every site): the
                                    records emitted, by (chrom, pos); see
                                    sid_regions_* below                            */
    int context;                 /* --context (default 0): with a selection, the N
                                    records before and after every selected record
                                    are emitted too (0 .. 64, else SID_EINVAL)      */
    int window;                  /* --windows (default 0 = off): the window size of
                                    the per-window summary (sid_engine_windows);
                                    negative: SID_EINVAL                            */
} sid_opts;
void sid_opts_default(sid_opts* o);
/* Sets SID_CODE_DROPPED on the n host codes whose label is not `select`, so
 * that sid_format_csv skips them (SID_SELECT_ALL: nothing changes).
 * SID_EINVAL for another value of select or a NULL code with n != 0. */
int sid_select_mark(uint8_t* code /* host */, size_t n, int select);
/* The context on the host path (the analogue of sid_select_mark and
 * sid_regions_mark, after them).  code_all: the n codes before any selection
 * marked them -- the sites without SID_CODE_DROPPED are U's records; code: the
 * codes after the marks -- its sites without SID_CODE_DROPPED are S.  Clears
 * SID_CODE_DROPPED in code for every record of U within `context` records of
 * one of S.  SID_EINVAL for a NULL pointer with n != 0 or a context outside
 * 0 .. 64. */
#define SID_CONTEXT_MAX 64
int sid_context_mark(const uint8_t* code_all /* host */, uint8_t* code /* host */, size_t n, int context);

/* ---------------------------------------------------------- region sets --
 * A set of (chrom, start, end) intervals in BED convention (0-based,
 * half-open), merged per chrom into sorted, disjoint intervals; a site is
 * inside when its chrom equals a set chrom byte for byte and start < pos <=
 * end.  A set without a non-empty interval is valid and holds nothing.
 *
 * sid_regions_from_bed: BED text.  Lines end in '\n' (a final line without
 *   one counts); empty lines and lines starting with '#', "track" or
 *   "browser" are skipped; fields are separated by runs of space or tab.
 *   Three or more fields: chrom start end (the rest ignored), start and end
 *   decimal with 0 <= start <= end, an end above 2^31-1 clamped, start == end
 *   an empty interval.  One field: the whole chromosome, 0 .. 2^31-1.
 *   Anything else (two fields, a sign, a non-digit, start > end): SID_EINVAL
 *   and the 1-based line number in *err_line.
 * sid_regions_from_intervals: n intervals from arrays (SID_EINVAL for a NULL
 *   or empty chrom, one holding a space, tab or newline, start < 0 or start >
 *   end).
 * sid_regions_intervals / _chroms: the intervals after the merge, and the
 *   chroms that own at least one.
 * sid_regions_contains: 1 / 0, on the host.
 * sid_regions_mark: sets SID_CODE_DROPPED on the host codes code[begin, end)
 *   of the sites outside (regions == NULL: nothing changes), so that
 *   sid_format_csv skips them -- the analogue of sid_select_mark. */
typedef struct sid_regions sid_regions;
struct sid_sites;
int sid_regions_from_bed(const char* text, size_t len, sid_regions** out, uint64_t* err_line);
int sid_regions_from_intervals(const char* const* chrom, const int32_t* start, const int32_t* end, size_t n,
                               sid_regions** out);
size_t sid_regions_intervals(const sid_regions* r);
size_t sid_regions_chroms(const sid_regions* r);
int sid_regions_contains(const sid_regions* r, const char* chrom, size_t chrom_len, int32_t pos);
void sid_regions_free(sid_regions* r);
int sid_regions_mark(const sid_regions* r, const struct sid_sites* s, size_t begin, size_t end,
                     uint8_t* code /* host */);
/* The variants on the host path (Conventions): sets SID_CODE_DROPPED on the
 * host codes code[begin, end) of the sites that are no variant -- the analogue
 * of sid_regions_mark, before sid_context_mark.  SID_EINVAL for a range outside
 * the sites or a NULL pointer. */
int sid_variants_mark(const struct sid_sites* s, size_t begin, size_t end, uint8_t* code /* host */);
/* The depth bounds on the host path (Conventions): sets SID_CODE_DROPPED on the
 * host codes code[begin, end) of the sites whose depth is below min or, with
 * max != 0, above max -- after the marks by label, region and variant, before
 * sid_context_mark.  SID_EINVAL for bounds outside the Conventions', a range
 * outside the sites or a NULL pointer. */
#define SID_DEPTH_MAX 262140
int sid_depth_mark(const struct sid_sites* s, size_t begin, size_t end, int min, int max, uint8_t* code /* host */);

/* -------------------------------------------------------------- windows --
 * The rows of the windowed summary (Conventions).  chrom is not NUL-terminated.
 *
 * sid_windows_host: the rows of sites [begin, end) on the host path (the
 *   analogue of sid_select_mark and its siblings): code_all are the codes
 *   before any selection marked them.  *rows is freed with sid_windows_free.
 *   SID_EINVAL for a window outside 1 .. 2^31-1, a range outside the sites or
 *   a NULL pointer.
 * sid_windows_format: "chrom,start,end,sites,records,het,hom\n" (with_header)
 *   and a line per row, the integers in decimal.  Returns bytes written in
 *   *len, or SID_ENOMEM if cap is too small (then *len is a sufficient size),
 *   as sid_format_csv. */
typedef struct {
    const char* chrom;
    uint32_t chrom_len;
    int64_t start, end;
    uint64_t sites, records, het, hom;
} sid_window;
int sid_windows_host(const struct sid_sites* s, size_t begin, size_t end, const uint8_t* code_all /* host */,
                     int window, sid_window** rows, size_t* n);
void sid_windows_free(sid_window* rows);
int sid_windows_format(const sid_window* rows, size_t n, int with_header, char* buf, size_t cap, size_t* len);

/* ------------------------------------------------------- depth histogram --
 * The rows of the depth histogram (Conventions), in ascending depth order.
 *
 * sid_depth_hist_host: the rows of sites [begin, end) on the host path (the
 *   analogue of sid_windows_host): code_all are the codes before any selection
 *   marked them.  *rows is freed with sid_depth_hist_free.  SID_EINVAL for a
 *   range outside the sites or a NULL pointer.
 * sid_depth_hist_format: "depth,sites,records,het,hom\n" (with_header) and a
 *   line per row, the integers in decimal.  Returns bytes written in *len, or
 *   SID_ENOMEM if cap is too small (then *len is a sufficient size), as
 *   sid_windows_format.
 * sid_depth_hist_merge: the sum of two row sets (ranks that took site ranges
 *   add their rows with it); *rows is freed with sid_depth_hist_free.
 *   SID_EINVAL for a NULL pointer or input that is not strictly ascending in
 *   depth. */
typedef struct {
    uint64_t sites, records, het, hom;
    uint32_t depth;
    uint32_t pad;
} sid_depth_row;
int sid_depth_hist_host(const struct sid_sites* s, size_t begin, size_t end, const uint8_t* code_all /* host */,
                        sid_depth_row** rows, size_t* n);
void sid_depth_hist_free(sid_depth_row* rows);
int sid_depth_hist_format(const sid_depth_row* rows, size_t n, int with_header, char* buf, size_t cap, size_t* len);
int sid_depth_hist_merge(const sid_depth_row* a, size_t na, const sid_depth_row* b, size_t nb, sid_depth_row** rows,
                         size_t* n);

/* ----------------------------------------------------------- region rows --
 * The region rows (Conventions), one per merged interval in the set's source
 * order.  chrom is not NUL-terminated.
 *
 * sid_regions_interval: interval j (0 .. sid_regions_intervals - 1) of the set
 *   in row order; *chrom points into the set.  Any out pointer may be NULL.
 *   SID_EINVAL for a NULL set or j out of range.
 * sid_region_stats_valid: SID_OK when the option can be switched on for the
 *   set, SID_EINVAL for NULL or more than SID_REGION_STATS_MAX intervals.
 * sid_region_stats_host: the rows of sites [begin, end) on the host path (the
 *   analogue of sid_depth_hist_host): code_all are the codes before any
 *   selection marked them.  *n is sid_regions_intervals.  *rows is freed with
 *   sid_region_stats_free and holds its own copy of the names.  SID_EINVAL for
 *   a NULL set, a range outside the sites or a NULL pointer.
 * sid_region_stats_format: "chrom,start,end,sites,depth,records,het,hom\n"
 *   (with_header) and a line per row, the integers in decimal.  Returns bytes
 *   written in *len, or SID_ENOMEM if cap is too small (then *len is a
 *   sufficient size), as sid_depth_hist_format.
 * sid_region_stats_merge: the elementwise sum of two lists of n rows over the
 *   same set (ranks that took site ranges add their rows with it); *rows is
 *   freed with sid_region_stats_free.  SID_EINVAL for a NULL pointer or two
 *   lists whose keys (chrom, start, end) differ in any row. */
#define SID_REGION_STATS_MAX (1u << 20)
typedef struct {
    const char* chrom;
    uint32_t chrom_len;
    int64_t start, end;
    uint64_t sites, depth, records, het, hom;
} sid_region_row;
int sid_regions_interval(const sid_regions* r, size_t j, const char** chrom, uint32_t* chrom_len, int64_t* start,
                         int64_t* end);
int sid_region_stats_valid(const sid_regions* r);
int sid_region_stats_host(const sid_regions* r, const struct sid_sites* s, size_t begin, size_t end,
                          const uint8_t* code_all /* host */, sid_region_row** rows, size_t* n);
void sid_region_stats_free(sid_region_row* rows);
int sid_region_stats_format(const sid_region_row* rows, size_t n, int with_header, char* buf, size_t cap, size_t* len);
int sid_region_stats_merge(const sid_region_row* a, const sid_region_row* b, size_t n, sid_region_row** rows);

/* -------------------------------------------------------- callable runs --
 * The rows of the callable runs (Conventions), in file order.
 *
 * sid_callable_host: the rows of sites [begin, end) on the host path: code_all
 *   are the codes before any selection marked them, (min, max) the depth
 *   bounds.  *rows is freed with sid_callable_free.  SID_EINVAL for a range
 *   outside the sites, a NULL pointer, or bounds that sid_depth_mark refuses.
 * sid_callable_format: "chrom\tstart\tend\thet\n" per row, no header line.
 *   Returns bytes written in *len, or SID_ENOMEM if cap is too small (then
 *   *len is a sufficient size), as sid_windows_format.
 * sid_callable_join: two row lists that are neighbours in file order (ranks
 *   that took site ranges): a's rows, then b's, the boundary rows merged into
 *   one only when a_open_end and b_open_start are both set -- a's last site
 *   lies in its last row and b's first site in its first row -- the chroms are
 *   equal and b's start == a's end.  *rows is freed with sid_callable_free. */
typedef struct {
    const char* chrom; /* chrom_len bytes, not terminated */
    uint32_t chrom_len;
    uint32_t pad;
    int64_t start, end;
    uint64_t het;
} sid_callable_row;
int sid_callable_host(const struct sid_sites* s, size_t begin, size_t end, const uint8_t* code_all /* host */, int min,
                      int max, sid_callable_row** rows, size_t* n);
void sid_callable_free(sid_callable_row* rows);
int sid_callable_format(const sid_callable_row* rows, size_t n, char* buf, size_t cap, size_t* len);
int sid_callable_join(const sid_callable_row* a, size_t na, int a_open_end, const sid_callable_row* b, size_t nb,
                      int b_open_start, sid_callable_row** rows, size_t* n);

/* ------------------------------------------------------------- contexts -- */
typedef struct sid_ctx sid_ctx;
struct sid_bgzf;
int sid_device_count(int* n);
/* Binds `device` (hipSetDevice) for the calling thread and builds the
 * per-context constant tables (log table, chi-square constants). */
int sid_create(int device, const sid_opts* opts, sid_ctx** out);
int sid_destroy(sid_ctx* ctx);
/* Replaces snp_prior after the -R estimate (call.cpp:223-234). */
int sid_set_prior(sid_ctx* ctx, double snp_prior);
/* The depth bounds (Conventions) of every formatter call made on the context
 * after it (sid_dtext_format and the chunk formatters behind it); (0, 0)
 * switches them off again.  SID_EINVAL for bounds outside the Conventions'. */
int sid_set_depth(sid_ctx* ctx, int min, int max);
/* The record format (Conventions, "VCF") of every formatter call made on the
 * context after it (sid_dtext_format and the chunk formatters behind it).
 * SID_EINVAL for any other value. */
enum { SID_FORMAT_CSV = 0, SID_FORMAT_VCF = 1 };
int sid_set_format(sid_ctx* ctx, int format);

/* ------------------------------------------------------- -m local (a5-a8) --
 * Per-site replacement of callSiteMLError's per-profile loop + per-site gather
 * (call.cpp:213-289; likelihoods lynch.hpp:48-55,76-80,92-96; LRT
 * stats.cpp:29-37).  counts/code/hom_conf/het_conf are device pointers. */
int sid_call_local(sid_ctx* ctx, const uint16_t* counts, size_t n, uint8_t* code,
                   double* hom_conf, double* het_conf, void* stream);

/* Measurement (bench.py): while enabled, sid_call_local records HIP events on
 * its stream around its main (class-table) kernel and its fix-up kernel.
 * sid_timing_read synchronises on them, returns the per-call averages of
 * the calls since the previous read, and resets. */
int sid_timing_enable(sid_ctx* ctx, int enable);
int sid_timing_read(sid_ctx* ctx, uint64_t* calls, double* main_ms, double* fixup_ms);

/* ---------------------------------------------- Lynch path (a11-a17) -------
 * 1. sid_profile_reset + sid_profile_accumulate (any number of batches):
 *    device hash histogram of the site profiles (countUniqueProfiles,
 *    pileup.cpp:169-196).
 * 2. optional multi-device / multi-rank merge: sid_profile_table exports the
 *    sorted unique profiles (cached until the histogram changes),
 *    sid_profile_load replaces the context's table by a merged one: the
 *    concatenated per-device tables may repeat keys, it sorts them and sums
 *    the counts of equal keys itself.
 * 3. sid_lynch_prepare: coverage >= 4 filter (call.cpp:66-70), nucleotide
 *    distribution (pileup.cpp:198-217), Nelder-Mead estimate of (pi, eps)
 *    with the objective evaluated on the GPU (lynch.cpp:17-61,
 *    optimization.hpp:50-89), per-profile 10-genotype likelihoods at eps-hat
 *    (lynch.hpp:57-74,82-90), then the per-method class table:
 *    likelihood_ratio: LRT + Benjamini-Hochberg (call.cpp:85-127,
 *    stats.cpp:58-80); bayes: posteriors (call.cpp:170-194); local -R: only
 *    the prior (use sid_set_prior + sid_call_local afterwards).
 * 4. sid_lookup_sites: per-site gather of the class table (call.cpp:129-140). */
typedef struct {
    double heterozygosity;   /* pi-hat   ("# heterozygosity: %e", call.cpp:79)   */
    double error_rate;       /* eps-hat  ("# error: %e", call.cpp:80)            */
    double fval;             /* objective at the returned vertex                */
    double dist[4];          /* nucleotide distribution                         */
    int iterations;          /* NM iterations (optimization.hpp:70)             */
    int converged;           /* 0: "did not converge in 1000 iterations"        */
    uint64_t evaluations;    /* objective evaluations                           */
    uint64_t n_unique;       /* profiles after the coverage filter ("# unique profiles") */
} sid_estimate;

int sid_profile_reset(sid_ctx* ctx, void* stream);
int sid_profile_accumulate(sid_ctx* ctx, const uint16_t* counts, size_t n, void* stream);
/* Synchronises.  keys[i] = A<<48 | C<<32 | G<<16 | T (numeric order ==
 * lexicographic profile_t order); counts64[i] = sites with that profile.
 * With keys == NULL only *u is returned. */
int sid_profile_table(sid_ctx* ctx, uint64_t* keys, uint64_t* counts64, size_t cap, size_t* u);
int sid_profile_load(sid_ctx* ctx, const uint64_t* keys, const uint64_t* counts64, size_t u);
/* Objective -sum count*log((1-pi)Lhom+pi*Lhet) over the filtered table at
 * (pi, eps), lynch.cpp:37-61.  Valid after sid_lynch_prepare (or
 * sid_lynch_setup).  Synchronises. */
int sid_lynch_setup(sid_ctx* ctx, sid_estimate* est /* dist, n_unique filled */);
int sid_lynch_objective(sid_ctx* ctx, double pi, double eps, double* out);
/* verbose != 0 prints the reference's "# ..." stderr lines. Synchronises.
 * -m bayes with no profile of coverage >= 4 succeeds and drops every site
 * (callBayes prints the header only); likelihood_ratio returns SID_EEMPTY. */
int sid_lynch_prepare(sid_ctx* ctx, int verbose, sid_estimate* est);
/* The same with (pi-hat, eps-hat) taken from `given` (an estimate another
 * device or rank computed on the same merged table, SURVEY.md §8(e) steps
 * 3-4): no Nelder-Mead here, only the per-profile classification.  Prints
 * only the "# unique profiles" line when verbose. */
int sid_lynch_prepare_given(sid_ctx* ctx, int verbose, const sid_estimate* given, sid_estimate* est);
int sid_lookup_sites(sid_ctx* ctx, const uint16_t* counts, size_t n, uint8_t* code,
                     double* hom_conf, double* het_conf, void* stream);

/* ----------------------------------------------------- synthetic input -----
 * Counter-based generator (BASELINE.md "Synthetic generator"): site i of a
 * run is a pure function of (seed, first_site + i), identical on host and
 * device.  sites_per_chrom splits the run into chromosomes chr1, chr2, ...
 * (positions restart at 1; keeps positions < 2^31). */
int sid_synth_counts(sid_ctx* ctx, uint64_t seed, double mean_depth, uint64_t first_site,
                     size_t n, uint16_t* counts /* device */, void* stream);
/* The same text generated on the device into out (cap bytes, device memory),
 * stream-ordered, then synchronised: *len = its bytes; SID_ERANGE when they
 * exceed cap (then out holds no usable text). */
int sid_synth_text_device(sid_ctx* ctx, uint64_t seed, double mean_depth, uint64_t first_site, size_t n,
                          uint64_t sites_per_chrom, char* out /* device */, size_t cap, size_t* len, void* stream);
/* Host text of sites [first_site, first_site+n).  Returns the bytes needed in
 * *len; writes at most cap bytes (call with buf == NULL to size). */
int sid_synth_text(uint64_t seed, double mean_depth, uint64_t first_site, size_t n,
                   uint64_t sites_per_chrom, char* buf, size_t cap, size_t* len);
/* The same text with a 7th column of mapping qualities (samtools mpileup -s,
 * uniform 0..60 per read), as the quality method requires. */
int sid_synth_text_mq(uint64_t seed, double mean_depth, uint64_t first_site, size_t n,
                      uint64_t sites_per_chrom, char* buf, size_t cap, size_t* len);
/* Host counts of the same sites (for tests; no GPU needed). */
int sid_synth_counts_host(uint64_t seed, double mean_depth, uint64_t first_site, size_t n,
                          uint16_t* counts);

/* ------------------------------------------------------ host parser --------
 * parsePileupLine / parseReadBases semantics (pileup.cpp:13-153) over a text
 * buffer, multi-threaded.  Empty lines are skipped (call.cpp:14).  On a
 * malformed line the status is SID_EMALFORMED / SID_ENULLCHROM and
 * *err_line is the 0-based line number of the first bad line. */
typedef struct sid_sites sid_sites;
int sid_parse_text(const char* text, size_t len, int nthreads, sid_sites** out,
                   uint64_t* err_line);
void sid_sites_free(sid_sites* s);
size_t sid_sites_count(const sid_sites* s);
const uint16_t* sid_sites_counts(const sid_sites* s);   /* host, n x 4          */
const int32_t* sid_sites_positions(const sid_sites* s); /* host, n              */
/* The reference base of every site: the byte of its line's third token, as it
 * stands in the text (not upper-cased). */
const uint8_t* sid_sites_refs(const sid_sites* s);      /* host, n              */
/* Chromosome runs: segment k covers sites [start_k, start_{k+1}). */
size_t sid_sites_chrom_segments(const sid_sites* s);
const char* sid_sites_chrom_name(const sid_sites* s, size_t k, uint64_t* start);

/* ------------------------------------------------------ line stripper ------
 * A copy of a pileup text without the columns that only -m quality reads: of
 * every line, the bytes from the end of its 5th token (tokens on runs of ' ' /
 * '\t', leading ones skipped, as the reference's strtok_r) up to, not
 * including, its newline are dropped.  A line is copied whole when it has
 * fewer than five tokens, no final newline, or a byte below 0x20 other than
 * '\t' in front of the cut.  For -m local, likelihood_ratio and bayes the
 * stripped text gives the output, warnings and errors of the original.
 *
 * sid_strip_lines: in[0, n) into out (cap >= n, no overlap); returns the bytes
 *   written ((size_t)-1: cap < n or a NULL buffer) and in *lines (may be NULL)
 *   the lines copied, an unterminated last one included.  The widest variant
 *   the CPU runs; all variants write the same bytes.
 * sid_strip_lines_impl: one variant (1 scalar, 2 AVX2, 3 AVX-512; 0 as
 *   above); (size_t)-1 when this CPU does not run it.  sid_strip_impl: the
 *   variant 0 stands for.
 * sid_strip_map: the offset in in[0, n) of the byte that sid_strip_lines
 *   writes at out_off (a stripped line's newline: the input line's newline;
 *   out_off at or past the output's end: n). */
size_t sid_strip_lines(const char* in, size_t n, char* out, size_t cap, uint64_t* lines);
size_t sid_strip_lines_impl(int impl, const char* in, size_t n, char* out, size_t cap, uint64_t* lines);
int sid_strip_impl(void);
size_t sid_strip_map(const char* in, size_t n, size_t out_off);

/* ------------------------------------------------------ CSV emitter --------
 * Formats records [begin, end) exactly like operator<<(OutputRecord)
 * (call.hpp:29-38: chrom,pos,label,gt,%g,%g,conf_type) into buf; sites with
 * code bit 6 set are skipped.  conf_type: "p_value" or "probability".
 * Returns bytes written in *len, or SID_ENOMEM if cap is too small (then *len
 * is a sufficient size). */
int sid_format_csv(const sid_sites* s, size_t begin, size_t end, const uint8_t* code,
                   const double* hom_conf, const double* het_conf, const char* conf_type,
                   char* buf, size_t cap, size_t* len);
/* The same records as VCF lines (Conventions, "VCF"): a line for exactly the
 * sites sid_format_csv prints a record for (code bit 6 set: skipped), REF from
 * sid_sites_refs and DP from the counts.  Sized as sid_format_csv: SID_ENOMEM
 * and a sufficient *len when cap is too small.  SID_EINVAL for a NULL pointer,
 * a range outside the sites, or sites that carry no reference bytes. */
int sid_format_vcf(const sid_sites* s, size_t begin, size_t end, const uint8_t* code,
                   const double* hom_conf, const double* het_conf, char* buf, size_t cap, size_t* len);
/* The VCF header of a run with these options, in place of the CSV's header
 * line: "##fileformat=VCFv4.2", "##source=" + sid_version(), an ##INFO line
 * each for DP (Integer), HOM and HET (Float), "##sidConfType=p_value" or
 * "probability" (the CSV's seventh column: probability for SID_METHOD_BAYES),
 * the ##FORMAT line of GT and the "#CHROM ... SAMPLE" line.  No NUL is
 * written.  Sized as sid_format_csv; SID_EINVAL for a NULL opts or len. */
int sid_vcf_header(const sid_opts* opts, char* buf, size_t cap, size_t* len);
/* %g formatting of one double exactly as std::ostream does (precision 6). */
int sid_format_double(double v, char* buf, size_t cap);

/* ------------------------------------ device text path
 * The same parse and the same CSV, on the device: the text of one shard is
 * copied to HBM, indexed (line starts) and parsed there, and stays resident
 * (the formatter re-reads chrom and pos from it).
 *
 * sid_dtext_parse: host text -> device counts (sid_dtext_counts, 4 x u16 per
 *   non-empty line, as sid_parse_text).  Synchronises.  `chunk` (0 = 256 MiB)
 *   is the size of the individual host-to-device copies.  On a malformed line
 *   returns SID_EMALFORMED or SID_ENULLCHROM for the first one in file order
 *   and its byte offset in *err_offset; *out stays NULL.
 * sid_dtext_format: the records of sites [begin, end) with the given device
 *   code/confs, formatted on the device and handed to write() in order, in
 *   pieces valid only during the call (write returns 0, else SID_EIO).
 *   Synchronises. */
typedef struct sid_dtext sid_dtext;
typedef int (*sid_write_fn)(void* user, const char* bytes, size_t len);
int sid_dtext_parse(sid_ctx* ctx, const char* text, size_t len, size_t chunk, sid_dtext** out,
                    uint64_t* err_offset, void* stream);
/* The same for bytes [offset, offset+len) of an open file (offset at a line
 * start): `threads` host threads (0 = 8) pread() into pinned staging owned by
 * the context, each buffer DMA'd to HBM as it fills -- no file mapping. */
int sid_dtext_parse_fd(sid_ctx* ctx, int fd, uint64_t offset, uint64_t len, int threads, sid_dtext** out,
                       uint64_t* err_offset, void* stream);
size_t sid_dtext_count(const sid_dtext* t);
const uint16_t* sid_dtext_counts(const sid_dtext* t);   /* device */
int sid_dtext_format(sid_ctx* ctx, const sid_dtext* t, size_t begin, size_t end, const uint8_t* code,
                     const double* hom_conf, const double* het_conf, const char* conf_type,
                     sid_write_fn write, void* user, void* stream);
int sid_dtext_free(sid_dtext* t);
/* The windowed summary (Conventions; the context's sid_opts.window, else
 * SID_ESTATE) of sites [begin, end) of a resident shard with the given device
 * codes: the window stage of the engine over one range, without chunk edges.
 * *rows is freed with sid_windows_free.  Synchronises. */
int sid_dtext_windows(sid_ctx* ctx, const sid_dtext* t, size_t begin, size_t end, const uint8_t* code /* device */,
                      sid_window** rows, size_t* n, void* stream);
/* The depth histogram (Conventions) of sites [begin, end) of a resident shard
 * with the given device codes: the engine's stage over one range.  It needs no
 * switch on the context.  *rows is freed with sid_depth_hist_free.
 * Synchronises. */
int sid_dtext_depth_hist(sid_ctx* ctx, const sid_dtext* t, size_t begin, size_t end, const uint8_t* code /* device */,
                         sid_depth_row** rows, size_t* n, void* stream);
/* The region rows (Conventions) of sites [begin, end) of a resident shard with
 * the given device codes, for the context's region set (sid_opts.regions at
 * sid_create): the engine's stage over one range.  It needs no switch on the
 * context.  *rows (sid_regions_intervals of them, with their own copy of the
 * names) is freed with sid_region_stats_free.  SID_EINVAL for a context
 * without a set or with one sid_region_stats_valid refuses.  Synchronises. */
int sid_dtext_region_stats(sid_ctx* ctx, const sid_dtext* t, size_t begin, size_t end,
                           const uint8_t* code /* device */, sid_region_row** rows, size_t* n, void* stream);
/* The callable runs (Conventions) of sites [begin, end) of a resident shard
 * with the given device codes, under the context's depth bounds (sid_set_depth):
 * the device stage over one range, the range's first site opening a row.  It
 * needs no switch on the context.  *rows is freed with
 * sid_callable_free.  Synchronises. */
int sid_dtext_callable(sid_ctx* ctx, const sid_dtext* t, size_t begin, size_t end, const uint8_t* code /* device */,
                       sid_callable_row** rows, size_t* n, void* stream);
/* -m quality (call.cpp:291-372) over a shard parsed by a context whose method
 * is SID_METHOD_QUALITY (7 fields per line): the read bases and both quality
 * fields are read from the resident text.  snp_prior / significance_level
 * from the context's options (sid_set_prior after a -R estimate). */
int sid_call_quality(sid_ctx* ctx, const sid_dtext* t, uint8_t* code, double* hom_conf, double* het_conf,
                     void* stream);
/* The device formatter's %g, host build (tests) and device batch: out gets
 * 16 bytes per value, NUL-padded. */
int sid_format_g6(double v, char* buf, size_t cap);
int sid_format_g6_device(sid_ctx* ctx, const double* values, size_t n, char* out, void* stream);


/* ------------------------------------------------ BGZF input ---------------
 * Block-compressed gzip (samtools mpileup ... | bgzip): a concatenation of
 * independent gzip members of at most 64 KiB of text each, the member's size
 * in its header (BSIZE), the text's size (ISIZE) and CRC32 in its trailer.
 *
 * sid_bgzf_index: the members of a byte range, found by hopping over headers
 *   and trailers (nothing is inflated).  SID_EBGZF and the compressed offset
 *   of the offending member when the bytes there are no BGZF header (plain
 *   gzip included), the member is truncated, or its ISIZE exceeds 64 KiB.
 *   Empty members (the EOF marker) are legal anywhere, a missing EOF marker is
 *   accepted, len == 0 is a valid empty input.
 * sid_bgzf_block: member k's compressed offset and size, its text's offset in
 *   the inflated text and size.
 * sid_bgzf_inflate_host: every member inflated and its CRC32 checked, on the
 *   host (no libz).  out == NULL sizes (*out_len); cap too small: SID_ENOMEM
 *   and a sufficient *out_len.  SID_EBGZF: *err_offset = the bad member's
 *   compressed offset.
 * sid_bgzf_inflate_device: members [first_block, first_block + nblocks) of the
 *   indexed range d_bytes (device memory, the whole range) inflated by the
 *   GPU, one wave per member, CRC32 checked; member k's text lands at d_out +
 *   toff(k) - toff(first_block).  cap too small: SID_ENOMEM, nothing launched.
 *   SID_EBGZF: *err_block = the lowest bad member.  Synchronises.
 * sid_crc32: zlib's crc32(), by the host build of the device routine. */
typedef struct sid_bgzf sid_bgzf;
int sid_bgzf_index(const void* bytes, size_t len, sid_bgzf** out, uint64_t* err_offset);
size_t sid_bgzf_blocks(const sid_bgzf* z);
uint64_t sid_bgzf_text_len(const sid_bgzf* z);
int sid_bgzf_block(const sid_bgzf* z, size_t k, uint64_t* coff, uint32_t* csize, uint64_t* toff, uint32_t* isize);
void sid_bgzf_free(sid_bgzf* z);
int sid_bgzf_inflate_host(const void* bytes, size_t len, char* out, size_t cap, size_t* out_len,
                          uint64_t* err_offset);
int sid_bgzf_inflate_device(sid_ctx* ctx, const void* d_bytes /* device */, const sid_bgzf* z, size_t first_block,
                            size_t nblocks, char* d_out /* device */, size_t cap, uint64_t* err_block, void* stream);
uint32_t sid_crc32(uint32_t crc, const void* p, size_t n);

/* ------------------------------------------------ streaming engine -------
 * The whole path of one sid run -- pileup text in, CSV records out, in file
 * order -- replacing readFile + callX + the output loop (call.cpp:11-20,
 * call.cpp:62-289, sid.cpp:92-105) with a bounded-memory pipeline over
 * line-aligned chunks of the input:
 *
 *   host text --H2D (ring of device buffers)--> line index + parse
 *     [-m local / quality: call + CSV format, held in HBM]
 *     [Lynch (likelihood_ratio, bayes, -R): profile histogram]
 *   (the whole input validated; Lynch: merge + one estimate + class tables)
 *   [second pass over the chunks not formatted yet: parse, call / lookup,
 *    format] --D2H (pinned ring)--> write() in file order
 *
 * Chunk j runs on pipeline j % (devices x lanes) (pipeline i on GPU i / lanes);
 * every pipeline formats and copies back
 * concurrently and one writer keeps file order.  As in the reference, no
 * record is written before the whole input has parsed: the first malformed
 * line in file order is reported (its input byte offset in err_offset) and
 * nothing is written.  Host memory stays bounded (pinned rings); device
 * memory holds the formatted records of the chunks processed before the input
 * was validated, up to hold_bytes per device, beyond which chunks are
 * formatted in the second pass (their text kept in HBM up to retain_bytes,
 * else read again from the source).
 *
 * Usage: sid_engine_create, one sid_engine_source_*, then sid_engine_run --
 * or the three phases separately (multi-rank runs exchange the Lynch
 * histogram between ingest and estimate: sid_engine_context + the
 * sid_profile_* calls).  An engine is reusable: set a new source and run
 * again.  Not thread-safe. */
typedef struct sid_engine sid_engine;
typedef struct {
    int devices;            /* GPUs used (0 = every visible one); chunk j runs on
                               device (first_device + j % devices) % visible       */
    int first_device;
    uint64_t chunk_bytes;   /* input text per chunk (0 = 128 MiB)                  */
    int slots;              /* device text buffers per device (0 = 3)              */
    uint64_t hold_bytes;    /* per device, HBM for records held until the input is
                               validated (0 = 40% of free HBM)                     */
    uint64_t retain_bytes;  /* per device, HBM for text kept for the second pass
                               (0 = 40% of free HBM)                               */
    int host_threads;       /* host threads generating / prefetching input (0 = 8) */
    int verbose;            /* the reference's "# ..." lines on stderr             */
    int device_sink;        /* 0: write() in file order; 1: records stay in HBM,
                               nothing is copied back (measurement); 2: records
                               copied back to pinned host memory, no write
                               (measurement of the PCIe path; with
                               host_hold_bytes they stay there for
                               sid_engine_records)                               */
    int lanes;              /* pipelines per GPU (0 = 1): each its own streams,
                               context and workspace, chunks dealt over all of
                               them, so one chunk's kernels run while another
                               waits on its host sync                            */
    uint64_t host_hold_bytes; /* per pipeline, pinned host memory (made once,
                               reused by every run) for the records: -m local /
                               quality copy each chunk's records into it during
                               the ingest, while later chunks upload (PCIe both
                               ways at once), and the emit only write()s them;
                               the second pass copies into it instead of the
                               pinned ring.  Chunks beyond it take the HBM hold.
                               0 = off.  Ignored with device_sink 1             */
    int strip;              /* host text that is pinned already, an option set
                               that reads no quality column: strip crews (host
                               threads, host_threads of them per device when set,
                               else the process's CPUs less two, at most 14) drop
                               the quality columns (sid_strip_lines) into pinned
                               staging ahead of the upload, and the upload moves
                               what they finished in time stripped, the rest as
                               it is.  0 = on (SID_STRIP=0 in the environment:
                               off), -1 = off; for tests, 1 = the upload waits
                               for the crew on every chunk, 2 = on every other
                               chunk (the others go as they are)               */
} sid_engine_cfg;
typedef struct {
    uint64_t sites;              /* non-empty lines parsed                           */
    uint64_t chunks;
    uint64_t bytes_in;           /* input text bytes                                 */
    uint64_t bytes_out;          /* CSV bytes written (header excluded; with a
                                    selection by label, region, variant or depth:
                                    the selected records', with a context theirs too;
                                    exact in every sink mode)                                */
    uint64_t chunks_held;        /* formatted in the first pass                      */
    uint64_t chunks_retained;    /* text kept in HBM for the second pass             */
    uint64_t chunks_reloaded;    /* text read from the source a second time          */
    int devices;
    int status_kind;             /* parse error status of the first bad line, or 0   */
    uint64_t err_offset;         /* its input byte offset                            */
    double ingest_s, estimate_s, emit_s;
    sid_estimate estimate;       /* Lynch paths                                      */
    /* the ingest's uploads of host text (host memory or a file's mapping):     */
    uint64_t chunks_registered;  /* copied from pages registered for DMA (the
                                    others: the runtime's pageable path, or the
                                    source was pinned already)                     */
    double register_s;           /* host time in hipHostRegister / Unregister,
                                    summed over the uploaders                      */
    double h2d_s;                /* device time of the host-to-device copies: the
                                    span from each upload stream's first copy to
                                    its last (HIP events), summed over the
                                    devices                                        */
    uint64_t h2d_bytes;          /* bytes those copies moved                       */
    uint64_t chunks_tiled;       /* parsed by the tile parse (text read once)       */
    uint64_t tile_overflows;     /* chunks with a tile of more lines than its slots
                                    (parsed again by the two-pass path; the next
                                    chunks get more slots)                         */
    uint64_t tile_overflows_queued; /* of those, overflows with the device's next
                                    chunk already popped behind it (its run-ahead
                                    tile parse dropped, the chunk kept)            */
    uint64_t bgzf_bytes;         /* BGZF sources: the compressed bytes of the members
                                    uploaded in the first pass, a member that two
                                    chunks share counted once (h2d_bytes counts it
                                    twice); empty members outside every chunk (the
                                    EOF marker) are not uploaded.  bytes_in stays
                                    the text parsed                                 */
    uint64_t bgzf_blocks;        /* ... and their number                            */
    uint64_t window_rows;        /* sid_opts.window: the rows of the summary (after
                                    the chunks' rows are stitched; set by the emit)  */
} sid_run_stats;
void sid_engine_cfg_default(sid_engine_cfg* cfg);
int sid_engine_create(const sid_opts* opts, const sid_engine_cfg* cfg, sid_engine** out);
int sid_engine_destroy(sid_engine* e);
int sid_engine_devices(const sid_engine* e);
sid_ctx* sid_engine_context(sid_engine* e, int i);
/* sid_set_depth on every pipeline's context.  Allowed after sid_engine_create
 * and again once a run has ended (the emit returned, or the ingest failed);
 * between a successful sid_engine_ingest and its emit: SID_ESTATE (-m local
 * formats during the ingest).  The bounds hold for every later run until they
 * are set again. */
int sid_engine_set_depth(sid_engine* e, int min, int max);
/* sid_set_format on every pipeline's context, under the same state rules:
 * SID_EINVAL for a value that is no SID_FORMAT_*, SID_ESTATE between a
 * successful sid_engine_ingest and its emit.  The format holds for every later
 * run until it is set again; the caller passes sid_vcf_header's text as the
 * emit's header.  bytes_out counts the VCF lines' bytes. */
int sid_engine_set_format(sid_engine* e, int format);
/* The depth histogram (Conventions) of every pipeline, under the same state
 * rules: SID_EINVAL for a value other than 0 and 1, SID_ESTATE between a
 * successful sid_engine_ingest and its emit.  The setting holds for every
 * later run until it is set again.  Off (the default): no kernel of the stage
 * is launched and no buffer of it allocated.  On, a selection by label goes the
 * context's route with N = 0, as under sid_opts.window: the same records. */
int sid_engine_set_depth_hist(sid_engine* e, int on);
/* The region rows (Conventions) of every pipeline, under the same state rules:
 * SID_EINVAL for a value other than 0 and 1, for an engine created without
 * sid_opts.regions, or for a set of more than SID_REGION_STATS_MAX intervals;
 * SID_ESTATE between a successful sid_engine_ingest and its emit.  The setting
 * holds for every later run until it is set again.  Off (the default): no
 * kernel of the stage is launched and no buffer of it allocated.  On, a
 * selection by label goes the context's route with N = 0, as under
 * sid_engine_set_depth_hist: the same records. */
int sid_engine_set_region_stats(sid_engine* e, int on);
/* Host placement of pipeline i (a multi-GPU node: each GPU's uploader,
 * compute and drain threads run on the CPUs local to its PCI device, and its
 * pinned host buffers are allocated from them, so their pages sit on the
 * GPU's NUMA node and its DMA does not cross sockets). */
typedef struct {
    int device;             /* HIP device                                          */
    int gpu_numa_node;      /* NUMA node of the GPU's PCI device (-1: unknown)     */
    int cpus;               /* CPUs its threads are bound to (0: not bound)        */
    int first_cpu;          /* the lowest of them (-1: not bound)                  */
    int arena_numa_node;    /* NUMA node of the host arena's first page (-1: none) */
    int ring_numa_node;     /* ... of the emit ring's first page (-1: none)        */
    char pci[16];           /* PCI bus id, e.g. "0000:05:00.0"                     */
} sid_placement;
int sid_engine_placement(const sid_engine* e, int i, sid_placement* out);
/* Sources.  The engine keeps the pointer / descriptor until the next source. */
int sid_engine_source_text(sid_engine* e, const char* text, uint64_t len);          /* host memory */
int sid_engine_source_file(sid_engine* e, int fd, uint64_t offset, uint64_t len);   /* regular file */
/* BGZF-compressed pileup text (host memory / a regular file, mapped): the
 * input is indexed at once (SID_EBGZF and the offending member's compressed
 * offset in *err_offset when it is not BGZF; the engine then has no source);
 * chunks are runs of whole members cut at line starts, their compressed bytes
 * cross the bus and are inflated on the device (sid_bgzf_inflate_device's
 * kernel) in front of the parse.  A member that does not inflate or fails its
 * CRC32 makes the ingest return SID_EBGZF, err_offset = its compressed
 * offset; inside a chunk it wins over a malformed line, across chunks the
 * earliest chunk in file order wins.  For a parse error err_offset is the
 * line's offset in the inflated text. */
int sid_engine_source_bgzf(sid_engine* e, const void* bytes, uint64_t len, uint64_t* err_offset);
int sid_engine_source_bgzf_file(sid_engine* e, int fd, uint64_t offset, uint64_t len, uint64_t* err_offset);
/* Text already in HBM on the engine's first device (measurement): d_text must
 * be readable for 256 bytes past len. */
int sid_engine_source_device_text(sid_engine* e, const char* d_text, uint64_t len);
/* The synthetic generator (sid_synth_text) streamed, never stored: sites
 * [first_site, first_site + n), sites_per_chunk per chunk (0 = about
 * chunk_bytes of text), generated by host threads into pinned buffers
 * (on_device = 0) or by a kernel straight into the device buffer (1). */
int sid_engine_source_synth(sid_engine* e, uint64_t seed, double mean_depth, uint64_t first_site, uint64_t n,
                            uint64_t sites_per_chrom, uint64_t sites_per_chunk, int on_device);
/* Phases.  ingest returns the parse status of the first malformed line
 * (stats->err_offset); estimate runs the Lynch estimate when the method needs
 * it (given != NULL: skip the Nelder-Mead, use given's pi/eps) and returns its
 * status (SID_EEMPTY, SID_EBADFUNC); emit writes `header` (unless NULL) and
 * the records through write(). */
int sid_engine_ingest(sid_engine* e, sid_run_stats* stats);
/* What the strip crews (sid_engine_cfg.strip) did in the last ingest: the
 * chunks uploaded with bytes of theirs stripped, and the input bytes not
 * uploaded for it (sid_run_stats.h2d_bytes = bytes_in - *strip_bytes, h2d_bytes
 * staying the bytes the copies moved).  Both 0 without crews.  sid_run_stats
 * has no field for them (its layout stands).  Either pointer may be NULL. */
int sid_engine_strip_stats(const sid_engine* e, uint64_t* chunks_stripped, uint64_t* strip_bytes);
int sid_engine_estimate(sid_engine* e, const sid_estimate* given, sid_estimate* out);
int sid_engine_emit(sid_engine* e, const char* header, sid_write_fn write, void* user, sid_run_stats* stats);
int sid_engine_run(sid_engine* e, const char* header, sid_write_fn write, void* user, sid_run_stats* stats);
/* Multi-rank Lynch runs: after ingest, the merged unique-
 * profile table of all the engine's pipelines (sid_profile_table layout;
 * keys == NULL: only *u), and the load of a table merged across ranks into
 * every pipeline (it is not merged again by sid_engine_estimate). */
int sid_engine_profile_table(sid_engine* e, uint64_t* keys, uint64_t* counts64, size_t cap, size_t* u);
int sid_engine_profile_load(sid_engine* e, const uint64_t* keys, const uint64_t* counts64, size_t u);
/* With host_hold_bytes: the CSV records of chunk `chunk` (0 .. stats.chunks-1,
 * file order) in the host arena, after the emit (device_sink 2: the records
 * are not written anywhere else), valid until the next ingest or source;
 * SID_ESTATE when that chunk's records did not go through the host arena.
 * With a context: exactly the bytes the chunk contributed to the output. */
int sid_engine_records(sid_engine* e, uint64_t chunk, const char** bytes, uint64_t* len);
/* The windowed summary of the run (sid_opts.window != 0), after a successful
 * sid_engine_emit in every device_sink mode: the rows in file order, owned by
 * the engine and valid until the next ingest or source.  SID_ESTATE before
 * that, after a failed run, or without the option. */
int sid_engine_windows(sid_engine* e, const sid_window** rows, size_t* n);
/* The depth histogram of the run (sid_engine_set_depth_hist), after a
 * successful sid_engine_emit in every device_sink mode: the rows in ascending
 * depth order, owned by the engine and valid until the next ingest or source.
 * SID_ESTATE before that, after a failed run, or with the option off.
 * sid_run_stats has no field for the number of rows (its layout stands, as
 * sid_opts'): *n is that number. */
int sid_engine_depth_hist(sid_engine* e, const sid_depth_row** rows, size_t* n);
/* The region rows of the run (sid_engine_set_region_stats), after a successful
 * sid_engine_emit in every device_sink mode: one row per interval of the set in
 * row order, owned by the engine (the names too) and valid until the next
 * ingest or source.  SID_ESTATE before that, after a failed run, or with the
 * option off.  sid_run_stats has no field for them (its layout stands). */
int sid_engine_region_stats(sid_engine* e, const sid_region_row** rows, size_t* n);
/* Measurement: with profiling on, every stage of every chunk is bracketed by
 * a pair of HIP events on its device's compute stream; _read sums the stages'
 * device time over the chunks and devices since the last read (synchronises). */
typedef struct {
    uint64_t chunks;        /* chunks processed (either pass)                      */
    double index_ms;        /* line index: line starts per tile + scan             */
    double parse_ms;        /* line offsets + parse to counts                      */
    double call_ms;         /* sid_call_local / sid_lookup_sites / quality kernels */
    double hist_ms;         /* Lynch profile histogram                             */
    double fmt_len_ms;      /* record lengths + scan                               */
    double fmt_write_ms;    /* records written                                     */
} sid_engine_prof;
int sid_engine_profile(sid_engine* e, int enable);
int sid_engine_profile_read(sid_engine* e, sid_engine_prof* out);

#ifdef __cplusplus
}
#endif
#endif /* SID_H */
