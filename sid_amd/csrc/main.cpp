// main.cpp — the `sid` command line on MI355X.
//
// Same surface as sid.cpp:1-110: getopt flags -h -m -r -R -p -E with the
// reference's defaults, help text, error messages and exit codes; CSV on
// stdout, "# ..." diagnostics on stderr.  Behind it, by default, the
// streaming engine (run.cpp, sid_engine_*): the input file in line-aligned
// chunks -> device text buffers -> parse -> call / Lynch -> records formatted
// on the device -> stdout in file order, every visible GPU taking chunks in
// turn, with bounded host memory (C4's 3G sites stream through).
//
// Extra long options (no short letter, so they cannot collide with the
// reference's flags): --devices N, --threads N, --stats, --host-parse,
// --chunk-bytes N, --hold-bytes N, --retain-bytes N, --host-hold N,
// --only het|hom|all, --regions FILE, --bgzf, --context N, --windows W,
// --windows-out FILE, --variants, --min-depth N, --max-depth N, --vcf,
// --depth-hist FILE, --callable FILE.
//
// --callable FILE (with --host-parse): beside the records, the callable runs
// of the run (sid_callable_host, sid.h Conventions) as BED into FILE --
// "chrom\tstart\tend\thet" a line per run, in file order, no header -- under the
// depth bounds of --min-depth / --max-depth, written after the records; stdout,
// stderr and the exit status are as without it, whatever --only, --regions,
// --variants, --context and --vcf select or print.  Error texts and file
// handling as --depth-hist's: "sid: --callable: could not open FILE" before any
// input is read, "sid: --callable: could not write FILE"; a failing run leaves
// no file.  The streaming engine does not produce the rows yet: without
// --host-parse, "sid: --callable: needs --host-parse" and exit status 1 before
// any input is read.  --stats prints callable_rows and callable_sites, the sum
// of end - start.  Not listed by -h.
//
// --region-stats FILE (with --regions BED): beside the records, the region rows
// of the run (sid_engine_set_region_stats, sid.h Conventions) as CSV into FILE
// -- "chrom,start,end,sites,depth,records,het,hom" and a line for every interval
// of the set after its merge, one without a site included, the chroms in the
// BED's order and a chrom's intervals ascending -- written after the records.
// The rows count every site inside an interval: stdout, stderr and the exit
// status are as without it, and --only, --variants, --min-depth / --max-depth,
// --context and --vcf, like --regions' own selection of the records, never
// change the rows.  Error texts and file handling as --depth-hist's: "sid:
// --region-stats: could not open FILE" before any input is read, "sid:
// --region-stats: could not write FILE"; a failing run leaves no file.  Without
// --regions: "sid: --region-stats: needs --regions"; a set of more than 2^20
// merged intervals: "sid: --region-stats: more than 1048576 intervals"; either
// with exit status 1 before any input is read.  With --host-parse:
// sid_region_stats_host.  --stats then also prints region_rows and
// region_sites, the sum of the sites column.  Not listed by -h.
//
// --depth-hist FILE: beside the records, the depth histogram of the run
// (sid_engine_set_depth_hist, sid.h Conventions) as CSV into FILE --
// "depth,sites,records,het,hom" and a line per depth that a site has, in
// ascending order, the columns as --windows-out's -- written after the records;
// stdout, stderr and the exit status are as without it, whatever --only,
// --regions, --variants, --min-depth / --max-depth, --context and --vcf select
// or print.  A FILE that cannot be created: "sid: --depth-hist: could not open
// FILE" on stderr, exit status 1, nothing on stdout, before any input is read;
// a failed write: "sid: --depth-hist: could not write FILE".  As with
// --windows-out the file is written only after the records: a failing run
// leaves none (one that was there before stays as it was).  With --host-parse:
// sid_depth_hist_host.  Not listed by -h, whose text stays the reference's.
//
// --vcf (no argument) writes the records as VCF lines behind a VCF header
// (sid_vcf_header) in place of the CSV and its header line (sid.h Conventions,
// "VCF"): a line for exactly the sites that print a CSV record under the same
// options, in the same order, with REF from the pileup's third column, DP the
// counted depth, the two confidences as INFO fields and the gt field as ALT and
// GT.  --only, --regions, --variants, --min-depth / --max-depth and --context
// decide which records exist exactly as for the CSV; stderr, the exit status
// and the --windows rows are as without it, and an unknown -m prints the VCF
// header alone.  The lines are formatted on the device (sid_engine_set_format);
// with --host-parse: sid_format_vcf.  Not listed by -h, whose text stays the
// reference's.
//
// --min-depth N / --max-depth N (decimal, 0 .. 262140; given twice, the last
// wins) write the header and only the records of the sites whose depth -- A +
// C + G + T of the parsed profile, not the pileup's fourth column (sid.h
// Conventions) -- is at least the one and, when --max-depth is not 0, at most
// the other, chosen before the records are formatted (sid_engine_set_depth).
// 0 and 0 is the run without them.  Everything else, stderr included, is as
// without them; with --only, --regions and / or --variants all must hold,
// --context N counts from what they all keep, and the --windows rows do not
// change.  An argument that is no such number: "sid: --min-depth: expected
// 0..262140, got ARG" (likewise --max-depth); a minimum above a maximum that is
// not 0: "sid: --min-depth above --max-depth"; each on stderr with exit status
// 1 and nothing on stdout.  With --host-parse: sid_depth_mark.  Not listed by
// -h, whose text stays the reference's.
//
// --variants (no argument) writes the header and only the records whose
// genotype is not homozygous reference (sid_opts.variants, sid.h Conventions):
// the reference base is the line's third column, upper-cased; a record stays
// when that is one of A, C, G, T, the site has a counted base and its gt field
// is not that base twice -- the het sites `--only het` finds and the
// homozygous non-reference sites it misses, chosen before the records are
// formatted.  Everything else, stderr included, is as without it; with --only
// and / or --regions all must hold, --context N counts from what they all
// keep, and the --windows rows do not change.  With --host-parse:
// sid_variants_mark.  Not listed by -h, whose text stays the reference's.
//
// --windows W --windows-out FILE (W in 1 .. 2147483647): beside the records,
// the windowed summary of the run (sid_opts.window, sid.h Conventions) as CSV
// into FILE -- "chrom,start,end,sites,records,het,hom" and a line per run of
// consecutive sites with one chrom and one window floor((pos - 1) / W) --
// written after the records; stdout, stderr and the exit status are as
// without them, whatever --only, --regions and --context select.  One
// without the other: "sid: --windows and --windows-out go together"; a W
// that is no such integer: "sid: --windows: expected 1..2147483647, got ARG";
// a FILE that cannot be created: "sid: --windows-out: could not open FILE";
// each on stderr with exit status 1 and nothing on stdout.
//
// --context N (0 .. 64): grep -C N over the unselected output -- with --only
// and / or --regions, every selected record comes with the N records before
// and after it (records, not positions; sid_opts.context), chosen before the
// records are formatted; the reference pipeline's identify-nonsyn.sh step
// then reads its SNPs' neighbouring lines from the selected output.  Without
// a selection, or with N = 0, nothing changes.  A value that is not a decimal
// integer in 0 .. 64: "sid: --context: expected 0..64, got ARG" on stderr,
// exit status 1, nothing on stdout.  Given twice, the last wins.
//
// --bgzf: the input is BGZF (samtools mpileup ... | bgzip), from a regular
// file (mapped) or a pipe (read into memory) -- the reference pipeline's
// `zcat input.plp.gz > input.plp` step: the compressed bytes cross the bus and
// are inflated on the device in front of the parse (sid_engine_source_bgzf*);
// with --host-parse they are inflated on the host (sid_bgzf_inflate_host).
// "sid: FILE: not a BGZF file" (plain gzip or anything else) or "sid: FILE:
// corrupt BGZF block at byte N" (N: the member's offset in the file) on
// stderr, exit status 1, nothing on stdout; everything else is the run on the
// inflated file's.
//
// --regions FILE (a BED file: chrom start end, 0-based half-open, or a chrom
// alone for all of it; sid_regions_from_bed) writes the header and only the
// records whose (chrom, pos) lies in the file's intervals -- the reference
// pipeline's filter-exon-sites.sh step, or one chromosome of parallel-run-
// sid.sh -- selected before the records are formatted (sid_opts.regions);
// everything else, stderr included, is as without it, and with --only both
// must hold.  The file is read when the option is parsed: "sid: --regions:
// could not open FILE" or "sid: --regions: FILE:LINE: malformed region" on
// stderr, exit status 1, nothing on stdout.  Given twice, the last wins.
//
// --only het (or hom) writes the header and only the records with that label
// -- the reference pipeline's `zgrep ,het,` step, done before the records are
// formatted (sid_opts.select); everything else, stderr included, is as
// without it.  Any other value: "sid: --only: expected het, hom or all" on
// stderr, exit status 1, nothing on stdout.  Not listed by -h, whose text
// stays the reference's.
//
// --host-parse keeps the round-1 path instead: the whole input parsed on the
// host (sid_parse_text), counts to the devices, records formatted on the host
// (sid_format_csv).
//
// As in the reference, the whole input is parsed before anything is written
// to stdout, so a malformed line aborts with no CSV output (call.cpp:11-20
// reads the file before sid.cpp:102 prints the header).
#include <fcntl.h>
#include <getopt.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <csignal>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sid.h"

namespace {

struct Options {
    std::string method = "local";
    sid_opts o;
    int devices = 0;   // 0: every visible device
    int threads = 0;
    bool stats = false;
    bool host_parse = false;   // parse and format on the host (sid_parse_text / sid_format_csv)
    bool bgzf = false;         // --bgzf: the input is BGZF
    uint64_t chunk_bytes = 0;  // engine knobs (0 = defaults)
    uint64_t hold_bytes = 0;
    uint64_t host_hold = 0;   // --host-hold: sid_engine_cfg.host_hold_bytes
    uint64_t retain_bytes = 0;
};

// sid.cpp:26-58; std::map<char,...> iterates E R h m p r
const struct {
    char flag;
    const char* name;
    int has_arg;
    const char* description;
} OPTIONS[] = {
    {'E', "ERROR", 1, "Maximum allowed site error rate for 'local' method. Default: 0.1"},
    {'R', "", 0, "Estimate SNP prior from data, applicable for methods 'likelihood_ratio', 'local', 'quality'. Conflicts -r."},
    {'h', "help", 0, "Print this help message"},
    {'m', "METHOD", 1, "Select the method to use for SNP calling: 'likelihood_ratio' , 'bayes', 'local' or 'quality', default: local"},
    {'p', "LEVEL", 1, "Significance level for statistical tests, only applicable for methods 'likelihood_ratio', 'local'. Default: 0.05"},
    {'r', "PRIOR", 1, "Use the given prior for SNPs, applicable for methods 'local', 'quality'. Conflicts -R. Default: no prior"},
};

[[noreturn]] void terminate_like(const char* type, const char* what)
{
    std::fflush(stdout);
    std::fprintf(stderr, "terminate called after throwing an instance of '%s'\n  what():  %s\n", type, what);
    std::abort();
}

[[noreturn]] void fail(const char* what, int rc)
{
    std::fflush(stdout);
    if (rc == SID_EHIP)
        std::fprintf(stderr, "sid: %s: %s (hip error %d)\n", what, sid_strerror(rc), sid_last_hip_error());
    else
        std::fprintf(stderr, "sid: %s: %s\n", what, sid_strerror(rc));
    std::exit(EXIT_FAILURE);
}

#define CHECK(call, what)                 \
    do {                                  \
        int rc_ = (call);                 \
        if (rc_ != SID_OK) fail(what, rc_); \
    } while (0)

#define HCHECK(call, what)                                                              \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            std::fprintf(stderr, "sid: %s: %s\n", what, hipGetErrorString(e_));         \
            std::exit(EXIT_FAILURE);                                                    \
        }                                                                               \
    } while (0)

double now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// wall-clock seconds (--stats: main's entry and exit, so a caller timing the
// process can split off the start-up and the teardown)
double unix_now()
{
    return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
}

// The end of a successful run: stdout and stderr flushed, then the process
// ends without the HIP runtime's teardown (the kernel driver releases the
// HBM, the pinned pages and the mapping with the process either way).
// (exit() with the runtime's static destructors measured 0.06-0.18 s slower;
// DESIGN.md §6.)  Under the profiler (ROCPROF* / ROCP_* in the environment: rocprofv3 sets
// them for its preloaded tool, which writes its buffers from atexit
// handlers) exit() is used too, so traces of this binary are complete.
bool tool_attached()
{
    for (char** e = environ; e && *e; ++e)
        if (std::strncmp(*e, "ROCPROF", 7) == 0 || std::strncmp(*e, "ROCP_", 5) == 0)
            return true;
    return false;
}

sid_regions* g_regions = nullptr;   // the --regions set: freed on the way out (finish, or exit's handler)
void free_regions()
{
    sid_regions_free(g_regions);
    g_regions = nullptr;
}

[[noreturn]] void finish(int code)
{
    std::fflush(stdout);
    std::fflush(stderr);
    free_regions();
    if (tool_attached()) std::exit(code);
    ::_exit(code);
}

struct Input {
    const char* data = nullptr;   // the text in memory (pipes, or mapped for --host-parse)
    size_t len = 0;
    void* map = nullptr;
    std::string owned;
    int fd = -1;                  // regular file: mapped by the engine (sid_engine_source_file)
};

void map_input(Input& in, bool populate)
{
    if (in.data || in.fd < 0 || !in.len) return;
    in.map = mmap(nullptr, in.len, PROT_READ, MAP_PRIVATE | (populate ? MAP_POPULATE : 0), in.fd, 0);
    if (in.map == MAP_FAILED) {
        in.map = nullptr;
        in.owned.resize(in.len);
        size_t off = 0;
        while (off < in.len) {
            ssize_t r = ::pread(in.fd, &in.owned[off], in.len - off, (off_t)off);
            if (r <= 0) break;
            off += (size_t)r;
        }
        in.owned.resize(off);
        in.data = in.owned.data();
        in.len = off;
    } else {
        madvise(in.map, in.len, MADV_SEQUENTIAL);
        in.data = (const char*)in.map;
    }
}

// std::ifstream semantics: open failure -> "Could not open file" (sid.cpp:86-89)
bool open_input(const char* path, Input& in)
{
    int fd = ::open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
        in.len = (size_t)st.st_size;
        in.fd = fd;   // kept open
        return true;
    }
    if (fstat(fd, &st) == 0 && S_ISDIR(st.st_mode)) {
        // std::ifstream opens a directory, getline then fails: no records
        in.len = 0;
    } else {   // pipe / character device
        char buf[1 << 16];
        ssize_t r;
        while ((r = ::read(fd, buf, sizeof buf)) > 0) in.owned.append(buf, (size_t)r);
        in.data = in.owned.data();
        in.len = in.owned.size();
    }
    ::close(fd);
    return true;
}

struct Shard {
    size_t begin = 0, end = 0;            // global site range
    sid_ctx* ctx = nullptr;
    const uint16_t* d_counts = nullptr;   // the shard's counts
    uint16_t* d_own_counts = nullptr;     // host-parse path: uploaded counts
    uint8_t* d_code = nullptr;
    double* d_hom = nullptr;
    double* d_het = nullptr;
    hipStream_t stream = nullptr;
};

}  // namespace

int main(int argc, char** argv)
{
    const double t_entry = unix_now();
    // host<->device copies on the copy engines (set before the HIP runtime
    // starts; an explicit setting in the environment wins): with the
    // runtime's default, device->host ran at 30 GB/s, with SDMA at ~57 GB/s
    // and concurrently with host->device (tools/debug/pcie_probe.cpp)
    setenv("HSA_ENABLE_SDMA", "1", 0);
    Options opt;
    sid_opts_default(&opt.o);
    sid_regions* regions = nullptr;   // --regions (kept for the run: --host-parse marks with it)
    std::atexit(free_regions);   // (the ways out that do not go through finish)
    const char* windows_out = nullptr;   // --windows-out
    int min_depth = 0, max_depth = 0;    // --min-depth, --max-depth
    bool vcf = false;                    // --vcf
    const char* depth_hist_out = nullptr;   // --depth-hist
    const char* callable_out = nullptr;     // --callable
    const char* region_stats_out = nullptr; // --region-stats
    static const struct option LONG[] = {{"devices", required_argument, nullptr, 1},
                                         {"threads", required_argument, nullptr, 2},
                                         {"stats", no_argument, nullptr, 3},
                                         {"host-parse", no_argument, nullptr, 4},
                                         {"chunk-bytes", required_argument, nullptr, 5},
                                         {"hold-bytes", required_argument, nullptr, 6},
                                         {"retain-bytes", required_argument, nullptr, 7},
                                         {"host-hold", required_argument, nullptr, 8},
                                         {"only", required_argument, nullptr, 9},
                                         {"regions", required_argument, nullptr, 10},
                                         {"bgzf", no_argument, nullptr, 11},
                                         {"context", required_argument, nullptr, 12},
                                         {"windows", required_argument, nullptr, 13},
                                         {"windows-out", required_argument, nullptr, 14},
                                         {"variants", no_argument, nullptr, 15},
                                         {"min-depth", required_argument, nullptr, 16},
                                         {"max-depth", required_argument, nullptr, 17},
                                         {"vcf", no_argument, nullptr, 18},
                                         {"depth-hist", required_argument, nullptr, 19},
                                         {"callable", required_argument, nullptr, 20},
                                         {"region-stats", required_argument, nullptr, 21},
                                         {nullptr, 0, nullptr, 0}};
    int flag;
    while ((flag = getopt_long(argc, argv, "E:Rhm:p:r:", LONG, nullptr)) != -1) {
        switch (flag) {
        case 'E': opt.o.site_error_threshold = std::atof(optarg); break;
        case 'R': opt.o.estimate_prior = 1; break;
        case 'm': opt.method = optarg; break;
        case 'p': opt.o.significance_level = std::atof(optarg); break;
        case 'r': opt.o.snp_prior = std::atof(optarg); break;
        case 'h':
            std::fputs("sid [flags] input_file\n", stdout);
            for (const auto& o : OPTIONS) {
                std::printf("\t-%c", o.flag);
                if (o.has_arg > 0) std::printf(" %s", o.name);
                std::printf("\t%s\n", o.description);
            }
            break;
        case 1: opt.devices = std::max(1, std::atoi(optarg)); break;
        case 2: opt.threads = std::max(1, std::atoi(optarg)); break;
        case 3: opt.stats = true; break;
        case 4: opt.host_parse = true; break;
        case 5: opt.chunk_bytes = std::strtoull(optarg, nullptr, 10); break;
        case 6: opt.hold_bytes = std::strtoull(optarg, nullptr, 10); break;
        case 7: opt.retain_bytes = std::strtoull(optarg, nullptr, 10); break;
        case 8: opt.host_hold = std::strtoull(optarg, nullptr, 10); break;
        case 9:
            if (std::strcmp(optarg, "het") == 0) opt.o.select = SID_SELECT_HET;
            else if (std::strcmp(optarg, "hom") == 0) opt.o.select = SID_SELECT_HOM;
            else if (std::strcmp(optarg, "all") == 0) opt.o.select = SID_SELECT_ALL;
            else {
                std::fflush(stdout);
                std::fputs("sid: --only: expected het, hom or all\n", stderr);
                std::exit(EXIT_FAILURE);
            }
            break;
        case 10: {
            std::string bed;
            FILE* f = std::fopen(optarg, "rb");
            if (!f) {
                std::fflush(stdout);
                std::fprintf(stderr, "sid: --regions: could not open %s\n", optarg);
                std::exit(EXIT_FAILURE);
            }
            char buf[1 << 16];
            for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) bed.append(buf, k);
            const bool unread = std::ferror(f) != 0;   // (a directory opens, and cannot be read)
            std::fclose(f);
            if (unread) {
                std::fflush(stdout);
                std::fprintf(stderr, "sid: --regions: could not open %s\n", optarg);
                std::exit(EXIT_FAILURE);
            }
            sid_regions* rg = nullptr;
            uint64_t bad = 0;
            if (sid_regions_from_bed(bed.data(), bed.size(), &rg, &bad) != SID_OK) {
                std::fflush(stdout);
                std::fprintf(stderr, "sid: --regions: %s:%llu: malformed region\n", optarg, (unsigned long long)bad);
                std::exit(EXIT_FAILURE);
            }
            sid_regions_free(regions);   // (given twice: the last wins)
            regions = rg;
            g_regions = rg;
            opt.o.regions = rg;
            break;
        }
        case 11: opt.bgzf = true; break;
        case 12: {
            int v = 0;
            bool good = *optarg != 0 && std::strlen(optarg) <= 3;
            for (const char* c = optarg; good && *c; ++c) {
                good = *c >= '0' && *c <= '9';
                v = v * 10 + (*c - '0');
            }
            if (!good || v > SID_CONTEXT_MAX) {
                std::fflush(stdout);
                std::fprintf(stderr, "sid: --context: expected 0..64, got %s\n", optarg);
                std::exit(EXIT_FAILURE);
            }
            opt.o.context = v;
            break;
        }
        case 13: {
            long long v = 0;
            bool good = *optarg != 0 && std::strlen(optarg) <= 10;
            for (const char* c = optarg; good && *c; ++c) {
                good = *c >= '0' && *c <= '9';
                v = v * 10 + (*c - '0');
            }
            if (!good || v < 1 || v > 2147483647LL) {
                std::fflush(stdout);
                std::fprintf(stderr, "sid: --windows: expected 1..2147483647, got %s\n", optarg);
                std::exit(EXIT_FAILURE);
            }
            opt.o.window = (int)v;   // (given twice: the last wins)
            break;
        }
        case 14: windows_out = optarg; break;
        case 15: opt.o.variants = 1; break;
        case 16:
        case 17: {
            int v = 0;
            bool good = *optarg != 0 && std::strlen(optarg) <= 6;
            for (const char* c = optarg; good && *c; ++c) {
                good = *c >= '0' && *c <= '9';
                v = v * 10 + (*c - '0');
            }
            if (!good || v > SID_DEPTH_MAX) {
                std::fflush(stdout);
                std::fprintf(stderr, "sid: --%s-depth: expected 0..262140, got %s\n", flag == 16 ? "min" : "max", optarg);
                std::exit(EXIT_FAILURE);
            }
            (flag == 16 ? min_depth : max_depth) = v;   // (given twice: the last wins)
            break;
        }
        case 18: vcf = true; break;
        case 19: depth_hist_out = optarg; break;   // (given twice: the last wins)
        case 20: callable_out = optarg; break;     // (likewise)
        case 21: region_stats_out = optarg; break; // (likewise)
        default: std::exit(EXIT_FAILURE);
        }
    }
    if (max_depth != 0 && min_depth > max_depth) {
        std::fflush(stdout);
        std::fputs("sid: --min-depth above --max-depth\n", stderr);
        std::exit(EXIT_FAILURE);
    }
    const bool depth_on = min_depth != 0 || max_depth != 0;
    if ((opt.o.window > 0) != (windows_out != nullptr)) {
        std::fflush(stdout);
        std::fputs("sid: --windows and --windows-out go together\n", stderr);
        std::exit(EXIT_FAILURE);
    }
    if (windows_out) {   // the file must be creatable; it is written after the records (a failed run leaves none)
        const bool was = ::access(windows_out, F_OK) == 0;
        const int fd = ::open(windows_out, O_WRONLY | O_CREAT, 0666);
        if (fd < 0) {
            std::fflush(stdout);
            std::fprintf(stderr, "sid: --windows-out: could not open %s\n", windows_out);
            std::exit(EXIT_FAILURE);
        }
        ::close(fd);
        if (!was) ::unlink(windows_out);
    }
    if (depth_hist_out) {   // likewise
        const bool was = ::access(depth_hist_out, F_OK) == 0;
        const int fd = ::open(depth_hist_out, O_WRONLY | O_CREAT, 0666);
        if (fd < 0) {
            std::fflush(stdout);
            std::fprintf(stderr, "sid: --depth-hist: could not open %s\n", depth_hist_out);
            std::exit(EXIT_FAILURE);
        }
        ::close(fd);
        if (!was) ::unlink(depth_hist_out);
    }
    if (callable_out && (!opt.host_parse || opt.method == "quality")) {
        // (the rows come from sid_callable_host; -m quality always takes the device text path)
        std::fflush(stdout);
        std::fputs("sid: --callable: needs --host-parse\n", stderr);
        std::exit(EXIT_FAILURE);
    }
    if (callable_out) {   // likewise
        const bool was = ::access(callable_out, F_OK) == 0;
        const int fd = ::open(callable_out, O_WRONLY | O_CREAT, 0666);
        if (fd < 0) {
            std::fflush(stdout);
            std::fprintf(stderr, "sid: --callable: could not open %s\n", callable_out);
            std::exit(EXIT_FAILURE);
        }
        ::close(fd);
        if (!was) ::unlink(callable_out);
    }
    if (region_stats_out && !regions) {
        std::fflush(stdout);
        std::fputs("sid: --region-stats: needs --regions\n", stderr);
        std::exit(EXIT_FAILURE);
    }
    if (region_stats_out && sid_region_stats_valid(regions) != SID_OK) {
        std::fflush(stdout);
        std::fprintf(stderr, "sid: --region-stats: more than %u intervals\n", (unsigned)SID_REGION_STATS_MAX);
        std::exit(EXIT_FAILURE);
    }
    if (region_stats_out) {   // the file must be creatable, as --depth-hist's
        const bool was = ::access(region_stats_out, F_OK) == 0;
        const int fd = ::open(region_stats_out, O_WRONLY | O_CREAT, 0666);
        if (fd < 0) {
            std::fflush(stdout);
            std::fprintf(stderr, "sid: --region-stats: could not open %s\n", region_stats_out);
            std::exit(EXIT_FAILURE);
        }
        ::close(fd);
        if (!was) ::unlink(region_stats_out);
    }
    if (optind >= argc) {
        std::fflush(stdout);
        std::fputs("No file name given!\n", stderr);
        std::exit(EXIT_FAILURE);
    }
    const char* path = argv[optind];
    Input in;
    if (!open_input(path, in)) {
        std::fflush(stdout);
        std::fprintf(stderr, "Could not open file: %s\n", path);
        std::exit(EXIT_FAILURE);
    }
    int method = -1;
    if (opt.method == "local") method = SID_METHOD_LOCAL;
    else if (opt.method == "bayes") method = SID_METHOD_BAYES;
    else if (opt.method == "likelihood_ratio") method = SID_METHOD_LIKELIHOOD_RATIO;
    else if (opt.method == "quality") method = SID_METHOD_QUALITY;   // call.cpp:291-372
    // --vcf: the VCF header of the run in place of the CSV's line
    std::string vcf_head;
    auto vcf_header = [&] {
        size_t need = 0;
        (void)sid_vcf_header(&opt.o, nullptr, 0, &need);
        vcf_head.assign(need, '\0');
        CHECK(sid_vcf_header(&opt.o, &vcf_head[0], need, &need), "header");
    };
    if (method < 0) {   // sid.cpp:92-102: unknown method -> header only
        if (vcf) {
            vcf_header();
            std::fwrite(vcf_head.data(), 1, vcf_head.size(), stdout);
        } else
            std::printf("chrom,pos,label,gt,hom_conf,het_conf,conf_type\n");
        return 0;
    }
    opt.o.method = method;
    if (method == SID_METHOD_BAYES) opt.o.estimate_prior = 0;   // callBayes(in) ignores -R/-r/-p
    if (vcf) vcf_header();
    const int T = opt.threads > 0 ? opt.threads
                                  : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));

    // The engine path over a regular file of up to 8 GiB: the HIP runtime's
    // start-up and the engine's creation (60-240 ms: the runtime's
    // initialisation, the contexts' class tables, the streams' hardware
    // queues) on a second thread while this one maps the file and populates
    // its page tables (~30 ms for 4 GB).
    const bool overlap = !opt.host_parse && in.fd >= 0 && !in.data && in.len && in.len <= (8ull << 30);
    int ndev = 0, D = 0;
    sid_engine* eng = nullptr;
    sid_engine_cfg cfg;
    sid_engine_cfg_default(&cfg);
    auto make_engine = [&]() -> int {
        cfg.devices = D;
        cfg.chunk_bytes = opt.chunk_bytes;
        cfg.hold_bytes = opt.hold_bytes;
        cfg.retain_bytes = opt.retain_bytes;
        cfg.host_hold_bytes = opt.host_hold;
        cfg.host_threads = T;
        cfg.verbose = 1;
        int rc = sid_engine_create(&opt.o, &cfg, &eng);
        if (rc == SID_OK && depth_on) rc = sid_engine_set_depth(eng, min_depth, max_depth);
        if (rc == SID_OK && vcf) rc = sid_engine_set_format(eng, SID_FORMAT_VCF);
        if (rc == SID_OK && depth_hist_out) rc = sid_engine_set_depth_hist(eng, 1);
        if (rc == SID_OK && region_stats_out) rc = sid_engine_set_region_stats(eng, 1);
        return rc;
    };
    int dev_rc = SID_OK, eng_rc = SID_OK;
    double t0 = 0, tc = 0;
    const char* pre_map = nullptr;
    auto start_devices = [&](bool engine) {
        dev_rc = sid_device_count(&ndev);
        if (dev_rc != SID_OK || ndev <= 0) return;
        D = opt.devices > 0 ? opt.devices : ndev;
        if (!engine) return;
        t0 = now();
        eng_rc = make_engine();
        tc = now();
    };
    if (overlap) {
        std::thread th(start_devices, true);
        void* m = mmap(nullptr, in.len, PROT_READ, MAP_PRIVATE | MAP_POPULATE, in.fd, 0);
        if (m != MAP_FAILED) {
            (void)madvise(m, in.len, MADV_SEQUENTIAL);
            pre_map = (const char*)m;
        }
        th.join();
    } else {
        start_devices(false);
    }
    CHECK(dev_rc, "device query");
    if (ndev <= 0) {
        std::fflush(stdout);
        std::fputs("sid: no HIP device available\n", stderr);
        std::exit(EXIT_FAILURE);
    }
    // shard d runs on device d % ndev (more shards than devices: a
    // multi-device run's splitting and merging on fewer GPUs)
    const bool quality = method == SID_METHOD_QUALITY;
    // the Lynch estimate: LR and bayes always, local and quality with -R
    const bool lynch = method == SID_METHOD_LIKELIHOOD_RATIO || method == SID_METHOD_BAYES || opt.o.estimate_prior;
    // per-read qualities live in the text: -m quality always takes the device text path
    if (quality) opt.host_parse = false;
    const char* conf_type = method == SID_METHOD_BAYES ? "probability" : "p_value";
    std::vector<Shard> sh(D);
    auto on_parse_error = [&](int prc) {
        if (prc == SID_EMALFORMED) terminate_like("std::invalid_argument", "Malformed pileup line");
        if (prc == SID_EMISSING_MQ)   // pileup.cpp:10,63
            terminate_like("std::invalid_argument", "Malformed pileup line or missing mapping qualities");
        if (prc == SID_ENULLCHROM || prc == SID_ENOBQ) {
            // pileup.cpp:18 assigns a NULL char* to std::string (or, for
            // -m quality, pileup.cpp:158 reads a NULL field): the reference
            // dies with SIGSEGV, printing nothing
            std::fflush(stdout);
            std::signal(SIGSEGV, SIG_DFL);
            std::raise(SIGSEGV);
        }
        CHECK(prc, "parse");
    };
    auto make_ctx = [&](int d) {
        Shard& s = sh[d];
        sid_opts o = opt.o;
        o.window = 0;   // (this path's rows come from the host codes: sid_windows_host)
        CHECK(sid_create(d % ndev, &o, &s.ctx), "context");
        if (depth_on) CHECK(sid_set_depth(s.ctx, min_depth, max_depth), "depth");
        HCHECK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), "stream");
    };
    auto alloc_out = [&](Shard& s) {
        const size_t m = std::max<size_t>(s.end - s.begin, 1);
        HCHECK(hipMalloc(&s.d_code, m), "device code");
        HCHECK(hipMalloc(&s.d_hom, m * 8), "device hom_conf");
        HCHECK(hipMalloc(&s.d_het, m * 8), "device het_conf");
    };
    auto parallel = [&](auto fn) {
        std::vector<std::thread> th;
        for (int d = 1; d < D; ++d) th.emplace_back(fn, d);
        fn(0);
        for (auto& x : th) x.join();
    };

    auto write_all = [](void*, const char* p, size_t len) -> int {
        size_t off = 0;
        while (off < len) {
            ssize_t w = ::write(1, p + off, len - off);
            if (w <= 0) return -1;
            off += (size_t)w;
        }
        return 0;
    };
    const char* HEADER = vcf ? vcf_head.c_str() : "chrom,pos,label,gt,hom_conf,het_conf,conf_type\n";
    // --windows-out: the rows as CSV, after the records
    auto write_windows = [&](const sid_window* rows, size_t nrows) {
        size_t need = 0;
        (void)sid_windows_format(rows, nrows, 1, nullptr, 0, &need);
        std::string csv(need, '\0');
        CHECK(sid_windows_format(rows, nrows, 1, &csv[0], need, &need), "windows");
        const int fd = ::open(windows_out, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        size_t off = 0;
        while (fd >= 0 && off < csv.size()) {
            const ssize_t w = ::write(fd, csv.data() + off, csv.size() - off);
            if (w <= 0) break;
            off += (size_t)w;
        }
        if (fd < 0 || off < csv.size() || ::close(fd) != 0) {
            std::fflush(stdout);
            std::fprintf(stderr, "sid: --windows-out: could not write %s\n", windows_out);
            std::exit(EXIT_FAILURE);
        }
    };
    // --depth-hist: the rows as CSV, after the records
    auto write_depth_hist = [&](const sid_depth_row* rows, size_t nrows) {
        size_t need = 0;
        (void)sid_depth_hist_format(rows, nrows, 1, nullptr, 0, &need);
        std::string csv(need, '\0');
        CHECK(sid_depth_hist_format(rows, nrows, 1, &csv[0], need, &need), "depth-hist");
        const int fd = ::open(depth_hist_out, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        size_t off = 0;
        while (fd >= 0 && off < csv.size()) {
            const ssize_t w = ::write(fd, csv.data() + off, csv.size() - off);
            if (w <= 0) break;
            off += (size_t)w;
        }
        if (fd < 0 || off < csv.size() || ::close(fd) != 0) {
            std::fflush(stdout);
            std::fprintf(stderr, "sid: --depth-hist: could not write %s\n", depth_hist_out);
            std::exit(EXIT_FAILURE);
        }
    };
    // --region-stats: the rows as CSV, after the records; returns the sum of the sites column
    auto write_region_stats = [&](const sid_region_row* rows, size_t nrows) {
        size_t need = 0;
        (void)sid_region_stats_format(rows, nrows, 1, nullptr, 0, &need);
        std::string csv(need, '\0');
        CHECK(sid_region_stats_format(rows, nrows, 1, &csv[0], need, &need), "region-stats");
        const int fd = ::open(region_stats_out, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        size_t off = 0;
        while (fd >= 0 && off < csv.size()) {
            const ssize_t w = ::write(fd, csv.data() + off, csv.size() - off);
            if (w <= 0) break;
            off += (size_t)w;
        }
        if (fd < 0 || off < csv.size() || ::close(fd) != 0) {
            std::fflush(stdout);
            std::fprintf(stderr, "sid: --region-stats: could not write %s\n", region_stats_out);
            std::exit(EXIT_FAILURE);
        }
        unsigned long long sites = 0;
        for (size_t k = 0; k < nrows; ++k) sites += (unsigned long long)rows[k].sites;
        return sites;
    };
    // --stats under --region-stats: its two fields (else nothing: the line as it was)
    auto region_stats_json = [&](size_t nrows, unsigned long long sites) {
        char b[96];
        b[0] = 0;
        if (region_stats_out)
            std::snprintf(b, sizeof b, "\"region_rows\": %zu, \"region_sites\": %llu, ", nrows, sites);
        return std::string(b);
    };
    // --callable: the rows as BED, after the records; returns the sum of end - start
    auto write_callable = [&](const sid_callable_row* rows, size_t nrows) {
        size_t need = 0;
        (void)sid_callable_format(rows, nrows, nullptr, 0, &need);
        std::string bed(need, '\0');
        if (need) CHECK(sid_callable_format(rows, nrows, &bed[0], need, &need), "callable");
        const int fd = ::open(callable_out, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        size_t off = 0;
        while (fd >= 0 && off < bed.size()) {
            const ssize_t w = ::write(fd, bed.data() + off, bed.size() - off);
            if (w <= 0) break;
            off += (size_t)w;
        }
        if (fd < 0 || off < bed.size() || ::close(fd) != 0) {
            std::fflush(stdout);
            std::fprintf(stderr, "sid: --callable: could not write %s\n", callable_out);
            std::exit(EXIT_FAILURE);
        }
        unsigned long long sites = 0;
        for (size_t k = 0; k < nrows; ++k) sites += (unsigned long long)(rows[k].end - rows[k].start);
        return sites;
    };
    // --bgzf: the bytes are not BGZF from their first member on / a member further in is truncated or corrupt
    auto bgzf_error = [&](uint64_t off, bool at_index) {
        std::fflush(stdout);
        if (at_index && off == 0) std::fprintf(stderr, "sid: %s: not a BGZF file\n", path);
        else std::fprintf(stderr, "sid: %s: corrupt BGZF block at byte %llu\n", path, (unsigned long long)off);
        std::exit(EXIT_FAILURE);
    };

    // ------------------------------------------------ streaming engine path --
    if (!opt.host_parse) {
        if (!overlap) {
            t0 = now();
            eng_rc = make_engine();
            tc = now();
        }
        CHECK(eng_rc, "engine");
        if (opt.bgzf) {
            uint64_t off = 0;
            const int zrc = pre_map ? sid_engine_source_bgzf(eng, pre_map, in.len, &off)
                            : in.fd >= 0 && !in.data ? sid_engine_source_bgzf_file(eng, in.fd, 0, in.len, &off)
                                                     : sid_engine_source_bgzf(eng, in.data, in.len, &off);
            if (zrc == SID_EBGZF) bgzf_error(off, true);
            CHECK(zrc, "input");
        } else if (pre_map) CHECK(sid_engine_source_text(eng, pre_map, in.len), "input");   // (mapped above)
        else if (in.fd >= 0 && !in.data) CHECK(sid_engine_source_file(eng, in.fd, 0, in.len), "input");
        else CHECK(sid_engine_source_text(eng, in.data, in.len), "input");
        sid_run_stats st;
        std::memset(&st, 0, sizeof st);
        int rc = sid_engine_ingest(eng, &st);
        if (rc == SID_EBGZF) bgzf_error(st.err_offset, false);
        if (rc != SID_OK) on_parse_error(rc);
        uint64_t chunks_stripped = 0, strip_bytes = 0;   // (no fields of sid_run_stats: sid_engine_strip_stats)
        (void)sid_engine_strip_stats(eng, &chunks_stripped, &strip_bytes);
        const double t1 = now();
        rc = sid_engine_estimate(eng, nullptr, &st.estimate);
        if (rc == SID_EEMPTY) {
            std::fflush(stdout);
            std::fputs("sid: no profile with coverage >= 4 (the reference crashes here)\n", stderr);
            std::exit(139);
        }
        if (rc == SID_EBADFUNC) {
            std::fflush(stdout);
            std::fputs("gsl: nmsimplex2.c: ERROR: non-finite function value encountered\n"
                       "Default GSL error handler invoked.\n", stderr);
            std::abort();
        }
        CHECK(rc, "estimate");
        const double t2 = now();
        std::fflush(stdout);
        rc = sid_engine_emit(eng, HEADER, write_all, nullptr, &st);
        if (rc == SID_EIO) std::exit(EXIT_FAILURE);
        CHECK(rc, "emit");
        if (windows_out) {
            const sid_window* rows = nullptr;
            size_t nrows = 0;
            CHECK(sid_engine_windows(eng, &rows, &nrows), "windows");
            write_windows(rows, nrows);
        }
        size_t depth_rows = 0;   // (sid_run_stats has no field for them: its layout stands)
        if (depth_hist_out) {
            const sid_depth_row* rows = nullptr;
            CHECK(sid_engine_depth_hist(eng, &rows, &depth_rows), "depth-hist");
            write_depth_hist(rows, depth_rows);
        }
        size_t region_rows = 0;
        unsigned long long region_sites = 0;
        if (region_stats_out) {
            const sid_region_row* rows = nullptr;
            CHECK(sid_engine_region_stats(eng, &rows, &region_rows), "region-stats");
            region_sites = write_region_stats(rows, region_rows);
        }
        const double t3 = now();
        std::string place;   // per pipeline: its GPU, the CPUs its threads ran on, its pinned buffers' NUMA nodes
        if (opt.stats)
            for (int i = 0; i < sid_engine_devices(eng); ++i) {
                sid_placement pl;
                if (sid_engine_placement(eng, i, &pl) != SID_OK) continue;
                char b[256];
                std::snprintf(b, sizeof b,
                              "%s{\"device\": %d, \"pci\": \"%s\", \"gpu_numa_node\": %d, \"cpus\": %d, "
                              "\"first_cpu\": %d, \"arena_numa_node\": %d, \"ring_numa_node\": %d}",
                              place.empty() ? "" : ", ", pl.device, pl.pci, pl.gpu_numa_node, pl.cpus, pl.first_cpu,
                              pl.arena_numa_node, pl.ring_numa_node);
                place += b;
            }
        if (opt.stats)
            std::fprintf(stderr,
                         "{\"sites\": %llu, \"devices\": %d, \"threads\": %d, \"path\": \"stream\", "
                         "\"create_s\": %.6f, \"parse_s\": %.6f, \"device_s\": %.6f, \"emit_s\": %.6f, \"total_s\": %.6f, "
                         "\"sites_per_s\": %.1f, \"chunks\": %llu, \"chunks_held\": %llu, "
                         "\"chunks_retained\": %llu, \"chunks_reloaded\": %llu, \"bytes_in\": %llu, "
                         "\"bytes_out\": %llu, \"ingest_s\": %.6f, \"chunks_registered\": %llu, "
                         "\"register_s\": %.6f, \"h2d_s\": %.6f, \"h2d_bytes\": %llu, \"chunks_tiled\": %llu, "
                         "\"tile_overflows\": %llu, \"tile_overflows_queued\": %llu, \"bgzf_bytes\": %llu, "
                         "\"bgzf_blocks\": %llu, \"window_rows\": %llu, \"depth_rows\": %llu, \"chunks_stripped\": %llu, "
                         "\"strip_bytes\": %llu, %s\"placement\": [%s], "
                         "\"main_entry_unix\": %.6f, \"main_exit_unix\": %.6f}\n",
                         (unsigned long long)st.sites, D, T, tc - t0, t1 - t0, t2 - t1, t3 - t2, t3 - t0,
                         st.sites / std::max(1e-9, t3 - t0), (unsigned long long)st.chunks,
                         (unsigned long long)st.chunks_held, (unsigned long long)st.chunks_retained,
                         (unsigned long long)st.chunks_reloaded, (unsigned long long)st.bytes_in,
                         (unsigned long long)st.bytes_out, st.ingest_s, (unsigned long long)st.chunks_registered,
                         st.register_s, st.h2d_s, (unsigned long long)st.h2d_bytes,
                         (unsigned long long)st.chunks_tiled, (unsigned long long)st.tile_overflows,
                         (unsigned long long)st.tile_overflows_queued, (unsigned long long)st.bgzf_bytes,
                         (unsigned long long)st.bgzf_blocks, (unsigned long long)st.window_rows,
                         (unsigned long long)depth_rows, (unsigned long long)chunks_stripped,
                         (unsigned long long)strip_bytes, region_stats_json(region_rows, region_sites).c_str(),
                         place.c_str(),
                         t_entry,
                         unix_now());
        // device memory, pinned staging and the mapping go with the process
        finish(0);
    }

    // ------------------------------------------------------ host-parse path --
    t0 = now();
    sid_sites* sites = nullptr;
    size_t n = 0;
    {
        uint64_t bad = 0;
        map_input(in, true);
        if (opt.bgzf) {   // inflated on the host, then as the plain file
            std::string text;
            size_t need = 0;
            uint64_t off = 0;
            int zrc = sid_bgzf_inflate_host(in.data, in.len, nullptr, 0, &need, &off);
            if (zrc == SID_EBGZF) bgzf_error(off, true);
            CHECK(zrc, "input");
            text.resize(need);
            zrc = sid_bgzf_inflate_host(in.data, in.len, &text[0], need, &need, &off);
            if (zrc == SID_EBGZF) bgzf_error(off, false);
            CHECK(zrc, "input");
            if (in.map) munmap(in.map, in.len);
            in.map = nullptr;
            in.owned.swap(text);
            in.data = in.owned.data();
            in.len = in.owned.size();
        }
        int prc = sid_parse_text(in.data, in.len, T, &sites, &bad);
        on_parse_error(prc);
        if (in.map) munmap(in.map, in.len);
        in.map = nullptr;
        n = sid_sites_count(sites);
        const uint16_t* h_counts = sid_sites_counts(sites);
        for (int d = 0; d < D; ++d) {
            sh[d].begin = n * d / D;
            sh[d].end = n * (d + 1) / D;
        }
        parallel([&](int d) {
            make_ctx(d);
            Shard& s = sh[d];
            HCHECK(hipMalloc(&s.d_own_counts, std::max<size_t>(s.end - s.begin, 1) * 8), "device counts");
            s.d_counts = s.d_own_counts;
            if (s.end > s.begin)
                HCHECK(hipMemcpyAsync(s.d_own_counts, h_counts + 4 * s.begin, (s.end - s.begin) * 8,
                                      hipMemcpyHostToDevice, s.stream),
                       "H2D");
            alloc_out(s);
            HCHECK(hipStreamSynchronize(s.stream), "H2D");
        });
    }
    double t1 = now();

    // -------------------------------------------------------------- compute --
    if (lynch) {
        parallel([&](int d) {
            Shard& s = sh[d];
            (void)hipSetDevice(d % ndev);
            CHECK(sid_profile_reset(s.ctx, s.stream), "histogram");
            CHECK(sid_profile_accumulate(s.ctx, s.d_counts, s.end - s.begin, s.stream), "histogram");
        });
        // merge the per-device histograms (the single exchange of the path)
        std::vector<uint64_t> keys, cnts;
        for (int d = 0; d < D; ++d) {
            (void)hipSetDevice(d % ndev);
            size_t u = 0;
            CHECK(sid_profile_table(sh[d].ctx, nullptr, nullptr, 0, &u), "profile table");
            size_t at = keys.size();
            keys.resize(at + u);
            cnts.resize(at + u);
            CHECK(sid_profile_table(sh[d].ctx, keys.data() + at, cnts.data() + at, u, &u), "profile table");
        }
        std::vector<int> rcs(D, SID_OK);
        std::vector<sid_estimate> est(D);
        auto prep = [&](int d) {
            (void)hipSetDevice(d % ndev);
            if (D > 1) {
                int rc = sid_profile_load(sh[d].ctx, keys.data(), cnts.data(), keys.size());
                if (rc) {
                    rcs[d] = rc;
                    return;
                }
            }
            rcs[d] = sid_lynch_prepare(sh[d].ctx, d == 0, &est[d]);
            if (rcs[d] == SID_OK && method == SID_METHOD_LOCAL)
                rcs[d] = sid_set_prior(sh[d].ctx, est[d].heterozygosity);   // call.cpp:233, :305
        };
        // device 0 prints the reference's diagnostics; the others run the same
        // deterministic estimate silently
        prep(0);
        if (rcs[0] == SID_EEMPTY) {
            std::fflush(stdout);
            std::fputs("sid: no profile with coverage >= 4 (the reference crashes here)\n", stderr);
            std::exit(139);
        }
        if (rcs[0] == SID_EBADFUNC) {
            std::fflush(stdout);
            std::fputs("gsl: nmsimplex2.c: ERROR: non-finite function value encountered\n"
                       "Default GSL error handler invoked.\n", stderr);
            std::abort();
        }
        CHECK(rcs[0], "estimate");
        std::vector<std::thread> th;
        for (int d = 1; d < D; ++d) th.emplace_back(prep, d);
        for (auto& x : th) x.join();
        for (int d = 1; d < D; ++d) CHECK(rcs[d], "estimate");
    }
    parallel([&](int d) {
        Shard& s = sh[d];
        (void)hipSetDevice(d % ndev);
        const size_t m = s.end - s.begin;
        if (method == SID_METHOD_LOCAL)
            CHECK(sid_call_local(s.ctx, s.d_counts, m, s.d_code, s.d_hom, s.d_het, s.stream), "local");
        else
            CHECK(sid_lookup_sites(s.ctx, s.d_counts, m, s.d_code, s.d_hom, s.d_het, s.stream), "lookup");
        HCHECK(hipStreamSynchronize(s.stream), "compute");
    });
    double t2 = now();

    // ----------------------------------------------------------------- emit --
    std::fputs(HEADER, stdout);
    std::fflush(stdout);
    size_t window_rows = 0, depth_rows = 0, callable_rows = 0, region_rows = 0;
    unsigned long long callable_sites = 0, region_sites = 0;
    {
        uint8_t* h_code = nullptr;
        double *h_hom = nullptr, *h_het = nullptr;
        const size_t nn = std::max<size_t>(n, 1);
        if (hipHostMalloc((void**)&h_code, nn, hipHostMallocDefault) != hipSuccess) h_code = (uint8_t*)std::malloc(nn);
        if (hipHostMalloc((void**)&h_hom, nn * 8, hipHostMallocDefault) != hipSuccess) h_hom = (double*)std::malloc(nn * 8);
        if (hipHostMalloc((void**)&h_het, nn * 8, hipHostMallocDefault) != hipSuccess) h_het = (double*)std::malloc(nn * 8);
        (void)hipGetLastError();   // a failed pinning above falls back to malloc: not an error
        parallel([&](int d) {
            Shard& s = sh[d];
            (void)hipSetDevice(d % ndev);
            const size_t m = s.end - s.begin;
            if (m) {
                HCHECK(hipMemcpyAsync(h_code + s.begin, s.d_code, m, hipMemcpyDeviceToHost, s.stream), "D2H");
                HCHECK(hipMemcpyAsync(h_hom + s.begin, s.d_hom, m * 8, hipMemcpyDeviceToHost, s.stream), "D2H");
                HCHECK(hipMemcpyAsync(h_het + s.begin, s.d_het, m * 8, hipMemcpyDeviceToHost, s.stream), "D2H");
            }
            HCHECK(hipStreamSynchronize(s.stream), "D2H");
        });
        sid_window* wrows = nullptr;   // --windows: from the codes before the selections mark them
        size_t nwrows = 0;
        if (windows_out) CHECK(sid_windows_host(sites, 0, n, h_code, opt.o.window, &wrows, &nwrows), "windows");
        window_rows = nwrows;
        sid_depth_row* drows = nullptr;   // --depth-hist: likewise
        size_t ndrows = 0;
        if (depth_hist_out) CHECK(sid_depth_hist_host(sites, 0, n, h_code, &drows, &ndrows), "depth-hist");
        depth_rows = ndrows;
        sid_region_row* rrows = nullptr;   // --region-stats: likewise
        size_t nrrows = 0;
        if (region_stats_out)
            CHECK(sid_region_stats_host(regions, sites, 0, n, h_code, &rrows, &nrrows), "region-stats");
        region_rows = nrrows;
        sid_callable_row* crows = nullptr;   // --callable: likewise, under the depth bounds
        size_t ncrows = 0;
        if (callable_out)
            CHECK(sid_callable_host(sites, 0, n, h_code, min_depth, max_depth, &crows, &ncrows), "callable");
        callable_rows = ncrows;
        std::vector<uint8_t> code_all;   // --context: the codes before the selections marked them
        if (opt.o.context > 0 && (opt.o.select != SID_SELECT_ALL || regions || opt.o.variants || depth_on))
            code_all.assign(h_code, h_code + n);
        CHECK(sid_select_mark(h_code, n, opt.o.select), "select");   // --only: the other labels' sites get no record
        CHECK(sid_regions_mark(regions, sites, 0, n, h_code), "regions");   // --regions: nor the sites outside
        if (opt.o.variants) CHECK(sid_variants_mark(sites, 0, n, h_code), "variants");   // --variants: nor the others
        if (depth_on) CHECK(sid_depth_mark(sites, 0, n, min_depth, max_depth, h_code), "depth");   // the depth bounds: nor those outside
        if (!code_all.empty()) CHECK(sid_context_mark(code_all.data(), h_code, n, opt.o.context), "context");
        const size_t BLOCK = 1u << 18;
        const size_t nblocks = (n + BLOCK - 1) / BLOCK;
        std::vector<std::vector<char>> bufs(nblocks);
        std::vector<size_t> lens(nblocks, 0);
        std::vector<std::atomic<int>> ready(nblocks);
        for (auto& r : ready) r.store(0);
        std::atomic<size_t> next{0};
        auto worker = [&] {
            for (;;) {
                size_t b = next.fetch_add(1);
                if (b >= nblocks) return;
                size_t lo = b * BLOCK, hi = std::min(n, lo + BLOCK);
                size_t need = 0;
                if (vcf) sid_format_vcf(sites, lo, hi, h_code, h_hom, h_het, nullptr, 0, &need);
                else sid_format_csv(sites, lo, hi, h_code, h_hom, h_het, conf_type, nullptr, 0, &need);
                bufs[b].resize(need);
                size_t len = 0;
                int rc = vcf ? sid_format_vcf(sites, lo, hi, h_code, h_hom, h_het, bufs[b].data(), need, &len)
                             : sid_format_csv(sites, lo, hi, h_code, h_hom, h_het, conf_type, bufs[b].data(), need, &len);
                lens[b] = rc == SID_OK ? len : 0;
                ready[b].store(1, std::memory_order_release);
            }
        };
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back(worker);
        for (size_t b = 0; b < nblocks; ++b) {
            while (!ready[b].load(std::memory_order_acquire)) std::this_thread::yield();
            size_t off = 0;
            while (off < lens[b]) {
                ssize_t w = ::write(1, bufs[b].data() + off, lens[b] - off);
                if (w <= 0) break;
                off += (size_t)w;
            }
            std::vector<char>().swap(bufs[b]);
        }
        for (auto& x : th) x.join();
        if (windows_out) write_windows(wrows, nwrows);
        sid_windows_free(wrows);
        if (depth_hist_out) write_depth_hist(drows, ndrows);
        sid_depth_hist_free(drows);
        if (region_stats_out) region_sites = write_region_stats(rrows, nrrows);
        sid_region_stats_free(rrows);
        if (callable_out) callable_sites = write_callable(crows, ncrows);
        sid_callable_free(crows);
    }
    double t3 = now();
    if (opt.stats) {
        std::fprintf(stderr,
                     "{\"sites\": %zu, \"devices\": %d, \"threads\": %d, \"path\": \"%s\", \"parse_s\": %.6f, "
                     "\"device_s\": %.6f, \"emit_s\": %.6f, \"total_s\": %.6f, \"sites_per_s\": %.1f, "
                     "\"window_rows\": %zu, \"depth_rows\": %zu, \"callable_rows\": %zu, \"callable_sites\": %llu, %s"
                     "\"main_entry_unix\": %.6f, \"main_exit_unix\": %.6f}\n",
                     n, D, T, "host", t1 - t0, t2 - t1, t3 - t2, t3 - t0,
                     n / std::max(1e-9, t3 - t0), window_rows, depth_rows, callable_rows, callable_sites,
                     region_stats_json(region_rows, region_sites).c_str(), t_entry, unix_now());
    }
    // device memory, pinned staging and mappings go with the process: freeing
    // gigabytes of HBM and pinned host memory one by one only delays the exit
    finish(0);
}
